"""AssignUniqueIdOperator restated in plain Python (AssignUniqueIdOperator.java:115-162): a pool that hands out blocks of 2^20 row ids,
and per operator the counter that walks its current block, row by row as the reference does."""
ROW_IDS_PER_REQUEST = 1 << 20
MAX_ROW_ID = 1 << 40


class LimitExceeded(Exception):
    """checkState(rowIdCounter < MAX_ROW_ID)"""


class Pool:
    def __init__(self, first_value=0):
        self.next = first_value

    def get_and_add(self, n):
        v = self.next
        self.next += n
        return v


class Assigner:
    def __init__(self, pool, stage_id=0, task_id=0):
        self.pool = pool
        self.mask = (stage_id << 54) | (task_id << 40)
        self.request_values()

    def request_values(self):
        self.counter = self.pool.get_and_add(ROW_IDS_PER_REQUEST)
        self.max = min(self.counter + ROW_IDS_PER_REQUEST, MAX_ROW_ID)
        if self.counter >= MAX_ROW_ID:
            raise LimitExceeded()

    def ids(self, position_count):
        out = []
        for _ in range(position_count):
            if self.counter >= self.max:
                self.request_values()
            assert self.counter & self.mask == 0
            out.append(self.mask | self.counter)
            self.counter += 1
        return out
