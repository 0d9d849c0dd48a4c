// C++ driver test of RowNumberOperator through include/presto_amd.hpp (the C++ host mirror), on the GPU:
//   rn-1  TestRowNumberOperator.testRowNumberPartitioned        three pages, BIGINT partition key, cap 10: 4 / 4 / 2 rows numbered in order
//   rn-2  TestRowNumberOperator.testRowNumberPartitionedLimit   the same pages, cap 3: 8 rows, 3 / 3 / 2 per partition
//   rn-3  TestRowNumberOperator.testRowNumberUnpartitionedLimit no partition channels, cap 3: the first 3 rows, then finished
//   a VARCHAR partition key with NULLs, no cap.
// Built by __graft_entry__.build(); executed by tests/test_gpu_row_number.py.  Exit code 0 = all cases pass.
#include <cstdio>
#include <map>

#include "presto_amd.hpp"

using namespace presto_amd;

static int failures = 0;
#define EXPECT(cond, ...)                              \
    do {                                               \
        if (!(cond)) {                                 \
            failures++;                                \
            fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
            fprintf(stderr, __VA_ARGS__);              \
            fprintf(stderr, "\n");                     \
        }                                              \
    } while (0)

// the input of the reference's four cases: (BIGINT key, DOUBLE value), three pages
static std::vector<Page> katPages()
{
    return {Page({Block::bigint({1, 2, 3, 3}), Block::doubles({0.3, 0.2, 0.1, 0.19})}), Page({Block::bigint({1}), Block::doubles({0.4})}),
            Page({Block::bigint({1, 1, 2, 2, 2}), Block::doubles({0.5, 0.6, 0.7, 0.8, 0.9})})};
}

struct Row {
    double value;
    int64_t key, rn;
};
static std::vector<Row> rowsOf(const std::vector<Page>& out)
{
    std::vector<Row> rows;
    for (const auto& p : out) {
        EXPECT(p.getChannelCount() == 3, "channels %d", p.getChannelCount());
        for (int32_t i = 0; i < p.getPositionCount(); i++) {
            EXPECT(p.getBlock(2).type == PA_BIGINT && !p.getBlock(2).isNull(i), "row number block");
            rows.push_back(Row{p.getBlock(0).getDouble(i), p.getBlock(1).getLong(i), p.getBlock(2).getLong(i)});
        }
    }
    return rows;
}

static void testPartitioned(int64_t cap, size_t expectedRows)
{
    auto op = createRowNumberOperator({PA_BIGINT, PA_DOUBLE}, {1, 0}, {0}, cap, -1, 10);
    auto rows = rowsOf(runDriver(katPages(), {op.get()}));
    EXPECT(rows.size() == expectedRows, "cap %ld: %zu rows", (long)cap, rows.size());
    // in arrival order every partition counts 1, 2, 3, ... up to the cap
    std::map<int64_t, int64_t> next;
    const double order[3][4] = {{0.3, 0.4, 0.5, 0.6}, {0.2, 0.7, 0.8, 0.9}, {0.1, 0.19, 0, 0}};
    for (const Row& r : rows) {
        const int64_t want = ++next[r.key];
        EXPECT(r.rn == want && want <= cap, "cap %ld key %ld: row number %ld, expected %ld", (long)cap, (long)r.key, (long)r.rn, (long)want);
        EXPECT(r.value == order[r.key - 1][want - 1], "cap %ld key %ld rn %ld: value %g", (long)cap, (long)r.key, (long)want, r.value);
    }
    EXPECT(next[1] == std::min<int64_t>(4, cap) && next[2] == std::min<int64_t>(4, cap) && next[3] == 2, "cap %ld: rows per partition", (long)cap);
    EXPECT(rowNumberPartitionCount(*op) == 3, "partitions %ld", (long)rowNumberPartitionCount(*op));
}

static void testUnpartitionedLimit()
{
    auto op = createRowNumberOperator({PA_BIGINT, PA_DOUBLE}, {1, 0}, {}, 3, -1, 10);
    auto rows = rowsOf(runDriver(katPages(), {op.get()}));
    EXPECT(rows.size() == 3, "rn-3: %zu rows", rows.size());
    const double values[3] = {0.3, 0.2, 0.1};
    for (size_t i = 0; i < rows.size() && i < 3; i++)
        EXPECT(rows[i].rn == (int64_t)i + 1 && rows[i].value == values[i] && rows[i].key == (int64_t)i + 1, "rn-3 row %zu: %g %ld %ld", i, rows[i].value,
               (long)rows[i].key, (long)rows[i].rn);
    EXPECT(op->isFinished(), "rn-3: finished once the cap is reached");
}

static void testVarcharKeys()
{
    Block keys = Block::varchar({"a", "", "a", "", "bb", "", "bb"});
    keys.nulls = {0, 0, 0, 1, 0, 1, 0};   // "" and NULL are different partitions
    auto op = createRowNumberOperator({PA_VARCHAR, PA_BIGINT}, {0, 1}, {0});
    auto out = runDriver({Page({keys, Block::bigint({0, 1, 2, 3, 4, 5, 6})})}, {op.get()});
    std::vector<int64_t> got;
    for (const auto& p : out)
        for (int32_t i = 0; i < p.getPositionCount(); i++) got.push_back(p.getBlock(2).getLong(i));
    EXPECT(got == std::vector<int64_t>({1, 1, 2, 1, 1, 2, 2}), "varchar row numbers: %zu rows", got.size());
}

int main()
{
    try {
        check(pa_init(0));
        testPartitioned(10, 10);
        testPartitioned(3, 8);
        testUnpartitionedLimit();
        testVarcharKeys();
        pa_shutdown();
    }
    catch (const std::exception& e) {
        fprintf(stderr, "exception: %s\n", e.what());
        return 2;
    }
    if (failures) {
        fprintf(stderr, "%d failure(s)\n", failures);
        return 1;
    }
    printf("row number ok\n");
    return 0;
}
