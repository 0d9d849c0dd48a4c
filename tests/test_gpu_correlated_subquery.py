"""The operator chain every decorrelated scalar subquery is planned as, on the device from end to end:
    SELECT k, x FROM t1 WHERE x < (SELECT avg(y) FROM t2 WHERE t2.k = t1.k)
  = AssignUniqueId(t1) -> LookupJoin PROBE_OUTER against HashBuilder(t2) -> StreamingAggregation grouped by (k, x, unique id) with
    avg(y), count(y) -> FilterAndProject x < avg.
The join keeps probe order, so the rows of one id arrive next to each other.  The result is compared exactly with two nested loops."""
import numpy as np
import pytest

from presto_amd import abi
from presto_amd.expr import call, field
from presto_amd.operators import (AssignUniqueIdOperator, Driver, FilterAndProjectOperator, HashBuilderOperator, LookupJoinOperator, LookupSourceFactory,
                                  StreamingAggregationOperator, to_pages)
from tests import agg_model as A

pytestmark = pytest.mark.gpu
B, D = abi.BIGINT, abi.DOUBLE


def page_of(types, rows):
    from presto_amd.page import Page
    return Page([A.block_of(t, [r[c] for r in rows]) for c, t in enumerate(types)], len(rows))


def tables():
    rng = np.random.default_rng(21)
    build = []
    for k in range(400):
        for _ in range(int(rng.integers(0, 6))):       # 0 .. 5 matches per key
            build.append((k, None if rng.random() < 0.1 else float(rng.integers(-40, 40)) / 4))      # quarters: every sum is exact
    build += [(None, 1.0), (None, 2.0)]                # a NULL key matches nothing
    order = rng.permutation(len(build))
    build = [build[i] for i in order]
    probe = [(None if rng.random() < 0.02 else int(rng.integers(0, 450)), float(rng.integers(-40, 40)) / 4) for _ in range(3000)]
    return probe, build


def nested_loops(probe, build):
    out = []
    for k, x in probe:
        ys = [y for bk, y in build if k is not None and bk == k and y is not None]
        if not ys:
            continue                                   # avg over no row is NULL: x < NULL is not true
        s = 0.0
        for y in ys:
            s += y
        avg = s / float(len(ys))
        if x < avg:
            out.append((k, x, avg, len(ys)))
    return out


@pytest.mark.parametrize("mem", [abi.MEM_HOST, abi.MEM_DEVICE], ids=["host_pages", "device_pages"])
@pytest.mark.parametrize("page_rows", [3000, 700, 1])
def test_scalar_subquery_chain(gpu, mem, page_rows):
    probe, build = tables()
    if page_rows == 1:
        probe = probe[:300]
    bridge = LookupSourceFactory()
    to_pages(HashBuilderOperator(bridge, [B, D], [0], [1]), [page_of([B, D], build[:len(build) // 2]), page_of([B, D], build[len(build) // 2:])])
    operators = [
        AssignUniqueIdOperator([B, D], stage_id=2, task_id=3, output_mem=mem),                                         # -> k, x, id
        LookupJoinOperator(bridge, [B, D, B], [0], [0, 1, 2], output_mem=mem, join_type=abi.JOIN_PROBE_OUTER),         # -> k, x, id, y
        StreamingAggregationOperator([B, D, B, D], [0, 1, 2], [(abi.AGG_AVG, 3, D), (abi.AGG_COUNT, 3, D)], output_mem=mem),   # -> k, x, id, avg, count
        FilterAndProjectOperator([B, D, B, D, B], call(abi.OP_LESS_THAN, abi.BOOLEAN, field(1, D), field(3, D)),
                                 [field(0, B), field(1, D), field(3, D), field(4, B), field(2, B)], output_mem=abi.MEM_HOST),
    ]      # (the last operator hands out host pages: the Driver collects them, and a device page is its operator's again with the next call)
    pages = [page_of([B, D], probe[at:at + page_rows]) for at in range(0, len(probe), page_rows)]
    out = Driver(pages, operators).run()
    rows = [r for p in out for r in p.to_rows()]
    for op in operators:
        op.close()
    assert [r[:4] for r in rows] == nested_loops(probe, build)
    # every surviving row still carries the id AssignUniqueId gave its probe row: ascending, with the stage and task bits
    ids = [r[4] for r in rows]
    assert ids == sorted(set(ids)) and all(i >> 40 == (2 << 14) | 3 for i in ids)
