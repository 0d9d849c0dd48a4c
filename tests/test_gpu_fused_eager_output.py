"""The fused aggregation's eager result ("Results ready at finish"): finish() enqueues the control block and the
small result behind the operator's last launch, getOutput waits for the operator's own event and validates what landed, close waits
for that event and not for the stream other operators share; the few-groups tier's control-block copies and the result's own copies
run on the operator's second stream.

Every case runs twice -- as built, and with PRESTO_AMD_EAGER_OUTPUT=0 (nothing enqueued at finish: the earlier path) -- and both legs
are compared with the oracle.  The legs are compared with each other bit for bit where the tier is reproducible (ungrouped: slab
merges in launch order; few groups: per-wave tables merged in a fixed order at a fixed grid), and to 1e-9 relative where rows pass
through the atomic tiers (tests/test_gpu_packed_keys.py gives the reason).  No case asserts a time."""
import ctypes as C

import numpy as np
import pytest

from presto_amd import _lib, abi, tpch
from presto_amd.expr import field
from presto_amd.operators import FusedAggregationOperator, FusedAggregationOperatorFactory, upload_page
from presto_amd.page import Block, Page
from tests.test_gpu_packed_keys import VV, bits, expected_rows, vv_page
from tests.util import rows_equal_ignore_order

pytestmark = pytest.mark.gpu
REL = 1e-9
EAGER_GROUPS = 1024   # FusedAggregationOperator::kEagerGroups (op_fused.hpp)
Q6_AGGS = tpch.Q6_AGGREGATES + [(abi.AGG_COUNT_STAR, -1, None)]
KV_TYPES = [abi.BIGINT, abi.BIGINT]
KV = dict(types=KV_TYPES, params=None, filter=None, proj=[field(i, t) for i, t in enumerate(KV_TYPES)], group_by=[0],
          aggs=[(abi.AGG_SUM, 1, abi.BIGINT), (abi.AGG_COUNT_STAR, -1, None)])


def operator(shape, **kw):
    return FusedAggregationOperator(shape["types"], shape["filter"], shape["proj"], shape["group_by"], shape["aggs"], type_params=shape["params"], **kw)


def q6_operator(**kw):
    return FusedAggregationOperator(tpch.Q6_TYPES, tpch.q6_filter(), tpch.q6_projections(), [], Q6_AGGS, **kw)


def q1_operator(**kw):
    return FusedAggregationOperator(tpch.Q1_TYPES, tpch.q1_filter(), tpch.q1_projections(), tpch.Q1_GROUP_BY, tpch.Q1_AGGREGATES,
                                    type_params=tpch.Q1_TYPE_PARAMS, **kw)


def drive(op, pages):
    """addInput per page (polling needsInput as a Driver does), finish, getOutput until finished, close: the operator's rows"""
    try:
        for p in pages:
            op.addInput(p)
        op.finish()
        rows = []
        for _ in range(1 << 20):
            if op.isFinished():
                break
            out = op.getOutput()
            if out is not None:
                rows += out.to_rows()
        assert op.isFinished()
        return rows
    finally:
        op.close()


def both_legs(monkeypatch, run):
    """run() as built (the eager result) and with the switch off; the switch is read when an operator is made"""
    monkeypatch.delenv("PRESTO_AMD_EAGER_OUTPUT", raising=False)
    eager = run()
    monkeypatch.setenv("PRESTO_AMD_EAGER_OUTPUT", "0")
    legacy = run()
    monkeypatch.delenv("PRESTO_AMD_EAGER_OUTPUT", raising=False)
    return eager, legacy


def hip_error_left():
    """hipGetLastError of this thread (0 = none); the runtime is the one the library has loaded"""
    try:
        return C.CDLL("libamdhip64.so").hipGetLastError()
    except OSError:
        return 0


@pytest.fixture(scope="module")
def lineitem(gpu, oracle):
    """2^22 + 3 lineitem rows on the device (Q1's columns, which include Q6's) and the oracle's Q6 over all of them, its Q1 over the
    first 2^22 and over the first 2^21 -- computed once, read by every case below"""
    n, sf = (1 << 22) + 3, 1.0
    cols = {c: oracle.tpch_column(c, sf, 0, n) for c in tpch.Q1_COLUMNS}

    def q1(rows):
        c = [(v[:rows], o) if o is None else (v[:rows], o[:rows + 1]) for v, o in (cols[k] for k in tpch.Q1_COLUMNS)]
        return sorted(oracle.q1([c[0][0], c[0][1], c[1][0], c[1][1]] + [x[0] for x in c[2:]]))

    return dict(n=n, sf=sf, dev=tpch.DeviceColumns(tpch.Q1_COLUMNS, sf, n), q6=oracle.q6(*(cols[c][0] for c in tpch.Q6_COLUMNS)),
                q1_22=q1(1 << 22), q1_21=q1(1 << 21))


def sub_pages(dev, columns, bounds):
    """stable device pages over row ranges of the table's columns"""
    sub = tpch.DeviceColumns.__new__(tpch.DeviceColumns)
    sub.columns, sub.rows, sub._bufs = columns, dev.rows, dev._bufs
    return [sub.page(lo, hi - lo) for lo, hi in zip(bounds[:-1], bounds[1:])]


def check_q1(rows, expected):
    rows = sorted(rows)
    assert len(rows) == len(expected)
    for a, e in zip(rows, expected):
        assert a[:2] == e[:2] and a[-1] == e[-1], (a, e)
        assert np.allclose(a[2:-1], e[2:-1], rtol=REL, atol=0), (a, e)


# ---- ungrouped -------------------------------------------------------------------------------------------------------------------
def test_ungrouped_without_a_page(gpu, monkeypatch):
    eager, legacy = both_legs(monkeypatch, lambda: drive(q6_operator(), []))
    assert eager == legacy == [(None, 0)]   # DoubleSumAggregation.output: NULL without input; count(*) = 0


@pytest.mark.parametrize("n", [1, 259])
def test_ungrouped_small_pages(gpu, oracle, monkeypatch, n):
    """1 row: the scalar tail alone; 259 rows: vector head plus tail"""
    cols = [oracle.tpch_column(c, 0.1, 0, n)[0] for c in tpch.Q6_COLUMNS]
    cols[0][:] = 8800   # (a ship date inside Q6's year: discount and quantity alone decide)
    ref_sum, ref_count = oracle.q6(*cols)
    host = Page([Block.flat(t, c) for t, c in zip(tpch.Q6_TYPES, cols)], n)
    eager, legacy = both_legs(monkeypatch, lambda: drive(q6_operator(), [upload_page(host)]))
    assert bits(eager) == bits(legacy)
    (revenue, count), = eager
    assert count == ref_count
    assert (revenue is None) if ref_count == 0 else abs(revenue - ref_sum) <= REL * abs(ref_sum)


def test_ungrouped_staged_kernel_over_two_pages(gpu, lineitem, monkeypatch):
    """2^22 + 3 rows as a page of 2^22 rows (a launch of its own: the staged kernel takes launches from 2^22 rows on) and one of 3 rows
    (launched at finish): two launches, two slab merges in front of the result's copies"""
    monkeypatch.setenv("PRESTO_AMD_GATHER_ROWS", str(1 << 22))
    names = []

    def run():
        op = q6_operator()
        pages = sub_pages(lineitem["dev"], tpch.Q6_COLUMNS, [0, 1 << 22, lineitem["n"]])
        try:
            op.addInput(pages[0])
            names.append(op.kernelName())   # (the first page's launch; the rows behind it go out as a table of ranges at finish)
            op.addInput(pages[1])
            op.finish()
            return op.getOutput().to_rows()
        finally:
            op.close()

    eager, legacy = both_legs(monkeypatch, run)
    assert bits(eager) == bits(legacy)
    assert all(n.startswith("pa_fused_global_staged_") for n in names), names
    ref_sum, ref_count = lineitem["q6"]
    (revenue, count), = eager
    assert count == ref_count and abs(revenue - ref_sum) <= REL * abs(ref_sum)


# ---- grouped, few groups ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", [abi.STEP_SINGLE, abi.STEP_PARTIAL])
@pytest.mark.parametrize("n", [3, 256 + 3])
def test_few_groups_small_pages(gpu, oracle, monkeypatch, n, step):
    """3 rows: the tail launch alone; 256 + 3: head and tail.  PARTIAL: the states a rank hands to the FINAL operator --
    (keys, [count, sum] of sum, [count, sum] of avg, count) -- checked against the oracle's final values"""
    page = vv_page(n, n, k0=b"AN", k1=b"FO")
    expected = expected_rows(oracle, VV, [page])
    eager, legacy = both_legs(monkeypatch, lambda: drive(operator(VV, step=step), [upload_page(page)]))
    assert bits(eager) == bits(legacy)
    if step == abi.STEP_PARTIAL:
        eager = [(k0, k1, s, s2 / c2, c3) for k0, k1, c1, s, c2, s2, c3 in eager]
    rows_equal_ignore_order(eager, expected, rel=REL)


@pytest.mark.parametrize("step", [abi.STEP_SINGLE, abi.STEP_PARTIAL])
def test_few_groups_two_device_pages_confirmed_late(gpu, lineitem, monkeypatch, step):
    """Q1 over two stable device pages of 2^20 rows -- rows [0, 2^20) of the table and rows [2^20, 2^21) generated into buffers of their
    own, so that the second page does not continue the first and is launched apart from it.  Launches over pages that stay readable
    are confirmed late -- at the latest by getOutput, behind the operator's event -- and their control blocks come from the second
    stream."""
    n = 1 << 20
    second = tpch.DeviceColumns(tpch.Q1_COLUMNS, lineitem["sf"], n, first_row=n)
    pages = sub_pages(lineitem["dev"], tpch.Q1_COLUMNS, [0, n]) + [second.page(0, n)]
    eager, legacy = both_legs(monkeypatch, lambda: drive(q1_operator(step=step), pages))
    assert bits(eager) == bits(legacy)
    if step == abi.STEP_PARTIAL:
        # (keys, then [count, sum] per sum / avg, then count(*)) -> Q1's final row
        eager = [(r[0], r[1], r[3], r[5], r[7], r[9], r[11] / r[10], r[13] / r[12], r[15] / r[14], r[16]) for r in eager]
    check_q1(eager, lineitem["q1_21"])


def test_grouped_empty_input_returns_nothing(gpu, monkeypatch):
    eager, legacy = both_legs(monkeypatch, lambda: drive(operator(VV), []))
    assert eager == legacy == []
    # ... and pages whose rows all fail the filter: the table exists, no group does
    page = upload_page(vv_page(1000, 1, dates=10_000))
    eager, legacy = both_legs(monkeypatch, lambda: drive(operator(VV), [page]))
    assert eager == legacy == []


# ---- speculation refused ---------------------------------------------------------------------------------------------------------
def test_refused_register_table_overflow_found_at_confirmation(gpu, oracle, monkeypatch):
    """Nine groups in a stable device page of 2^20 rows: the wave's register table (8 groups) overflows.  Once the plan is known to
    fit the few-groups tier (the first operator below tells), the page goes out whole and unconfirmed, finish() enqueues the result
    on that guess, and getOutput finds the overflow, redoes the rows on the next tier and drops the eager result."""
    few = vv_page(5000, 7)
    page = vv_page(1 << 20, 9, k0=b"ANR", k1=b"FOX")
    expected = expected_rows(oracle, VV, [page])
    dev = upload_page(page)
    stable = Page(dev.blocks, page.position_count, abi.MEM_DEVICE, stable=True)

    def run():
        drive(operator(VV), [upload_page(few)])
        return drive(operator(VV), [stable])

    eager, legacy = both_legs(monkeypatch, run)
    rows_equal_ignore_order(eager, legacy, rel=REL)
    rows_equal_ignore_order(eager, expected, rel=REL)
    rows_equal_ignore_order(legacy, expected, rel=REL)


def test_refused_one_group_more_than_the_eager_bound(gpu, oracle, monkeypatch):
    """BIGINT keys 0 .. bound in one page: bound + 1 groups, one more than finish() copies rows for"""
    n = 4 * (EAGER_GROUPS + 1)
    rng = np.random.default_rng(11)
    keys = np.arange(n, dtype=np.int64) % (EAGER_GROUPS + 1)
    page = Page([Block.bigint(keys), Block.bigint(rng.integers(-1000, 1000, n))], n)
    expected = expected_rows(oracle, KV, [page])
    assert len(expected) == EAGER_GROUPS + 1
    for groups_hint in (8, 10000):   # (expected_groups is a hint: the result may not depend on it)
        eager, legacy = both_legs(monkeypatch, lambda: drive(operator(KV, expected_groups=groups_hint), [upload_page(page)]))
        assert sorted(eager) == sorted(legacy) == sorted(expected)   # integer sums: exact on every tier
    # ... and exactly the bound: the eager result holds
    keys = np.arange(n, dtype=np.int64) % EAGER_GROUPS
    page = Page([Block.bigint(keys), Block.bigint(rng.integers(-1000, 1000, n))], n)
    eager, legacy = both_legs(monkeypatch, lambda: drive(operator(KV), [upload_page(page)]))
    assert sorted(eager) == sorted(legacy) == sorted(expected_rows(oracle, KV, [page]))


# ---- two operators on one stream, as bench.py drives them ------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["outputs then closes", "close A without its output", "close B after finish"])
def test_two_operators_on_one_stream(gpu, lineitem, monkeypatch, order):
    """A: pages, finish; B: pages, finish; getOutput(A), close(A), getOutput(B), close(B) -- B Q1-shaped over 2^22 rows, A Q6-shaped over the
    same rows, both on one stream handed in.  close(A) must not wait for B's kernels, and may not hand A's buffers back while A's own
    work is pending: a fresh operator made afterwards on the same stream, which takes those buffers from the pool, computes a right
    result."""
    dev = lineitem["dev"]
    # (a page of 2^21 rows is launched on its own at this threshold, the two behind it together at finish: two launches per operator)
    monkeypatch.setenv("PRESTO_AMD_GATHER_ROWS", str(1 << 21))
    bounds = [0, 1 << 21, (1 << 22) - 256, 1 << 22]
    q6_sum, q6_count = None, None

    def run():
        stream = _lib.DeviceStream()
        a = FusedAggregationOperatorFactory(tpch.Q6_TYPES, tpch.q6_filter(), tpch.q6_projections(), [], Q6_AGGS, stream=stream.handle).createOperator()
        b = FusedAggregationOperatorFactory(tpch.Q1_TYPES, tpch.q1_filter(), tpch.q1_projections(), tpch.Q1_GROUP_BY, tpch.Q1_AGGREGATES,
                                            type_params=tpch.Q1_TYPE_PARAMS, stream=stream.handle).createOperator()
        out = {}
        try:
            for op, columns in ((a, tpch.Q6_COLUMNS), (b, tpch.Q1_COLUMNS)):
                for p in sub_pages(dev, columns, bounds):
                    op.addInput(p)
                op.finish()
            if order == "close B after finish":
                b.close()
            if order != "close A without its output":
                out["a"] = a.getOutput().to_rows()
            a.close()
            if order != "close B after finish":
                out["b"] = b.getOutput().to_rows()
            b.close()
            # reuse after close: the pooled buffers of A and B go to a fresh operator on the same stream
            c = FusedAggregationOperatorFactory(tpch.Q1_TYPES, tpch.q1_filter(), tpch.q1_projections(), tpch.Q1_GROUP_BY, tpch.Q1_AGGREGATES,
                                                type_params=tpch.Q1_TYPE_PARAMS, stream=stream.handle).createOperator()
            out["c"] = drive(c, sub_pages(dev, tpch.Q1_COLUMNS, [0, 1 << 21]))
            assert hip_error_left() == 0
            return out
        finally:
            a.close()
            b.close()
            stream.synchronize()
            stream.destroy()

    eager, legacy = both_legs(monkeypatch, run)
    for leg in (eager, legacy):
        if "a" in leg:
            (revenue, count), = leg["a"]
            assert q6_count in (None, count) and q6_sum in (None, revenue)   # the same bytes in both legs
            q6_sum, q6_count = revenue, count
        if "b" in leg:
            check_q1(leg["b"], lineitem["q1_22"])
        check_q1(leg["c"], lineitem["q1_21"])
    if "b" in eager:
        assert bits(eager["b"]) == bits(legacy["b"])
    assert bits(eager["c"]) == bits(legacy["c"])


def test_q6_over_the_first_rows_matches_the_oracle(gpu, oracle, lineitem, monkeypatch):
    """(the reference for A above: Q6 over rows [0, 2^22), in the launches test_two_operators_on_one_stream makes)"""
    n = 1 << 22
    cols = [oracle.tpch_column(c, lineitem["sf"], 0, n)[0] for c in tpch.Q6_COLUMNS]
    ref_sum, ref_count = oracle.q6(*cols)
    monkeypatch.setenv("PRESTO_AMD_GATHER_ROWS", str(1 << 21))
    eager, legacy = both_legs(monkeypatch, lambda: drive(q6_operator(), sub_pages(lineitem["dev"], tpch.Q6_COLUMNS, [0, 1 << 21, n - 256, n])))
    assert bits(eager) == bits(legacy)
    (revenue, count), = eager
    assert count == ref_count and abs(revenue - ref_sum) <= REL * abs(ref_sum)


# ---- fifty operator lives in a row on one stream ---------------------------------------------------------------------------------
def test_fifty_operator_lives_on_one_stream(gpu, lineitem):
    """A fresh Q1 and a fresh Q6 operator per life, as a bench step makes them: the same bytes every time, and once both are closed the
    pool has all its HBM back (pa_memory_stats' bytes in use are what they were after the first life)."""
    stream = _lib.DeviceStream()
    dev = lineitem["dev"]
    f6 = FusedAggregationOperatorFactory(tpch.Q6_TYPES, tpch.q6_filter(), tpch.q6_projections(), [], Q6_AGGS, stream=stream.handle)
    f1 = FusedAggregationOperatorFactory(tpch.Q1_TYPES, tpch.q1_filter(), tpch.q1_projections(), tpch.Q1_GROUP_BY, tpch.Q1_AGGREGATES,
                                         type_params=tpch.Q1_TYPE_PARAMS, stream=stream.handle)
    p6 = sub_pages(dev, tpch.Q6_COLUMNS, [0, 1 << 19, 1 << 20])
    p1 = sub_pages(dev, tpch.Q1_COLUMNS, [0, 1 << 19, 1 << 20])

    def in_use():
        used, cached, limit = C.c_int64(), C.c_int64(), C.c_int64()
        _lib.check(_lib.lib().pa_memory_stats(C.byref(used), C.byref(cached), C.byref(limit)))
        return used.value

    first, before = None, None
    for life in range(50):
        ops = []
        for f, pages in ((f1, p1), (f6, p6)):
            op = f.createOperator()
            for p in pages:
                op.addInput(p)
            op.finish()
            ops.append(op)
        got = []
        for op in ops:
            got.append(bits(op.getOutput().to_rows()))
            op.kernelTime()
            op.close()
        if first is None:   # (the first life of a process also makes what the plan's operators share: the word-kind tables)
            first, before = got, in_use()
        assert got == first, life
        assert in_use() == before, life
    stream.synchronize()
    stream.destroy()
    assert hip_error_left() == 0
