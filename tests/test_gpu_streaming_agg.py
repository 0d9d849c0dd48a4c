"""GPU checks of StreamingAggregationOperator against tests/streaming_agg_model.py (runs by IS NOT DISTINCT FROM, tests/agg_model.py per
run): the reference's known answers, the run geometries around tiles and pages, page-cut invariance by bytes, every key type at run
and page boundaries, sum(BIGINT) as Math.addExact in row order, the DOUBLE / REAL edge values, seeded fuzz and a cross-check against the
hash aggregation.  Integer results and everything agg_model.order_free() covers compare exactly; other floating sums within relative
1e-9 of the sequential sum."""
import math
import os
import struct

import numpy as np
import pytest

from presto_amd import abi
from presto_amd._lib import PrestoAmdError
from presto_amd.operators import HashAggregationOperator, StreamingAggregationOperator, download_page, upload_page
from presto_amd.page import Block, Page
from tests import agg_model as A
from tests import streaming_agg_model as S
from tests.test_streaming_agg_cpu import KATS, same_rows

pytestmark = pytest.mark.gpu
FUZZ_SEEDS = int(os.environ.get("PA_FUZZ_SEEDS", "16"))
OUT_OF_RANGE = abi.ERR_NUMERIC_VALUE_OUT_OF_RANGE
NAN = float("nan")
I64_MAX, I64_MIN = 2 ** 63 - 1, -2 ** 63
COUNT_STAR = (abi.AGG_COUNT_STAR, -1, None)
D122 = abi.decimal(12, 2)


def page_of(types, rows):
    return Page([A.block_of(t, [r[c] for r in rows]) for c, t in enumerate(types)], len(rows))


def cut(rows, sizes):
    """rows cut into pages of the given sizes, the last size repeated"""
    out, at, i = [], 0, 0
    while at < len(rows):
        s = sizes[min(i, len(sizes) - 1)]
        out.append(rows[at:at + s])
        at += s
        i += 1
    return out


def host(page):
    return download_page(page) if page.mem == abi.MEM_DEVICE else page


def drive(op, pages, device_input=False):
    """Feeds host pages one by one, following the protocol call by call -> (output pages as host Pages, status of the call that failed or None)."""
    outs = []
    try:
        for page in pages:
            assert op.needsInput() and not op.isFinished()
            op.addInput(upload_page(page) if device_input and page.position_count else page)
            pending = not op.needsInput()            # at most one page: the runs that closed inside the input page
            out = op.getOutput()
            assert (out is not None) == pending
            if out is not None:
                assert out.position_count >= 1
                outs.append(host(out))
            assert op.getOutput() is None and op.needsInput()
        op.finish()
        assert not op.needsInput()
        out = op.getOutput()                          # the run left open, if any row was seen
        if out is not None:
            assert out.position_count == 1
            outs.append(host(out))
        assert op.getOutput() is None and op.isFinished()
    except PrestoAmdError as e:
        assert op.isFinished() and op.getOutput() is None      # nothing is emitted from then on
        return outs, e.status
    return outs, None


def run(types, group, aggs, row_pages, output_mem=abi.MEM_HOST, device_input=False):
    op = StreamingAggregationOperator(types, group, aggs, output_mem=output_mem)
    outs, error = drive(op, [page_of(types, rows) for rows in row_pages], device_input)
    op.close()
    return [r for p in outs for r in p.to_rows()], error, outs


def close_enough(t, got, want, exact):
    if exact or not A.is_fp(t):
        return A.bits(t, got) == A.bits(t, want)
    got, want = float(got), float(want)
    if want != want or math.isinf(want):
        return A.bits(t, got) == A.bits(t, want)
    return abs(got - want) <= 1e-9 * abs(want)


def check_against_model(types, group, aggs, rows, got, error):
    """got / error of an operator over `rows` (however they were cut into pages) against the model"""
    nk = len(group)
    key_types = [types[c] for c in group]
    expected, expected_error = [], None
    for key, results, exact in S.outcomes(rows, types, group, aggs):
        if any(r.row_order[0] == "error" for r in results):
            expected_error = OUT_OF_RANGE
            break
        expected.append((key, results, exact))
    if expected_error is None:
        assert error is None and len(got) == len(expected), (error, len(got), len(expected))
    else:
        assert error == expected_error and len(got) <= len(expected), (error, len(got), len(expected))
    for row, (key, results, exact) in zip(got, expected):
        assert same_rows(key_types, [row[:nk]], [key]), (row, key)
        for a, r, e, v in zip(aggs, results, exact, row[nk:]):
            if r.row_order[0] == "null":
                assert v is None, (a, row)
            else:
                assert v is not None and close_enough(r.type, v, r.row_order[1], e), (a, row, r.row_order)


# ---- the reference's known answers ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("output_mem,device_input", [(abi.MEM_HOST, False), (abi.MEM_DEVICE, False), (abi.MEM_DEVICE, True)])
@pytest.mark.parametrize("name", sorted(KATS))
def test_reference_known_answers(gpu, name, output_mem, device_input):
    types, group, aggs, pages, want = KATS[name]
    got, error, outs = run(types, group, aggs, pages, output_mem, device_input)
    out_types = [types[c] for c in group] + [A.result_type(a[0], a[2]) for a in aggs]
    assert error is None and same_rows(out_types, got, want), (got, want)
    if name == "testEmptyInput":
        assert outs == []


def test_empty_pages_and_protocol(gpu):
    types, aggs = [abi.BIGINT, abi.BIGINT], [(abi.AGG_SUM, 1, abi.BIGINT)]
    op = StreamingAggregationOperator(types, [0], aggs)
    empty = page_of(types, [])
    op.addInput(empty)
    assert op.needsInput() and op.getOutput() is None
    op.addInput(page_of(types, [(1, 2), (1, 3)]))
    assert op.needsInput() and op.getOutput() is None           # no run closed
    op.addInput(empty)                                          # an empty page does not close the open run
    assert op.needsInput() and op.getOutput() is None
    op.addInput(page_of(types, [(1, 4), (2, 1), (3, 1)]))
    assert not op.needsInput()
    with pytest.raises(PrestoAmdError) as e:
        op.addInput(empty)
    assert e.value.status == abi.ERR_ILLEGAL_STATE
    op.finish()
    assert not op.isFinished()
    assert op.getOutput().to_rows() == [(1, 9), (2, 1)]
    assert not op.isFinished()
    assert op.getOutput().to_rows() == [(3, 1)]
    assert op.isFinished() and op.getOutput() is None
    assert op.kernelName() == "k_stream_agg_apply" and op.memoryBytes() > 0
    op.close()


# ---- run geometries -------------------------------------------------------------------------------------------------------------------------
GEOMETRY_TYPES = [abi.BIGINT, abi.BIGINT, abi.BOOLEAN]
GEOMETRY_AGGS = [(abi.AGG_COUNT_STAR, -1, None, 2), (abi.AGG_COUNT, 1, abi.BIGINT), (abi.AGG_SUM, 1, abi.BIGINT, 2), (abi.AGG_MIN, 1, abi.BIGINT, 2),
                 (abi.AGG_MAX, 1, abi.BIGINT)]


def geometry_columns(keys, seed):
    rng = np.random.default_rng(seed)
    n = len(keys)
    values = rng.integers(-1000, 1000, n).astype(np.int64)
    nulls = (rng.random(n) < 0.2).astype(np.uint8)
    mask = (rng.random(n) < 0.7).astype(np.uint8)
    mask_nulls = (rng.random(n) < 0.1).astype(np.uint8)
    return np.asarray(keys, dtype=np.int64), values, nulls, mask, mask_nulls


def numpy_reference(keys, values, nulls, mask, mask_nulls):
    """GEOMETRY_AGGS over runs of equal adjacent keys, by numpy; pinned to the model by test_numpy_reference_is_the_model"""
    n = len(keys)
    starts = np.flatnonzero(np.concatenate(([True], keys[1:] != keys[:-1])))
    masked = (mask != 0) & (mask_nulls == 0)
    present = nulls == 0
    red = lambda x: np.add.reduceat(x.astype(np.int64), starts)
    both = masked & present
    big = np.int64(1 << 40)
    out = {"key": keys[starts], "count_star": red(masked), "count": red(present), "sum": red(np.where(both, values, 0)), "sum_n": red(both),
           "min": np.minimum.reduceat(np.where(both, values, big), starts), "min_n": red(both),
           "max": np.maximum.reduceat(np.where(present, values, -big), starts), "max_n": red(present)}
    assert n == 0 or len(out["key"]) >= 1
    return out


def reference_rows(ref):
    rows = []
    for i in range(len(ref["key"])):
        rows.append((int(ref["key"][i]), int(ref["count_star"][i]), int(ref["count"][i]), int(ref["sum"][i]) if ref["sum_n"][i] else None,
                     int(ref["min"][i]) if ref["min_n"][i] else None, int(ref["max"][i]) if ref["max_n"][i] else None))
    return rows


def geometry_pages(cols, bounds):
    keys, values, nulls, mask, mask_nulls = cols
    pages = []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        pages.append(Page([Block.bigint(keys[lo:hi]), Block.flat(abi.BIGINT, values[lo:hi], nulls[lo:hi]), Block.boolean(mask[lo:hi], mask_nulls[lo:hi])], hi - lo))
    return pages


def run_geometry(keys, bounds, seed=1, device_input=True):
    cols = geometry_columns(keys, seed)
    op = StreamingAggregationOperator(GEOMETRY_TYPES, [0], GEOMETRY_AGGS, output_mem=abi.MEM_DEVICE)
    outs, error = drive(op, geometry_pages(cols, bounds), device_input)
    op.close()
    assert error is None
    return cols, outs


def assert_geometry(keys, bounds, **kw):
    cols, outs = run_geometry(keys, bounds, **kw)
    ref = numpy_reference(*cols)
    got = {name: np.concatenate([p.blocks[c].values[:p.position_count] for p in outs]) for c, name in enumerate(["key", "count_star", "count", "sum", "min", "max"])}
    nulls = {name: np.concatenate([p.blocks[c].nulls[:p.position_count] if p.blocks[c].nulls is not None else np.zeros(p.position_count, np.uint8) for p in outs])
             for c, name in ((3, "sum"), (4, "min"), (5, "max"))}
    for name in ("key", "count_star", "count"):
        assert np.array_equal(got[name], ref[name]), name
    for name in ("sum", "min", "max"):
        has = ref[name + "_n"] > 0
        assert np.array_equal(nulls[name] == 0, has), name
        assert np.array_equal(got[name][has], ref[name][has]), name
    return outs


def test_numpy_reference_is_the_model():
    keys = np.repeat(np.arange(40), np.random.default_rng(3).integers(1, 6, 40))
    cols = geometry_columns(keys, 5)
    k, v, nl, m, mn = cols
    rows = [(int(k[i]), None if nl[i] else int(v[i]), None if mn[i] else bool(m[i])) for i in range(len(k))]
    want, error = S.expected_rows(rows, GEOMETRY_TYPES, [0], GEOMETRY_AGGS)
    assert error is None and reference_rows(numpy_reference(*cols)) == want


def test_every_run_of_length_one(gpu):
    outs = assert_geometry(np.arange(2500), [0, 1100, 1101, 2500])
    assert [p.position_count for p in outs] == [1099, 1, 1399, 1]


def test_one_run_over_all_pages(gpu):
    outs = assert_geometry(np.full(3000, 7), [0, 1024, 1025, 3000])
    assert [p.position_count for p in outs] == [1]


def test_runs_ending_exactly_on_page_ends(gpu):
    outs = assert_geometry(np.arange(4096) // 256, [0, 1024, 2048, 3072, 4096])
    # a run that ends with a page is closed by the first row of the next one
    assert [p.position_count for p in outs] == [3, 4, 4, 4, 1]


@pytest.mark.parametrize("edge", [1023, 1024, 1025])
def test_run_boundary_at_the_tile_edge(gpu, edge):
    keys = np.zeros(2600, dtype=np.int64)
    keys[edge:] = 1
    keys[2048:] = 2
    assert_geometry(keys, [0, 2600])
    assert_geometry(np.concatenate([keys, keys + 3]), [0, 2600, 5200])       # the same edges in a page with a run carried in


@pytest.mark.parametrize("run_length", [3, 0])
def test_tile_state_scan_crosses_its_own_step(gpu, run_length):
    """one page of 2^20 + 1025 rows: more than 1024 tiles, so the scan of the tile states takes a second round"""
    n = (1 << 20) + 1025
    keys = np.arange(n) // run_length if run_length else np.zeros(n, dtype=np.int64)
    outs = assert_geometry(keys, [0, n])
    assert sum(p.position_count for p in outs) == ((n + 2) // 3 if run_length else 1)


# ---- page cuts ------------------------------------------------------------------------------------------------------------------------------
def invariance_rows():
    rng = np.random.default_rng(11)
    lengths = rng.choice([1, 1, 2, 3, 7, 40, 300], 40)
    rows = []
    for g, length in enumerate(lengths):
        zero = -0.0 if g % 2 else 0.0
        for j in range(int(length)):
            key = (zero if j % 2 == 0 else -zero) if g % 3 == 0 else float(g)      # runs that mix the zeros: the key is the first row's
            v = None if rng.random() < 0.15 else float(rng.integers(-64, 64)) / 4
            rows.append((key, b"k%d" % (g // 2), v, int(rng.integers(-5, 5)), bool(rng.random() < 0.8)))
    return rows


def block_bytes(pages):
    """every output column of the concatenated pages as bytes: values, NULL flags, and VARCHAR strings one by one"""
    out = []
    for c in range(pages[0].channel_count):
        vals, nulls = [], []
        for p in pages:
            b, n = p.blocks[c], p.position_count
            nulls.append(bytes(n) if b.nulls is None else bytes(np.asarray(b.nulls[:n], dtype=np.uint8)))
            if b.type == abi.VARCHAR:
                raw, off = b.values.tobytes(), b.offsets
                vals.append(b"|".join(raw[off[i]:off[i + 1]] for i in range(n)) + b"|")
            else:
                nl = np.zeros(n, bool) if b.nulls is None else np.asarray(b.nulls[:n]) != 0
                v = b.values[:n].copy()
                v[nl] = 0            # what stands under a NULL is not part of the result
                vals.append(v.tobytes())
        out.append((b"".join(vals), b"".join(nulls)))
    return out


def test_page_cuts_do_not_change_a_byte(gpu):
    types = [abi.DOUBLE, abi.VARCHAR, abi.DOUBLE, abi.BIGINT, abi.BOOLEAN]
    aggs = [COUNT_STAR, (abi.AGG_SUM, 2, abi.DOUBLE), (abi.AGG_AVG, 2, abi.DOUBLE, 4), (abi.AGG_MIN, 2, abi.DOUBLE), (abi.AGG_SUM, 3, abi.BIGINT), (abi.AGG_AVG, 3, abi.BIGINT)]
    rows = invariance_rows()
    results = []
    for sizes in ([len(rows)], [1], [7], [1024], [1025], [len(rows)]):
        got, error, outs = run(types, [0, 1], aggs, cut(rows, sizes), abi.MEM_DEVICE, device_input=True)
        assert error is None
        results.append(block_bytes(outs))
        if len(results) == 1:
            check_against_model(types, [0, 1], aggs, rows, got, error)
    assert all(r == results[0] for r in results[1:])


# ---- key types --------------------------------------------------------------------------------------------------------------------------------
LONG = b"0123456789abcdef" * 9
KEY_VALUES = {
    abi.BIGINT: [5, 5, None, None, 0, I64_MIN, I64_MIN, I64_MAX, 5],
    abi.INTEGER: [5, 5, None, None, 0, -2 ** 31, -2 ** 31, 2 ** 31 - 1, 5],
    abi.DATE: [5, 5, None, None, 0, -2 ** 31, 7, 7, 5],
    abi.DOUBLE: [0.0, -0.0, 0.0, None, None, NAN, A.NAN_PAYLOAD, A.NAN_NEGATIVE, 1.5, -0.0, 0.0, A.NAN_NEGATIVE, NAN, float("inf"), float("inf")],
    abi.REAL: [np.float32(v) for v in (0.0, -0.0, 0.0)] + [None, None, np.float32(NAN), A.NAN_NEGATIVE_F32, np.float32(1.5), np.float32(-0.0), np.float32(0.0),
                                                              A.NAN_NEGATIVE_F32, np.float32(NAN)],
    abi.BOOLEAN: [True, True, False, None, None, False, False, True],
    abi.VARCHAR: [b"", b"", None, None, b"", LONG, LONG, LONG[:-1], LONG[:-1] + b"g", b"a", b"a", b"", b"\x00", b"\x00"],
    D122: [5, 5, None, None, 0, -10 ** 12 + 1, -10 ** 12 + 1, 10 ** 12 - 1, 5],
}
RAW = {abi.BIGINT: np.int64, abi.INTEGER: np.int32, abi.DATE: np.int32, abi.DOUBLE: np.float64, abi.REAL: np.float32, abi.BOOLEAN: np.uint8, abi.DECIMAL: np.int64}


@pytest.mark.parametrize("t", list(KEY_VALUES), ids=A.label)
def test_key_types_at_run_and_page_boundaries(gpu, t):
    """every boundary between two values -- equal, NULL, the zeros, NaN payloads, strings that differ in length or in their last byte --
    falls once inside a page and once between two pages; the key bits are the first row's"""
    values = KEY_VALUES[t]
    types, aggs = [t, abi.BIGINT], [COUNT_STAR, (abi.AGG_SUM, 1, abi.BIGINT)]
    rows = [(v, i) for i, v in enumerate(values)]
    expected = S.outcomes(rows, types, [0], aggs)
    for sizes in ([len(rows)], [1], [2], [1, 2], [3]):
        got, error, outs = run(types, [0], aggs, cut(rows, sizes), abi.MEM_DEVICE, device_input=sizes != [2])
        check_against_model(types, [0], aggs, rows, got, error)
        # the bits of the key column: not only "a NaN" but the first row's NaN
        firsts = [key[0] for key, _, _ in expected]
        if t == abi.VARCHAR:
            assert [r[0] for r in got] == firsts
            continue
        dt = RAW[int(t)]
        want = np.array([0 if v is None else v for v in firsts], dtype=dt)
        have = np.concatenate([p.blocks[0].values[:p.position_count] for p in outs]).astype(dt, copy=False)
        keep = np.array([v is not None for v in firsts])
        if t == abi.BOOLEAN:
            assert np.array_equal(have[keep] != 0, want[keep] != 0)
        else:
            assert have[keep].tobytes() == want[keep].tobytes(), sizes


def test_several_group_channels(gpu):
    types = [abi.BIGINT, abi.VARCHAR, abi.DOUBLE, abi.BIGINT]
    rows = [(1, b"a", 0.0, 1), (1, b"a", -0.0, 2), (1, b"b", 0.0, 3), (None, b"b", 0.0, 4), (None, b"b", NAN, 5), (None, None, NAN, 6), (None, None, NAN, 7),
            (1, b"a", 0.0, 8)]
    aggs = [(abi.AGG_SUM, 3, abi.BIGINT), (abi.AGG_MAX, 2, abi.DOUBLE)]
    for sizes in ([8], [1], [3], [5]):
        got, error, _ = run(types, [0, 1, 2], aggs, cut(rows, sizes))
        check_against_model(types, [0, 1, 2], aggs, rows, got, error)
        assert [r[3] for r in got] == [3, 3, 4, 5, 13, 8]


# ---- sum(BIGINT): Math.addExact in row order --------------------------------------------------------------------------------------------------
SUM_TYPES, SUM_AGGS = [abi.BIGINT, abi.BIGINT], [(abi.AGG_SUM, 1, abi.BIGINT), COUNT_STAR]
BACK = [(2, I64_MAX), (2, 1), (2, -5)]           # the prefix leaves int64 at the second row and comes back with the third


@pytest.mark.parametrize("sizes", [[9], [2], [3], [1]], ids=lambda s: "pages_of_%d" % s[0])
def test_sum_prefix_that_overflows_and_comes_back(gpu, sizes):
    rows = [(1, 3)] + BACK + [(3, 4), (4, 1)]
    got, error, _ = run(SUM_TYPES, [0], SUM_AGGS, cut(rows, sizes), abi.MEM_DEVICE, device_input=True)
    assert error == OUT_OF_RANGE
    check_against_model(SUM_TYPES, [0], SUM_AGGS, rows, got, error)
    # in an order whose prefixes fit, the same values have a sum
    fits = [(1, 3), (2, I64_MAX), (2, -5), (2, 1), (3, 4), (4, 1)]
    got, error, _ = run(SUM_TYPES, [0], SUM_AGGS, cut(fits, sizes))
    assert error is None and got == [(1, 3, 1), (2, I64_MAX - 4, 3), (3, 4, 1), (4, 1, 1)]


def test_sum_overflow_does_not_depend_on_the_neighbours(gpu):
    for sizes in ([6], [1], [2]):
        # two runs that would overflow as one; a run that reaches both ends of int64; NULL and masked rows repeat the prefix before them
        rows = [(1, I64_MAX), (2, I64_MAX), (3, I64_MIN), (3, None), (3, I64_MAX), (4, I64_MIN)]
        got, error, _ = run(SUM_TYPES, [0], SUM_AGGS, cut(rows, sizes))
        assert error is None and got == [(1, I64_MAX, 1), (2, I64_MAX, 1), (3, -1, 3), (4, I64_MIN, 1)]
        # the run left open fails when finish closes it
        rows = [(1, 5), (2, I64_MIN), (2, -1), (2, 1)]
        got, error, _ = run(SUM_TYPES, [0], SUM_AGGS, cut(rows, sizes))
        assert error == OUT_OF_RANGE and got in ([], [(1, 5, 1)])
        check_against_model(SUM_TYPES, [0], SUM_AGGS, rows, got, error)
    masked = [abi.BIGINT, abi.BIGINT, abi.BOOLEAN]
    rows = [(1, I64_MAX, True), (1, 1, False), (1, 1, None), (1, -1, True), (2, 1, True)]
    got, error, _ = run(masked, [0], [(abi.AGG_SUM, 1, abi.BIGINT, 2)], [rows])
    assert error is None and got == [(1, I64_MAX - 1), (2, 1)]


def test_after_an_error_the_operator_closes_cleanly(gpu):
    op = StreamingAggregationOperator(SUM_TYPES, [0], SUM_AGGS, output_mem=abi.MEM_DEVICE)
    op.addInput(page_of(SUM_TYPES, [(1, 1), (2, I64_MAX)]))
    assert op.getOutput().position_count == 1
    with pytest.raises(PrestoAmdError) as e:
        op.addInput(page_of(SUM_TYPES, [(2, 1), (3, 1)]))
    assert e.value.status == OUT_OF_RANGE
    assert not op.needsInput() and op.getOutput() is None and op.isFinished()
    op.finish()
    assert op.getOutput() is None
    op.close()
    del op


def test_integer_sum_column(gpu):
    types, aggs = [abi.BIGINT, abi.INTEGER], [(abi.AGG_SUM, 1, abi.INTEGER), (abi.AGG_AVG, 1, abi.INTEGER)]
    top = 2 ** 31 - 1
    rows = [(1, top), (1, 1), (1, -1), (2, -top - 1), (2, None), (3, None)]
    got, error, _ = run(types, [0], aggs, cut(rows, [2]))
    check_against_model(types, [0], aggs, rows, got, error)
    assert error is None and got[0][1] == top and got[2][1:] == (None, None)
    rows = [(1, 5), (2, top), (2, 1), (3, 1)]
    got, error, _ = run(types, [0], aggs, cut(rows, [4]))
    assert error == OUT_OF_RANGE and got == []            # the page that closes run 2 also closes run 1: the call fails as a whole
    check_against_model(types, [0], aggs, rows, got, error)


# ---- DOUBLE / REAL edge values ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fn", ["count_star", "count", "sum", "avg", "min", "max"])
@pytest.mark.parametrize("t", [abi.DOUBLE, abi.REAL], ids=A.label)
def test_floating_edge_cases(gpu, t, fn):
    """every DOUBLE / REAL row of agg_model.CASES as one run, the runs one behind the other and cut into pages of five rows"""
    cases = [c for c in A.CASES if c.type == t and c.fn == A.FNS[fn] and c.values]
    types = [abi.BIGINT, t, abi.BOOLEAN]
    rows = []
    for i, c in enumerate(cases):
        rows += [(i, v, True if c.mask is None else c.mask[j]) for j, v in enumerate(c.values)]
    aggs = [(A.FNS[fn], -1 if fn == "count_star" else 1, None if fn == "count_star" else t, 2)]
    got, error, _ = run(types, [0], aggs, cut(rows, [5]), abi.MEM_DEVICE)
    assert error is None and len(got) == len(cases)
    for c, row in zip(cases, got):
        o = A.case_result(c).outcome
        assert o[0] in ("value", "null"), c.name          # (no floating row of the table is an error or an `either` row)
        if o[0] == "null":
            assert row[1] is None, c.name
        else:
            exact = A.order_free(c.fn, t, A.counted(c.fn, c.values, c.mask))
            assert row[1] is not None and close_enough(A.result_type(c.fn, t), row[1], o[1], exact), (c.name, row, o)


# ---- shapes -----------------------------------------------------------------------------------------------------------------------------------
def test_no_aggregates(gpu):
    types = [abi.VARCHAR, abi.BIGINT]
    rows = [(b"a", 1), (b"a", 2), (b"b", 3), (None, 4), (None, 5), (b"", 6)]
    for sizes in ([6], [1], [4]):
        for mem in (abi.MEM_HOST, abi.MEM_DEVICE):
            got, error, _ = run(types, [0], [], cut(rows, sizes), mem)
            assert error is None and got == [(b"a",), (b"b",), (None,), (b"",)]


def test_dictionary_and_rle_input_blocks(gpu):
    key = Block.dictionary_block(Block.flat(abi.BIGINT, [5, 4, 0], [0, 0, 1]), [0, 0, 1, 2, 2, 0])
    rle = Block.rle(Block.bigint([10]), 6)
    for device in (False, True):
        op = StreamingAggregationOperator([abi.BIGINT, abi.BIGINT], [0], [(abi.AGG_SUM, 1, abi.BIGINT)])
        outs, error = drive(op, [Page([key, rle], 6)], device)
        op.close()
        assert error is None and [r for p in outs for r in p.to_rows()] == [(5, 20), (4, 10), (None, 20), (5, 10)]


def test_retained_input_pages(gpu):
    from tests.test_gpu_small_pages import retained_pages
    n = 5000
    keys = np.arange(n, dtype=np.int64) // 37
    hostp = Page([Block.bigint(keys), Block.double(np.ones(n))], n)
    bounds = [0, 700, 701, 2000, n]
    released = []
    pages = retained_pages(hostp, bounds, released)
    op = StreamingAggregationOperator([abi.BIGINT, abi.DOUBLE], [0], [(abi.AGG_SUM, 1, abi.DOUBLE), COUNT_STAR], output_mem=abi.MEM_DEVICE)
    outs = []
    for i, p in enumerate(pages):
        op.addInput(p)
        assert released == list(range(i + 1))          # the operator keeps nothing of a page: its carry is a copy
        out = op.getOutput()
        if out is not None:
            outs.append(host(out))
    op.finish()
    outs.append(host(op.getOutput()))
    op.close()
    rows = [r for p in outs for r in p.to_rows()]
    counts = np.bincount(keys)
    assert rows == [(k, float(c), int(c)) for k, c in enumerate(counts)]
    assert released == list(range(len(pages)))


# ---- fuzz -------------------------------------------------------------------------------------------------------------------------------------
FUZZ_KEYS = [abi.BIGINT, abi.INTEGER, abi.DOUBLE, abi.REAL, abi.BOOLEAN, abi.VARCHAR, abi.DATE]


def fuzz_value(rng, t, small):
    if rng.random() < 0.15:
        return None
    if t == abi.DOUBLE:
        return float(rng.choice([0.0, -0.0, NAN, 1.5, -2.25, 1e300, 0.1])) if small else float(rng.normal()) * 10 ** int(rng.integers(-3, 6))
    if t == abi.REAL:
        return np.float32(rng.choice([0.0, -0.0, NAN, 1.5, -2.25, 3e38, 0.1])) if small else np.float32(rng.normal())
    if t == abi.BOOLEAN:
        return bool(rng.integers(0, 2))
    if t == abi.VARCHAR:
        return bytes(rng.choice([b"", b"a", b"ab", b"b", LONG]))
    if t in (abi.INTEGER, abi.DATE):
        return int(rng.integers(-3, 3)) if small else int(rng.integers(-2 ** 27, 2 ** 27))
    # (magnitudes at which a run of thirty sometimes, not always, leaves its type)
    return int(rng.integers(-3, 3)) if small else int(rng.integers(-2 ** 60, 2 ** 60))


@pytest.mark.parametrize("seed", range(FUZZ_SEEDS))
def test_fuzz(gpu, seed):
    rng = np.random.default_rng(1000 + seed)
    key_types = [FUZZ_KEYS[int(i)] for i in rng.integers(0, len(FUZZ_KEYS), int(rng.integers(1, 4)))]
    types = key_types + [abi.BIGINT, abi.INTEGER, abi.DOUBLE, abi.REAL, abi.BOOLEAN, abi.DATE]
    nk = len(key_types)
    B, I, D, R, M, DT = nk, nk + 1, nk + 2, nk + 3, nk + 4, nk + 5
    pool = [COUNT_STAR, (abi.AGG_COUNT_STAR, -1, None, M), (abi.AGG_COUNT, D, abi.DOUBLE), (abi.AGG_SUM, B, abi.BIGINT), (abi.AGG_SUM, B, abi.BIGINT, M),
            (abi.AGG_AVG, B, abi.BIGINT), (abi.AGG_SUM, I, abi.INTEGER), (abi.AGG_AVG, I, abi.INTEGER, M), (abi.AGG_SUM, D, abi.DOUBLE), (abi.AGG_AVG, D, abi.DOUBLE, M),
            (abi.AGG_SUM, R, abi.REAL), (abi.AGG_AVG, R, abi.REAL), (abi.AGG_MIN, D, abi.DOUBLE), (abi.AGG_MAX, D, abi.DOUBLE, M), (abi.AGG_MIN, R, abi.REAL),
            (abi.AGG_MAX, R, abi.REAL), (abi.AGG_MIN, B, abi.BIGINT), (abi.AGG_MAX, I, abi.INTEGER), (abi.AGG_MIN, DT, abi.DATE), (abi.AGG_MAX, M, abi.BOOLEAN),
            (abi.AGG_MIN, M, abi.BOOLEAN, M)]
    aggs = [pool[int(i)] for i in rng.choice(len(pool), int(rng.integers(0, 9)), replace=False)]
    rows = []
    while len(rows) < 250:
        key = tuple(fuzz_value(rng, t, True) for t in key_types)
        for _ in range(int(rng.choice([1, 1, 2, 5, 30]))):
            # the zeros and the NaNs of one run may differ in their bits: the run goes on
            k = tuple((-v if isinstance(v, float) and v == 0 and rng.random() < 0.5 else v) for v in key)
            rows.append(k + tuple(fuzz_value(rng, t, False) for t in types[nk:]))
    sizes = [int(s) for s in rng.choice([1, 2, 3, 17, 64, 300], 4)]
    got, error, _ = run(types, list(range(nk)), aggs, cut(rows, sizes), abi.MEM_DEVICE if seed % 2 else abi.MEM_HOST, device_input=seed % 3 == 0)
    check_against_model(types, list(range(nk)), aggs, rows, got, error)


# ---- the hash aggregation over the same pages -------------------------------------------------------------------------------------------------
def test_hash_aggregation_gives_the_same_rows(gpu):
    """pre-grouped input with distinct run keys: the two operators agree on the multiset of rows (exact columns only)"""
    from presto_amd.operators import to_pages
    rng = np.random.default_rng(5)
    n = 6000
    keys = np.repeat(np.arange(400, dtype=np.int64) * 3 - 600, rng.integers(1, 30, 400))[:n]
    n = len(keys)
    values = rng.integers(-10 ** 9, 10 ** 9, n).astype(np.int64)
    nulls = (rng.random(n) < 0.1).astype(np.uint8)
    mask = (rng.random(n) < 0.8).astype(np.uint8)
    types = [abi.BIGINT, abi.BIGINT, abi.BOOLEAN]
    aggs = [COUNT_STAR, (abi.AGG_COUNT, 1, abi.BIGINT, 2), (abi.AGG_SUM, 1, abi.BIGINT, 2), (abi.AGG_MIN, 1, abi.BIGINT), (abi.AGG_MAX, 1, abi.BIGINT, 2)]
    bounds = [0, 1000, 1001, 4000, n]
    pages = [Page([Block.bigint(keys[lo:hi]), Block.flat(abi.BIGINT, values[lo:hi], nulls[lo:hi]), Block.boolean(mask[lo:hi])], hi - lo)
             for lo, hi in zip(bounds[:-1], bounds[1:])]
    op = StreamingAggregationOperator(types, [0], aggs)
    outs, error = drive(op, pages)
    op.close()
    streamed = [r for p in outs for r in p.to_rows()]
    hashed = [r for p in to_pages(HashAggregationOperator(types, [0], aggs), pages) for r in p.to_rows()]
    assert error is None and [r[0] for r in streamed] == sorted(set(keys.tolist()))       # in input order
    assert sorted(streamed, key=repr) == sorted(hashed, key=repr)
