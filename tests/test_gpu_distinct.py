"""GPU checks of MarkDistinctOperator and DistinctLimitOperator against a restatement of the reference's rule in this file
(MarkDistinctHash.markDistinctRows, MarkDistinctHash.java:52-69: a row is marked when its group id is one GroupByHash had not given
out before; GroupByHash compares by IS NOT DISTINCT FROM): the reference's own known-answer cases (TestMarkDistinctOperator,
TestDistinctLimitOperator), the NULL / NaN / -0.0 edges, determinism inside a page, growth, encodings, the DistinctLimit state machine,
the mark fed into a masked aggregation, seeded fuzz.  Every comparison is exact and in row order.  The oracle has no DISTINCT: the
expected marks come from `expected_marks` below."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from presto_amd import abi
from presto_amd._lib import check, lib
from presto_amd.operators import (DistinctLimitOperator, Driver, HashAggregationOperator, MarkDistinctOperator, download, download_page,
                                  to_pages, upload_page)
from presto_amd.page import Block, DeviceBuffer, Page

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the contract, restated (MarkDistinctHash.java:52-69) ---------------------------------------------------------------------
def canon(t, v):
    """GroupByHash's equality: IS NOT DISTINCT FROM (DoubleType.java:181-192 -- NaN matches NaN, -0.0 matches +0.0; BOOLEAN: any
    non-zero byte is true; NULL is one value)."""
    if v is None:
        return None
    if t in (abi.DOUBLE, abi.REAL):
        v = float(np.float32(v)) if t == abi.REAL else float(v)
        return "NaN" if math.isnan(v) else v + 0.0
    if t == abi.BOOLEAN:
        return v != 0
    if t == abi.VARCHAR:
        return v.encode("utf-8") if isinstance(v, str) else bytes(v)
    return int(v)


def key_of(types, row):
    return tuple(canon(t, v) for t, v in zip(types, row))


def expected_marks(types, rows, seen=None):
    """rows: key tuples in arrival order -> the mark of each; `seen` carries the keys over pages."""
    seen = set() if seen is None else seen
    out = []
    for r in rows:
        k = key_of(types, r)
        out.append(k not in seen)
        seen.add(k)
    return out


def block(t, values):
    """Host block of `values` (None = NULL)."""
    if t == abi.VARCHAR:
        return Block.varchar(values)
    nulls = [v is None for v in values]
    zero = 0.0 if t in (abi.DOUBLE, abi.REAL) else 0
    return Block.flat(t, [zero if v is None else v for v in values], nulls if any(nulls) else None)


def hash_block(n):
    """A $hashvalue channel: the operators never read it, so any BIGINT values must give the same result."""
    return Block.bigint([(i * 7919) & 0xFFFF for i in range(n)])


def split(rows, sizes):
    out, at = [], 0
    for s in sizes:
        if at >= len(rows):
            break
        out.append(rows[at:at + s])
        at += s
    if at < len(rows):
        out.append(rows[at:])
    return out


def raw_marks(op):
    """The mark column of the operator's next output page, from the C page itself (a device page may carry the input's dictionary /
    RLE blocks, which the Python page view does not decode): one byte per row, no nulls."""
    out = abi.pa_page()
    assert check(lib().pa_op_get_output(op._h, C.byref(out))) == 1
    n = out.position_count
    col = out.columns[out.channel_count - 1]
    assert col.type == abi.BOOLEAN and col.encoding == abi.FLAT and not col.nulls
    if out.mem == abi.MEM_DEVICE:
        return download(DeviceBuffer(col.values, n), np.uint8, n)
    return np.frombuffer(C.string_at(col.values, n), np.uint8) if n else np.zeros(0, np.uint8)


def feed(op, page):
    assert op.needsInput()
    op.addInput(page)
    assert not op.needsInput()          # a page is pending
    marks = raw_marks(op)
    assert op.needsInput() and not op.isFinished()
    return marks


def mark_rows(types, rows, sizes=None, hashed=False, output_mem=abi.MEM_HOST, device_input=False, expected_distinct=0, payload=True):
    """rows (key tuples) through a MarkDistinctOperator over (keys..., [BIGINT payload], [$hashvalue]) pages cut by `sizes`:
    checks marks and count against the restatement; returns the operator."""
    nk = len(types)
    page_types = list(types) + ([abi.BIGINT] if payload else []) + ([abi.BIGINT] if hashed else [])
    op = MarkDistinctOperator(page_types, list(range(nk)), hash_channel=len(page_types) - 1 if hashed else -1, output_mem=output_mem,
                              expected_distinct=expected_distinct)
    got = []
    for chunk in split(rows, sizes or [len(rows)]):
        n = len(chunk)
        blocks = [block(t, [r[c] for r in chunk]) for c, t in enumerate(types)]
        blocks += ([Block.bigint(list(range(n)))] if payload else []) + ([hash_block(n)] if hashed else [])
        page = Page(blocks, n)
        got += feed(op, upload_page(page) if device_input else page).tolist()
    want = expected_marks(types, rows)
    assert [bool(m) for m in got] == want
    assert all(m in (0, 1) for m in got)
    count, capacity = op.distinctStats()
    assert count == sum(want)
    assert capacity >= 2 * count and capacity & (capacity - 1) == 0
    op.finish()
    assert op.isFinished()
    return op


# ---- TestMarkDistinctOperator (core/trino-main/src/test/java/io/trino/operator/TestMarkDistinctOperator.java) -------------------
@pytest.mark.parametrize("hashed", [False, True])
def test_mark_distinct_kat(gpu, hashed):
    """testMarkDistinct: two sequence pages 0..99 -> the first all true, the second all false."""
    types = [abi.BIGINT] + ([abi.BIGINT] if hashed else [])
    op = MarkDistinctOperator(types, [0], hash_channel=1 if hashed else -1)
    pages = [Page([Block.bigint(list(range(100)))] + ([hash_block(100)] if hashed else []), 100) for _ in range(2)]
    out = to_pages(op, pages)
    rows = [r for p in out for r in p.to_rows()]
    assert [(r[0], r[-1]) for r in rows] == [(i, True) for i in range(100)] + [(i, False) for i in range(100)]
    assert [p.position_count for p in out] == [100, 100]
    assert all(len(r) == len(types) + 1 for r in rows)
    assert op.distinctStats()[0] == 100


# ---- TestDistinctLimitOperator (…/operator/TestDistinctLimitOperator.java) ----------------------------------------------------
def limit_pages(specs, hashed):
    """rowPagesBuilder(...).addSequencePage(length, start) per spec"""
    return [Page([Block.bigint(list(range(start, start + n)))] + ([hash_block(n)] if hashed else []), n) for n, start in specs]


def drive_limit(op, pages):
    """OperatorAssertion.toPages for an operator that may stop needing input: feed while needsInput, then finish."""
    out = []
    for page in pages:
        if not op.needsInput():
            break
        op.addInput(page)
        p = op.getOutput()
        if p is not None:
            out.append(p)
    op.finish()
    p = op.getOutput()
    assert p is None
    assert op.isFinished()
    return out


@pytest.mark.parametrize("hashed", [False, True])
@pytest.mark.parametrize("specs,limit,expected", [
    ([(3, 1), (5, 2)], 5, [1, 2, 3, 4, 5]),      # testDistinctLimit
    ([(3, 1), (3, 2)], 3, [1, 2, 3]),            # testDistinctLimitWithPageAlignment
    ([(3, 1), (3, 2)], 5, [1, 2, 3, 4]),         # testDistinctLimitValuesLessThanLimit
])
def test_distinct_limit_kats(gpu, hashed, specs, limit, expected):
    types = [abi.BIGINT] + ([abi.BIGINT] if hashed else [])
    op = DistinctLimitOperator(types, [0], limit, hash_channel=1 if hashed else -1)
    rows = [r for p in drive_limit(op, limit_pages(specs, hashed)) for r in p.to_rows()]
    assert [r[0] for r in rows] == expected
    assert all(len(r) == len(types) for r in rows)


# ---- testMemoryReservationYield's shape: pages of all-new keys -----------------------------------------------------------------
@pytest.mark.parametrize("t", [abi.BIGINT, abi.VARCHAR])
def test_pages_of_new_keys_only(gpu, t):
    """Every row carries a key not seen before: every mark is true and the count is the rows fed (the table grows on the way)."""
    pages, rows_per_page = (16, 1 << 16) if t == abi.BIGINT else (6, 20000)
    op = MarkDistinctOperator([t], [0])
    before = op.distinctStats()[1]
    fed = 0
    for p in range(pages):
        ids = np.arange(fed, fed + rows_per_page, dtype=np.int64)
        key = Block.bigint(ids * 1000003 - 7) if t == abi.BIGINT else Block.varchar(["key-%d" % i for i in ids])
        marks = feed(op, Page([key], rows_per_page))
        assert marks.dtype == np.uint8 and len(marks) == rows_per_page and bool((marks == 1).all())
        fed += rows_per_page
    count, capacity = op.distinctStats()
    assert count == fed
    assert capacity > before and capacity >= 2 * fed and capacity & (capacity - 1) == 0
    assert op.memoryBytes() >= capacity * 8 + fed * 8


# ---- edges ---------------------------------------------------------------------------------------------------------------------
def test_null_keys(gpu):
    mark_rows([abi.BIGINT], [(None,), (1,), (None,), (0,), (1,), (None,)])
    mark_rows([abi.BIGINT], [(None,), (None,), (5,)], sizes=[1, 1, 1])
    mark_rows([abi.VARCHAR], [(None,), ("",), (None,), ("",), ("a",)])        # the empty string is not NULL


@pytest.mark.parametrize("t", [abi.DOUBLE, abi.REAL])
def test_nan_and_signed_zero(gpu, t):
    nan, other_nan = float("nan"), np.frombuffer(np.uint64(0x7FF0000000000123).tobytes(), np.float64)[0]
    if t == abi.REAL:
        other_nan = np.frombuffer(np.uint32(0x7FC01234).tobytes(), np.float32)[0]
    rows = [(nan,), (-0.0,), (other_nan,), (0.0,), (1.5,), (-1.5,), (None,), (nan,), (-0.0,), (1.5,), (None,)]
    mark_rows([t], rows)
    mark_rows([t], rows, sizes=[3, 1, 4])
    mark_rows([t], list(reversed(rows)), device_input=True, output_mem=abi.MEM_DEVICE)


def test_boolean_bytes_other_than_0_and_1(gpu):
    mark_rows([abi.BOOLEAN], [(2,), (1,), (0,), (255,), (None,), (0,), (7,)])
    mark_rows([abi.BOOLEAN, abi.BOOLEAN], [(2, 0), (1, 0), (1, 3), (9, 1), (0, 0), (None, 0), (0, None)])


def test_real_and_short_decimal_keys(gpu):
    mark_rows([abi.REAL], [(1.25,), (1.25,), (-1.25,), (3.0e38,), (1.0e-40,), (3.0e38,)])
    t = abi.decimal(12, 2)
    op = MarkDistinctOperator([t, abi.BIGINT], [0])
    out = to_pages(op, [Page([Block.decimal([12345, -5, 0, 12345, 5, -5]), Block.bigint(list(range(6)))], 6)])
    assert [r[-1] for p in out for r in p.to_rows()] == [True, True, True, False, True, False]
    op = MarkDistinctOperator([abi.DATE, abi.INTEGER], [0, 1])
    out = to_pages(op, [Page([Block.date([1, 1, 2, 1]), Block.integer([-1, -1, -1, 1])], 4)])
    assert [r[-1] for p in out for r in p.to_rows()] == [True, False, True, True]


def test_varchar_lengths(gpu):
    rows = [(b"",), (b"a",), (b"abcdefghijklmnop",), (b"abcdefghijklmnoq",), (b"abcdefghX",), (b"abcdefghY",), (b"abcdefgh",), (b"x" * 100,),
            (b"x" * 99,), (None,), (b"abcdefghY",), (b"x" * 100,), (b"",), (None,), (b"abcdefghijklmnop",)]
    mark_rows([abi.VARCHAR], rows)
    mark_rows([abi.VARCHAR], rows, sizes=[4, 4, 4], device_input=True)


def test_multi_channel_keys_with_nulls_in_different_channels(gpu):
    types = [abi.BIGINT, abi.DOUBLE, abi.VARCHAR]
    rows = [(None, 1.0, "a"), (None, 2.0, "a"), (1, None, "a"), (1, 1.0, None), (None, None, None), (None, 1.0, "a"), (1, None, "a"),
            (0, 0.0, ""), (None, 0.0, ""), (0, None, ""), (0, -0.0, ""), (None, None, None), (1, 1.0, "a"), (1, 1.0, "b"), (1, 1.0, "a")]
    mark_rows(types, rows)
    mark_rows(types, rows, sizes=[5, 5], hashed=True)
    # (NULL, 1) and (NULL, 2) are different keys; (NULL, 1) and (0, 1) too
    mark_rows([abi.BIGINT, abi.BIGINT], [(None, 1), (None, 2), (0, 1), (None, 1), (0, None), (0, 0), (0, None)])
    # eight channels
    eight = [abi.BIGINT, abi.INTEGER, abi.DATE, abi.DOUBLE, abi.REAL, abi.BOOLEAN, abi.VARCHAR, abi.BIGINT]
    base = (1, 2, 3, 4.0, 5.0, 1, "s", 8)
    rows8 = [base, base] + [tuple(None if c == i else v for c, v in enumerate(base)) for i in range(8)] + [base, tuple([None] * 8), tuple([None] * 8)]
    mark_rows(eight, rows8)


# ---- determinism inside a page ---------------------------------------------------------------------------------------------------
def numpy_marks(keys):
    marks = np.zeros(len(keys), np.uint8)
    marks[np.unique(keys, return_index=True)[1]] = 1
    return marks


def run_numpy(keys, sizes, device_input=True, expected_distinct=0):
    op = MarkDistinctOperator([abi.BIGINT], [0], output_mem=abi.MEM_DEVICE if device_input else abi.MEM_HOST, expected_distinct=expected_distinct)
    got, at, i = [], 0, 0
    while at < len(keys):
        n = sizes[min(i, len(sizes) - 1)]
        page = Page([Block.bigint(keys[at:at + n])], len(keys[at:at + n]))
        got.append(feed(op, upload_page(page) if device_input else page))
        at += n
        i += 1
    return np.concatenate(got), op


def test_one_key_on_every_row_of_a_large_page(gpu):
    n = 1 << 20
    for _ in range(2):
        marks, op = run_numpy(np.full(n, 42, np.int64), [n])
        assert marks[0] == 1 and int(marks.sum()) == 1
        assert op.distinctStats()[0] == 1


def test_every_key_twice_marks_the_smaller_position(gpu):
    rng = np.random.default_rng(11)
    half = 1 << 19
    keys = np.concatenate([np.arange(half), np.arange(half)]).astype(np.int64) * 2654435761
    keys = keys[rng.permutation(len(keys))]
    want = numpy_marks(keys)
    assert int(want.sum()) == half
    first, _ = run_numpy(keys, [len(keys)])
    second, _ = run_numpy(keys, [len(keys)])
    assert np.array_equal(first, want)
    assert first.tobytes() == second.tobytes()


def test_page_splits_do_not_change_the_marks(gpu):
    rng = np.random.default_rng(12)
    n = 1 << 20
    keys = rng.integers(0, 200000, n).astype(np.int64)
    want = numpy_marks(keys)
    whole, op = run_numpy(keys, [n])
    assert np.array_equal(whole, want)
    assert op.distinctStats()[0] == int(want.sum())
    marks4096, _ = run_numpy(keys, [4096])
    assert np.array_equal(marks4096, want)
    # pages of 1 and 7 rows over a prefix (a page per row is host time), then the rest in one page
    for small in (1, 7):
        sizes = [small] * (3000 // small) + [n]
        got, op = run_numpy(keys, sizes, device_input=False)
        assert np.array_equal(got, want), small
        assert op.distinctStats()[0] == int(want.sum())


# ---- growth ----------------------------------------------------------------------------------------------------------------------
def test_growth_from_one_expected_key(gpu):
    rng = np.random.default_rng(13)
    keys = rng.integers(0, 1 << 40, 300000).astype(np.int64)
    keys[1000:2000] = keys[:1000]
    keys[250000:] = keys[100000:150000]
    op = MarkDistinctOperator([abi.BIGINT], [0], expected_distinct=1)
    capacities = [op.distinctStats()[1]]
    got, at = [], 0
    for n in (1, 10, 100, 889, 1000, 8000, 40000, 50000, 100000, 100000):
        got.append(feed(op, Page([Block.bigint(keys[at:at + n])], n)))
        at += n
        count, capacity = op.distinctStats()
        assert count == len(np.unique(keys[:at]))
        assert capacity & (capacity - 1) == 0 and capacity >= 2 * count
        capacities.append(capacity)
    assert at == len(keys)
    assert np.array_equal(np.concatenate(got), numpy_marks(keys))
    assert capacities == sorted(capacities) and len(set(capacities)) >= 5      # several rehashes
    assert capacities[0] <= 64


def test_growth_with_varchar_and_two_channels(gpu):
    rng = np.random.default_rng(14)
    rows = [("s%d" % v, int(v) % 3 if v % 5 else None) for v in rng.integers(0, 20000, 30000)]
    mark_rows([abi.VARCHAR, abi.BIGINT], rows, sizes=[10, 100, 1000, 5000, 10000], expected_distinct=1)


def test_memory_limit_applies_to_growth(gpu):
    L = lib()
    op = MarkDistinctOperator([abi.BIGINT], [0], expected_distinct=1)
    feed(op, Page([Block.bigint([1, 2, 3])], 3))
    n = 1 << 22
    page = upload_page(Page([Block.bigint(np.arange(n, dtype=np.int64))], n))
    cpage, _keep = page.to_c()
    L.pa_memory_set_limit(32 << 20)             # the table for 4 Mi more keys alone is 64 MiB
    try:
        assert L.pa_op_add_input(op._h, C.byref(cpage)) == abi.ERR_INSUFFICIENT_RESOURCES
    finally:
        L.pa_memory_set_limit(0)
    op.close()


# ---- encodings and memory spaces -------------------------------------------------------------------------------------------------
def test_dictionary_and_rle_key_channels(gpu):
    key = Block.dictionary_block(Block.flat(abi.BIGINT, [5, 4, 0], [0, 0, 1]), [0, 1, 2, 2, 0, 1])
    rle = Block.rle(Block.bigint([4]), 6)
    strings = Block.dictionary_block(Block.varchar(["x", "yy", None]), [1, 1, 2, 0, 2, 0])
    for output_mem in (abi.MEM_HOST, abi.MEM_DEVICE):
        for t, k in ((abi.BIGINT, key), (abi.BIGINT, rle), (abi.VARCHAR, strings)):
            op = MarkDistinctOperator([t, abi.BIGINT], [0], output_mem=output_mem)
            seen = set()
            for page in (Page([k, Block.bigint(list(range(6)))], 6), upload_page(Page([k, Block.bigint(list(range(6)))], 6))):
                want = expected_marks([t], [(v,) for v in k.to_pylist()], seen)
                assert [bool(m) for m in feed(op, page)] == want, (output_mem, k.encoding)
            op.close()


def test_pass_through_channels_are_the_input(gpu):
    names = Block.varchar(["a", None, "ccc", "a"])
    dic = Block.dictionary_block(Block.varchar(["x", "yy"]), [1, 0, 0, 1])
    types = [abi.VARCHAR, abi.BIGINT, abi.VARCHAR, abi.DOUBLE]
    host = Page([names, Block.bigint([1, 5, 3, 1]), dic, Block.double([0.5, -1.0, 2.0, 3.0])], 4)
    for output_mem in (abi.MEM_HOST, abi.MEM_DEVICE):       # host in -> host out / device out
        op = MarkDistinctOperator(types, [0, 1], output_mem=output_mem)
        op.addInput(host)
        out = op.getOutput()
        assert out.mem == output_mem
        if out.mem == abi.MEM_DEVICE:
            out = download_page(out)
        assert [r[:-1] for r in out.to_rows()] == host.to_rows()
        assert [r[-1] for r in out.to_rows()] == [True, True, True, False]

    # device -> device: the input blocks themselves, encodings included; only the mark is new, and it has no nulls
    dev = upload_page(host)
    op = MarkDistinctOperator(types, [0, 1], output_mem=abi.MEM_DEVICE)
    cpage, _keep = dev.to_c()
    check(lib().pa_op_add_input(op._h, C.byref(cpage)))
    out = abi.pa_page()
    assert check(lib().pa_op_get_output(op._h, C.byref(out))) == 1
    assert out.channel_count == 5 and out.position_count == 4 and out.mem == abi.MEM_DEVICE
    for c in range(4):
        assert out.columns[c].encoding == cpage.columns[c].encoding
        assert out.columns[c].values == cpage.columns[c].values
        assert out.columns[c].offsets == cpage.columns[c].offsets
        assert out.columns[c].nulls == cpage.columns[c].nulls
        assert out.columns[c].ids == cpage.columns[c].ids
    assert out.columns[2].dictionary[0].values == cpage.columns[2].dictionary[0].values
    assert out.columns[4].type == abi.BOOLEAN and out.columns[4].encoding == abi.FLAT and not out.columns[4].nulls
    assert download(DeviceBuffer(out.columns[4].values, 4), np.uint8, 4).tolist() == [1, 1, 1, 0]
    op.close()


def test_mark_distinct_retained_pages_are_released_exactly_once(gpu):
    """A PA_PAGE_RETAINED page is released once its output page has been let go -- not before (the zero-copy output page IS the input's
    blocks: the release callback scribbles over them) -- and exactly once, also when the operator is closed over a pending output."""
    from tests.test_gpu_row_number import host_page_of, raw_output
    from tests.test_gpu_small_pages import retained_pages
    n = 5000
    keys = np.arange(n, dtype=np.int64) % 97
    host = Page([Block.bigint(keys), Block.double(np.arange(n, dtype=np.float64))], n)
    bounds = [0, 700, 701, 2000, n]
    want = numpy_marks(keys)
    released = []
    pages = retained_pages(host, bounds, released)
    op = MarkDistinctOperator([abi.BIGINT, abi.DOUBLE], [0], output_mem=abi.MEM_DEVICE)
    for i, p in enumerate(pages):
        lo, hi = bounds[i], bounds[i + 1]
        assert op.needsInput()
        op.addInput(p)
        assert released == list(range(i))                                # page i is still held
        out = raw_output(op)
        assert out is not None and out.mem == abi.MEM_DEVICE and out.position_count == hi - lo and out.channel_count == 3
        got = host_page_of(op, out)                                      # reads the caller's blocks: they must still be intact
        assert np.array_equal(got.blocks[0].values[:hi - lo], keys[lo:hi])
        assert np.array_equal(got.blocks[1].values[:hi - lo], np.arange(lo, hi, dtype=np.float64))
        assert np.array_equal(got.blocks[2].values[:hi - lo], want[lo:hi])
        assert released == list(range(i))                                # ... while its output page is out
        op.needsInput()                                                  # the output page has been let go
        assert released == list(range(i + 1))
    op.finish()
    op.close()
    assert released == list(range(len(pages)))

    # closed while an output page is still pending: the page goes back once, at close
    released = []
    pages = retained_pages(host, bounds, released)
    op = MarkDistinctOperator([abi.BIGINT, abi.DOUBLE], [0], output_mem=abi.MEM_DEVICE)
    op.addInput(pages[0])
    assert not op.needsInput() and released == []
    op.close()
    assert released == [0]
    del op
    assert released == [0]


def test_empty_pages_and_protocol(gpu):
    op = MarkDistinctOperator([abi.BIGINT], [0])
    empty = Page([Block.bigint([])], 0)
    check(lib().pa_op_add_input(op._h, C.byref(empty.to_c()[0])))
    assert op.getOutput() is None and op.needsInput()
    page = Page([Block.bigint([1, 1])], 2)
    op.addInput(page)
    assert lib().pa_op_add_input(op._h, C.byref(page.to_c()[0])) == abi.ERR_ILLEGAL_STATE      # a page is pending
    op.finish()
    assert not op.isFinished()                                                                # finishing, but a page is pending
    assert raw_marks(op).tolist() == [1, 0]
    assert op.isFinished() and not op.needsInput()
    assert lib().pa_op_add_input(op._h, C.byref(page.to_c()[0])) == abi.ERR_ILLEGAL_STATE
    count, capacity = C.c_int64(), C.c_int64()
    agg = HashAggregationOperator([abi.BIGINT], [0], [(abi.AGG_COUNT_STAR, -1, None)])
    assert lib().pa_distinct_stats(agg._h, C.byref(count), C.byref(capacity)) == abi.ERR_INVALID_ARGUMENT
    assert op.kernelName() == "k_distinct_insert"
    ms, launches = op.kernelTime()
    assert launches == 1 and ms > 0


# ---- DistinctLimit ---------------------------------------------------------------------------------------------------------------
def check_limit(types, channels, limit, pages_rows, hashed=False, output_mem=abi.MEM_HOST, device_input=False):
    """pages_rows: per page the rows over `types`.  Follows DistinctLimitOperator's state machine call by call and compares the
    emitted rows (distinct channels in descriptor order, then the hash channel) exactly and in order."""
    page_types = list(types) + ([abi.BIGINT] if hashed else [])
    hc = len(page_types) - 1 if hashed else -1
    op = DistinctLimitOperator(page_types, channels, limit, hash_channel=hc, output_mem=output_mem)
    key_types = [types[c] for c in channels]
    remaining, seen = limit, set()
    assert op.isFinished() == (limit == 0) and op.needsInput() == (limit > 0)
    for rows in pages_rows:
        n = len(rows)
        blocks = [block(t, [r[c] for r in rows]) for c, t in enumerate(types)] + ([hash_block(n)] if hashed else [])
        page = Page(blocks, n)
        if remaining == 0:
            assert not op.needsInput() and op.isFinished()
            assert lib().pa_op_add_input(op._h, C.byref(page.to_c()[0])) == abi.ERR_ILLEGAL_STATE
            break
        assert op.needsInput() and not op.isFinished()
        op.addInput(upload_page(page) if device_input else page)
        hashes = hash_block(n).to_pylist()
        want = []
        for i, r in enumerate(rows):
            k = key_of(key_types, [r[c] for c in channels])
            if k not in seen and len(want) < remaining:
                seen.add(k)
                want.append(tuple(k) + ((hashes[i],) if hashed else ()))
        remaining -= len(want)
        if want:
            assert not op.needsInput() and not op.isFinished()        # a page is pending
        out = op.getOutput()
        if not want:
            assert out is None                                           # a page without a new key gives no page
        else:
            assert out.mem == output_mem
            if out.mem == abi.MEM_DEVICE:
                out = download_page(out)
            got = [tuple(key_of(key_types, r[:len(channels)])) + tuple(r[len(channels):]) for r in out.to_rows()]
            assert got == want
        assert op.getOutput() is None
        assert op.needsInput() == (remaining > 0) and op.isFinished() == (remaining == 0)
    count, _ = op.distinctStats()
    assert count >= limit - remaining
    op.finish()
    assert op.isFinished() and not op.needsInput() and op.getOutput() is None
    op.close()
    return limit - remaining


def test_distinct_limit_state_machine(gpu):
    t = [abi.BIGINT]
    # the limit is reached inside a page: only the first `remaining` new keys, in position order
    assert check_limit(t, [0], 4, [[(5,), (5,), (3,)], [(3,), (9,), (5,), (8,), (7,), (6,)], [(1,)]]) == 4
    # a page without a new key gives no page; limit equal to the distinct count
    assert check_limit(t, [0], 3, [[(1,), (2,)], [(2,), (1,), (1,)], [(3,)], [(4,)]]) == 3
    assert check_limit(t, [0], 3, [[(1,), (2,)], [(2,), (1,)], [(3,)]]) == 3
    # fewer keys than the limit
    assert check_limit(t, [0], 10, [[(1,), (None,)], [(None,), (1,)]]) == 2
    # limit 0: finished at creation
    assert check_limit(t, [0], 0, [[(1,)]]) == 0


@pytest.mark.parametrize("device", [False, True])
def test_distinct_limit_output_channels(gpu, device):
    """Output = the distinct channels in descriptor order, then the hash channel; other channels are dropped."""
    types = [abi.BIGINT, abi.VARCHAR, abi.DOUBLE, abi.BIGINT]
    rows = [(7, "a", 0.0, 1), (8, "bb", -0.0, 1), (9, "a", float("nan"), 2), (7, None, 1.0, 1), (7, "a", 0.0, 2), (7, None, 1.0, 2),
            (1, "a-long-string-past-eight-bytes", 2.0, 3), (1, "a-long-string-past-eight-bytez", 2.0, 3)]
    mem = abi.MEM_DEVICE if device else abi.MEM_HOST
    assert check_limit(types, [1, 3], 100, [rows[:3], rows[3:]], hashed=True, output_mem=mem, device_input=device) == 7
    assert check_limit(types, [2, 1], 4, [rows], hashed=True, output_mem=mem, device_input=device) == 4
    assert check_limit(types, [3], 2, [rows], hashed=False, output_mem=mem, device_input=device) == 2


def test_distinct_limit_inside_a_large_page(gpu):
    rng = np.random.default_rng(15)
    n = 1 << 18
    keys = rng.integers(0, 50000, n).astype(np.int64)
    first = np.sort(np.unique(keys, return_index=True)[1])
    for limit in (1, 1000, len(first), len(first) + 5):
        op = DistinctLimitOperator([abi.BIGINT], [0], limit)
        out = drive_limit(op, [Page([Block.bigint(keys)], n), Page([Block.bigint(keys[::-1].copy())], n)])
        got = np.concatenate([p.blocks[0].values for p in out])
        assert np.array_equal(got, keys[first[:limit]]), limit


# ---- the mark feeds a masked aggregation: SELECT g, count(DISTINCT x), sum(DISTINCT x), count(*) ... GROUP BY g -------------------
@pytest.mark.parametrize("device", [False, True])
def test_mark_distinct_into_masked_aggregation(gpu, device):
    rng = np.random.default_rng(16)
    n, pages = 50000, 4
    g = rng.integers(0, 37, n * pages).astype(np.int64)
    x = rng.integers(-500, 500, n * pages).astype(np.int64)
    mem = abi.MEM_DEVICE if device else abi.MEM_HOST
    mark = MarkDistinctOperator([abi.BIGINT, abi.BIGINT], [0, 1], output_mem=mem)
    agg = HashAggregationOperator([abi.BIGINT, abi.BIGINT, abi.BOOLEAN], [0],
                                  [(abi.AGG_COUNT, 1, abi.BIGINT, 2), (abi.AGG_SUM, 1, abi.BIGINT, 2), (abi.AGG_COUNT_STAR, -1, None)])
    source = []
    for p in range(pages):
        page = Page([Block.bigint(g[p * n:(p + 1) * n]), Block.bigint(x[p * n:(p + 1) * n])], n)
        source.append(upload_page(page) if device else page)
    out = Driver(source, [mark, agg]).run()
    got = sorted(tuple(r) for p in out for r in p.to_rows())
    want = []
    for key in np.unique(g):
        xs = x[g == key]
        distinct = set(xs.tolist())
        want.append((int(key), len(distinct), sum(distinct), len(xs)))
    assert got == want
    assert mark.distinctStats()[0] == sum(w[1] for w in want)


# ---- seeded fuzz -----------------------------------------------------------------------------------------------------------------
FUZZ_SEEDS = int(os.environ.get("PA_FUZZ_SEEDS", "16"))
FUZZ_TYPES = [abi.BIGINT, abi.INTEGER, abi.DATE, abi.DOUBLE, abi.REAL, abi.BOOLEAN, abi.VARCHAR]


def _fuzz_column(rng, t, n, domain, null_rate):
    out = []
    for v in rng.integers(-domain, domain, n):
        v = int(v)
        if rng.random() < null_rate:
            out.append(None)
        elif t in (abi.DOUBLE, abi.REAL):
            r = rng.random()
            out.append(float("nan") if r < 0.05 else (-0.0 if r < 0.1 else float(v) / 4))
        elif t == abi.BOOLEAN:
            out.append(v & 0xFF)
        elif t == abi.VARCHAR:
            out.append(("k%d" % v) * (1 + abs(v) % 5))
        else:
            out.append(v)
    return out


def _fuzz_case(seed):
    rng = np.random.default_rng(2000 + seed)
    nk = int(rng.integers(1, 5))
    types = [FUZZ_TYPES[int(rng.integers(0, len(FUZZ_TYPES)))] for _ in range(nk)]
    n = int(rng.integers(1, 12000))
    # cardinality from 1 to all-distinct: the per-channel domain
    domain = int(rng.choice([1, 2, 30, 1000, 1 << 30]))
    cols = [_fuzz_column(rng, t, n, domain if t != abi.VARCHAR else min(domain, 1 << 20), float(rng.choice([0.0, 0.02, 0.4]))) for t in types]
    rows = list(zip(*cols))
    sizes = [int(s) for s in rng.integers(1, max(2, n // 2), int(rng.integers(1, 6)))]
    return rng, types, rows, sizes


@pytest.mark.parametrize("seed", range(FUZZ_SEEDS))
def test_fuzz_mark_distinct(gpu, seed):
    rng, types, rows, sizes = _fuzz_case(seed)
    mark_rows(types, rows, sizes=sizes, hashed=bool(rng.integers(0, 2)), output_mem=int(rng.integers(0, 2)), device_input=bool(rng.integers(0, 2)),
              expected_distinct=int(rng.choice([0, 1, 100])))


@pytest.mark.parametrize("seed", range(FUZZ_SEEDS))
def test_fuzz_distinct_limit(gpu, seed):
    rng, types, rows, sizes = _fuzz_case(seed)
    distinct = len({key_of(types, r) for r in rows})
    limit = int(rng.choice([1, max(1, distinct // 2), distinct, distinct + 3]))
    order = [int(c) for c in rng.permutation(len(types))]
    device = bool(rng.integers(0, 2))
    emitted = check_limit(types, order, limit, split(rows, sizes), hashed=bool(rng.integers(0, 2)), output_mem=abi.MEM_DEVICE if device else abi.MEM_HOST,
                          device_input=device)
    assert emitted == min(limit, distinct)


# ---- a scrubbed pool, in a child process -------------------------------------------------------------------------------------------
def test_on_a_scrubbed_pool(gpu):
    """Growth, VARCHAR keys and the limit once more with every recycled HBM block overwritten before it is handed out
    (PRESTO_AMD_POOL_SCRUB, pool.cpp): a table or store that relied on what a block's previous owner left behind fails here."""
    env = dict(os.environ, PRESTO_AMD_POOL_SCRUB="0xA5", PA_FUZZ_SEEDS="4")
    picks = ["test_growth_from_one_expected_key", "test_growth_with_varchar_and_two_channels", "test_distinct_limit_state_machine",
             "test_fuzz_mark_distinct", "test_fuzz_distinct_limit", "test_multi_channel_keys_with_nulls_in_different_channels"]
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider", "tests/test_gpu_distinct.py", "-k",
                        " or ".join(picks)], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    tail = r.stdout.decode()[-3000:]
    assert r.returncode == 0, tail
    assert " passed" in tail and "failed" not in tail


# ---- the C++ mirror (include/presto_amd.hpp) ---------------------------------------------------------------------------------------
def test_cpp_mirror(gpu):
    """tests/cpp/test_distinct.cpp: both operators through the C++ host mirror's runDriver."""
    exe = os.path.join(ROOT, "tests", "cpp", "test_distinct")
    src = exe + ".cpp"
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-L" + os.path.join(ROOT, "presto_amd"),
                               "-lpresto_amd", "-Wl,-rpath,$ORIGIN/../../presto_amd", "-Wl,--allow-shlib-undefined", "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode == 0, r.stdout.decode()[-2000:]
    assert "distinct ok" in r.stdout.decode()
