"""GPU checks of SetBuilderOperator + HashSemiJoinOperator against a restatement of the reference's mark rules in this file
(HashSemiJoinOperator.java:190-218; ChannelSet.contains is IS NOT DISTINCT FROM): the reference's own known-answer cases
(TestHashSemiJoinOperator), the NULL / NaN / -0.0 edges, every layout of the set, page handling, sharing and lifetimes, and seeded
fuzz.  The oracle has no semi-join: the expected marks come from `expected_marks` below."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from presto_amd import abi
from presto_amd._lib import check, lib
from presto_amd.operators import (HashSemiJoinOperator, HashSemiJoinOperatorFactory, SetBuilderOperator, SetBuilderOperatorFactory, SetSupplier,
                                  download, download_page, to_pages, upload_page)
from presto_amd.page import Block, DeviceBuffer, Page

pytestmark = pytest.mark.gpu


# ---- the contract, restated (HashSemiJoinOperator.java:190-218) ----------------------------------------------------------------
def canon(t, v):
    """The set's equality: IS NOT DISTINCT FROM (DoubleType.java:181-192 -- NaN matches NaN, -0.0 matches +0.0; BOOLEAN: any
    non-zero byte is true)."""
    if t in (abi.DOUBLE, abi.REAL):
        v = float(np.float32(v)) if t == abi.REAL else float(v)
        return "NaN" if math.isnan(v) else v + 0.0
    if t == abi.BOOLEAN:
        return v != 0
    return v


def expected_marks(t, build_values, probe_values):
    values = {canon(t, v) for v in build_values if v is not None}
    has_null = any(v is None for v in build_values)
    empty = len(build_values) == 0
    out = []
    for v in probe_values:
        if v is None:
            out.append(False if empty else None)
        elif canon(t, v) in values:
            out.append(True)
        else:
            out.append(None if has_null else False)
    return out


def expected_size(t, build_values):
    """ChannelSet.size(): distinct values, NULL counted as one."""
    return len({canon(t, v) for v in build_values if v is not None}) + (1 if any(v is None for v in build_values) else 0)


def block(t, values):
    """Host block of `values` (None = NULL)."""
    if t == abi.VARCHAR:
        return Block.varchar(values)
    nulls = [v is None for v in values]
    zero = 0.0 if t in (abi.DOUBLE, abi.REAL) else 0
    return Block.flat(t, [zero if v is None else v for v in values], nulls if any(nulls) else None)


def hash_block(values):
    """A $hashvalue channel: the operators do not read it, so any BIGINT values must give the same marks."""
    return Block.bigint([(hash(v) * 31) & 0x7FFFFFFFFFFFFFFF for v in values])


def split(values, sizes):
    out, at = [], 0
    for s in sizes:
        out.append(values[at:at + s])
        at += s
    if at < len(values):
        out.append(values[at:])
    return out


def build_set(t, build_values, hashed=False, page_rows=None):
    """A set over channel 1 of (BIGINT payload, key[, $hashvalue]) pages."""
    types = [abi.BIGINT, t] + ([abi.BIGINT] if hashed else [])
    pages = []
    for chunk in split(build_values, [page_rows] * (len(build_values) // page_rows + 1) if page_rows else [len(build_values)]):
        blocks = [Block.bigint(list(range(len(chunk)))), block(t, chunk)] + ([hash_block(chunk)] if hashed else [])
        pages.append(Page(blocks, len(chunk)))
    s = SetSupplier()
    b = SetBuilderOperator(s, types, 1, hash_channel=2 if hashed else -1)
    to_pages(b, [p for p in pages if p.position_count > 0])
    return s, b


def probe(s, t, probe_pages_values, hashed=False, output_mem=abi.MEM_HOST, device_input=False):
    """(key, BIGINT payload[, $hashvalue]) probe pages -> output rows and the operator's kernel name."""
    types = [t, abi.BIGINT] + ([abi.BIGINT] if hashed else [])
    j = HashSemiJoinOperator(s, types, 0, probe_hash_channel=2 if hashed else -1, output_mem=output_mem)
    rows, at = [], 0
    for vals in probe_pages_values:
        blocks = [block(t, vals), Block.bigint(list(range(at, at + len(vals))))] + ([hash_block(vals)] if hashed else [])
        at += len(vals)
        page = Page(blocks, len(vals))
        if device_input:
            page = upload_page(page)
        for out in to_pages_keep(j, page):
            host = out if out.mem == abi.MEM_HOST else download_page(out)
            rows += host.to_rows()
    j.finish()
    assert j.isFinished()
    return rows, j.kernelName()


def to_pages_keep(op, page):
    assert op.needsInput()
    op.addInput(page)
    out = []
    while True:
        p = op.getOutput()
        if p is None:
            return out
        out.append(p)


def check_marks(t, build_values, probe_pages_values, hashed=False, output_mem=abi.MEM_HOST, device_input=False, page_rows=None):
    s, _ = build_set(t, build_values, hashed=hashed, page_rows=page_rows)
    rows, name = probe(s, t, probe_pages_values, hashed=hashed, output_mem=output_mem, device_input=device_input)
    flat = [v for vals in probe_pages_values for v in vals]
    assert len(rows) == len(flat)
    marks = [r[-1] for r in rows]
    assert marks == expected_marks(t, build_values, flat)
    # the input channels come out unchanged and in order
    assert [r[1] for r in rows] == list(range(len(flat)))
    assert s.stats() == (expected_size(t, build_values), any(v is None for v in build_values))
    return name


# ---- TestHashSemiJoinOperator (core/trino-main/src/test/java/io/trino/operator/TestHashSemiJoinOperator.java) ---------------
@pytest.mark.parametrize("hashed", [False, True])
def test_semi_join_kat(gpu, hashed):
    """testSemiJoin: build 10, 30, 30, 35, 36, 37, 50; probe 30..39 -> true for 30, 35, 36, 37."""
    s, _ = build_set(abi.BIGINT, [10, 30, 30, 35, 36, 37, 50], hashed=hashed)
    rows, _ = probe(s, abi.BIGINT, [list(range(30, 40))], hashed=hashed)
    assert [(r[0], r[-1]) for r in rows] == [(30, True), (31, False), (32, False), (33, False), (34, False), (35, True), (36, True),
                                             (37, True), (38, False), (39, False)]


@pytest.mark.parametrize("hashed", [False, True])
def test_semi_join_on_varchar_kat(gpu, hashed):
    """testSemiJoinOnVarcharType: the same with the keys as strings."""
    s, _ = build_set(abi.VARCHAR, [str(v) for v in [10, 30, 30, 35, 36, 37, 50]], hashed=hashed)
    rows, name = probe(s, abi.VARCHAR, [[str(v) for v in range(30, 40)]], hashed=hashed)
    assert [r[-1] for r in rows] == [True, False, False, False, False, True, True, True, False, False]
    assert name == "k_semi_mark_tagged"


@pytest.mark.parametrize("hashed", [False, True])
def test_build_side_nulls_kat(gpu, hashed):
    """testBuildSideNulls: build 0, 1, 2, 2, 3, NULL; probe 0..4 -> true, true, true, true, NULL."""
    s, _ = build_set(abi.BIGINT, [0, 1, 2, 2, 3, None], hashed=hashed)
    rows, _ = probe(s, abi.BIGINT, [[0, 1, 2, 3, 4]], hashed=hashed)
    assert [r[-1] for r in rows] == [True, True, True, True, None]


@pytest.mark.parametrize("hashed", [False, True])
def test_probe_side_nulls_kat(gpu, hashed):
    """testProbeSideNulls: build 0, 1, 3; probe 0, NULL, 1, 2 -> true, NULL, true, false."""
    s, _ = build_set(abi.BIGINT, [0, 1, 3], hashed=hashed)
    rows, _ = probe(s, abi.BIGINT, [[0, None, 1, 2]], hashed=hashed)
    assert [r[-1] for r in rows] == [True, None, True, False]


@pytest.mark.parametrize("hashed", [False, True])
def test_probe_and_build_nulls_kat(gpu, hashed):
    """testProbeAndBuildNulls: build 0, 1, NULL, 3; probe 0, NULL, 1, 2 -> true, NULL, true, NULL."""
    s, _ = build_set(abi.BIGINT, [0, 1, None, 3], hashed=hashed)
    rows, _ = probe(s, abi.BIGINT, [[0, None, 1, 2]], hashed=hashed)
    assert [r[-1] for r in rows] == [True, None, True, None]


# ---- edges ---------------------------------------------------------------------------------------------------------------------
def test_empty_set(gpu):
    # no build page at all, and zero-row build pages only: NULL probes mark false, not NULL
    for pages in ([], [Page([Block.bigint([]), Block.bigint([])], 0)]):
        s = SetSupplier()
        b = SetBuilderOperator(s, [abi.BIGINT, abi.BIGINT], 1)
        for p in pages:
            check(lib().pa_op_add_input(b._h, C.byref(p.to_c()[0])))
        b.finish()
        rows, name = probe(s, abi.BIGINT, [[1, None, 3]])
        assert [r[-1] for r in rows] == [False, False, False]
        assert name == "k_semi_mark_empty"
        assert s.stats() == (0, False)


def test_all_null_set(gpu):
    name = check_marks(abi.BIGINT, [None] * 5, [[1, None, 7]])
    assert name == "k_semi_mark_slots"


@pytest.mark.parametrize("t", [abi.DOUBLE, abi.REAL])
def test_nan_and_signed_zero(gpu, t):
    nan, other_nan = float("nan"), np.frombuffer(np.uint64(0x7FF0000000000123).tobytes(), np.float64)[0]
    if t == abi.REAL:
        other_nan = np.frombuffer(np.uint32(0x7FC01234).tobytes(), np.float32)[0]
    check_marks(t, [nan, -0.0, 1.5], [[other_nan, 0.0, -0.0, 1.5, 2.5, None]])
    check_marks(t, [0.0, 2.0, None], [[-0.0, nan, 2.0]])
    check_marks(t, [other_nan], [[nan, 0.0]])


def test_boolean_keys(gpu):
    # any non-zero byte is true
    check_marks(abi.BOOLEAN, [2], [[1, 0, 255, None]])
    check_marks(abi.BOOLEAN, [0, None], [[7, 0]])
    check_marks(abi.BOOLEAN, [0, 1, 1], [[1, 0, 9]])


def test_varchar_lengths(gpu):
    build = [b"", b"a", b"abcdefghijklmnop", b"abcdefghijklmnopq", b"x" * 100, None]
    probe_vals = [b"", b"a", b"b", b"abcdefghijklmnop", b"abcdefghijklmnoq", b"abcdefghijklmnopq", b"x" * 100, b"x" * 99, None]
    check_marks(abi.VARCHAR, build, [probe_vals])
    check_marks(abi.VARCHAR, build[:-1], [probe_vals])


def test_short_decimal_keys(gpu):
    t = abi.decimal(12, 2)
    s = SetSupplier()
    b = SetBuilderOperator(s, [abi.BIGINT, t], 1)
    to_pages(b, [Page([Block.bigint([0, 1, 2]), Block.decimal([12345, -5, 0])], 3)])
    j = HashSemiJoinOperator(s, [t], 0)
    out = to_pages(j, [Page([Block.decimal([12345, 5, -5, 0, 1])], 5)])
    assert [r[-1] for p in out for r in p.to_rows()] == [True, False, True, True, False]


def raw_marks(j):
    """The mark column of the operator's next output page, from the C page itself (device pages may carry the input's
    dictionary / RLE blocks, which the Python page view does not decode)."""
    out = abi.pa_page()
    assert check(lib().pa_op_get_output(j._h, C.byref(out))) == 1
    n = out.position_count
    col = out.columns[out.channel_count - 1]
    assert col.type == abi.BOOLEAN and col.encoding == abi.FLAT
    if out.mem == abi.MEM_DEVICE:
        marks = download(DeviceBuffer(col.values, n), np.uint8, n).tolist()
        nulls = download(DeviceBuffer(col.nulls, n), np.uint8, n).tolist() if col.nulls else [0] * n
    else:
        marks = list(C.string_at(col.values, n)) if n else []
        nulls = list(C.string_at(col.nulls, n)) if col.nulls else [0] * n
    return [None if nl else bool(m) for m, nl in zip(marks, nulls)]


def test_dictionary_and_rle_probe_keys(gpu):
    s, _ = build_set(abi.BIGINT, [3, 5, None])
    key = Block.dictionary_block(Block.flat(abi.BIGINT, [5, 4, 0], [0, 0, 1]), [0, 1, 2, 2, 0, 1])
    rle = Block.rle(Block.bigint([3]), 6)
    for output_mem in (abi.MEM_HOST, abi.MEM_DEVICE):
        for k in (key, rle):
            j = HashSemiJoinOperator(s, [abi.BIGINT, abi.BIGINT], 0, output_mem=output_mem)
            for page in (Page([k, Block.bigint(list(range(6)))], 6), upload_page(Page([k, Block.bigint(list(range(6)))], 6))):
                j.addInput(page)
                assert raw_marks(j) == expected_marks(abi.BIGINT, [3, 5, None], k.to_pylist()), (output_mem, k.encoding)
            j.close()


def test_heavy_duplicates(gpu):
    rng = np.random.default_rng(7)
    values = [int(v) for v in np.repeat(rng.integers(0, 1 << 20, 500), 64)]
    rng.shuffle(values)
    check_marks(abi.BIGINT, values, [[int(v) for v in rng.integers(0, 1 << 20, 3000)] + values[:1000]])
    check_marks(abi.INTEGER, values, [[int(v) for v in rng.integers(0, 1 << 20, 3000)]], page_rows=10000)


# ---- every layout ----------------------------------------------------------------------------------------------------------------
def _layout_case(build, probe_keys, t=abi.BIGINT):
    s, _ = build_set(t, build)
    rows, name = probe(s, t, [probe_keys])
    assert [r[-1] for r in rows] == expected_marks(t, build, probe_keys)
    assert s.stats() == (expected_size(t, build), any(v is None for v in build))
    return name


def test_dense_keys_take_the_bitmap(gpu):
    rng = np.random.default_rng(1)
    build = [int(v) for v in rng.permutation(200000)[:120000]]
    assert _layout_case(build, [int(v) for v in rng.integers(-100, 200100, 50001)]) == "k_semi_mark_bitmap"
    assert _layout_case([int(v) for v in rng.integers(0, 50000, 20000)], [int(v) for v in rng.integers(0, 50000, 20000)], abi.DATE) == "k_semi_mark_bitmap"


@pytest.mark.parametrize("with_nulls", [False, True])
def test_sparse_keys_take_the_slot_table(gpu, with_nulls):
    rng = np.random.default_rng(2)
    keys = rng.integers(0, 1 << 40, 60000)
    build = [int(v) for v in keys] + ([None] * 7 if with_nulls else [])
    probe_keys = [int(v) for v in keys[:20000]] + [int(v) for v in rng.integers(0, 1 << 40, 20000)] + [None]
    assert _layout_case(build, probe_keys) == "k_semi_mark_slots"


def test_large_sparse_set_built_in_partitions(gpu):
    """2^21 keys: the partitioned build of the keyed table (probe sequences wrap inside a partition)."""
    rng = np.random.default_rng(3)
    keys = rng.integers(-(1 << 40), 1 << 40, 1 << 21)
    s = SetSupplier()
    b = SetBuilderOperator(s, [abi.BIGINT], 0)
    to_pages(b, [Page([Block.bigint(keys)], len(keys))])
    probe_keys = np.concatenate([keys[::3], rng.integers(-(1 << 40), 1 << 40, 1 << 20)])
    j = HashSemiJoinOperator(s, [abi.BIGINT], 0)
    out = to_pages(j, [Page([Block.bigint(probe_keys)], len(probe_keys))])
    marks = np.concatenate([p.blocks[-1].values for p in out]).astype(bool)
    assert np.array_equal(marks, np.isin(probe_keys, keys))
    assert j.kernelName() == "k_semi_mark_slots"
    assert s.stats() == (len(np.unique(keys)), False)


def test_without_rank_index(gpu, monkeypatch):
    monkeypatch.setenv("PRESTO_AMD_NO_RANK_INDEX", "1")
    rng = np.random.default_rng(4)
    build = [int(v) for v in rng.permutation(100000)[:70000]]
    assert _layout_case(build, [int(v) for v in rng.integers(0, 100000, 30000)]) == "k_semi_mark_bitmap"


# ---- pages -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("output_mem", [abi.MEM_HOST, abi.MEM_DEVICE])
@pytest.mark.parametrize("device_input", [False, True])
def test_several_pages_host_and_device(gpu, output_mem, device_input):
    rng = np.random.default_rng(5)
    build = [int(v) for v in rng.integers(0, 5000, 3000)] + [None]
    pages = [[int(v) if rng.random() > 0.1 else None for v in rng.integers(0, 6000, n)] for n in (1, 5, 1000, 4097, 3)]
    check_marks(abi.BIGINT, build, pages, output_mem=output_mem, device_input=device_input)
    check_marks(abi.VARCHAR, [None if v is None else str(v) for v in build], [[None if v is None else str(v) for v in p] for p in pages],
                output_mem=output_mem, device_input=device_input)


def test_pass_through_channels_are_the_input(gpu):
    s, _ = build_set(abi.BIGINT, [1, 2, 3])
    names = Block.varchar(["a", None, "ccc", "dd"])
    dic = Block.dictionary_block(Block.varchar(["x", "yy"]), [1, 0, 0, 1])
    types = [abi.VARCHAR, abi.BIGINT, abi.VARCHAR, abi.DOUBLE]
    host = Page([names, Block.bigint([1, 5, 3, 4]), dic, Block.double([0.5, -1.0, 2.0, 3.0])], 4)
    for output_mem in (abi.MEM_HOST, abi.MEM_DEVICE):
        j = HashSemiJoinOperator(s, types, 1, output_mem=output_mem)
        j.addInput(host)
        out = j.getOutput()
        if out.mem == abi.MEM_DEVICE:
            out = download_page(out)
        assert [r[:-1] for r in out.to_rows()] == host.to_rows()
        assert [r[-1] for r in out.to_rows()] == [True, False, True, False]

    # device -> device: the input blocks themselves, encodings included; only the mark is new (no nulls: no NULL mark)
    dev = upload_page(host)
    j = HashSemiJoinOperator(s, types, 1, output_mem=abi.MEM_DEVICE)
    cpage, _keep = dev.to_c()
    check(lib().pa_op_add_input(j._h, C.byref(cpage)))
    out = abi.pa_page()
    assert check(lib().pa_op_get_output(j._h, C.byref(out))) == 1
    assert out.channel_count == 5 and out.position_count == 4
    for c in range(4):
        assert out.columns[c].encoding == cpage.columns[c].encoding
        assert out.columns[c].values == cpage.columns[c].values
        assert out.columns[c].offsets == cpage.columns[c].offsets
        assert out.columns[c].nulls == cpage.columns[c].nulls
        assert out.columns[c].ids == cpage.columns[c].ids
    assert out.columns[2].dictionary[0].values == cpage.columns[2].dictionary[0].values
    assert out.columns[4].type == abi.BOOLEAN and out.columns[4].encoding == abi.FLAT and not out.columns[4].nulls
    j.close()


def test_semi_join_retained_pages_are_released_exactly_once(gpu):
    """A PA_PAGE_RETAINED probe page is released once its output page has been let go -- not before (the zero-copy output page IS the
    input's blocks: the release callback scribbles over them) -- and exactly once, also when the operator is closed over a pending
    output.  The set holds a NULL, so every miss is a NULL mark: the mark column carries its NULL flags."""
    from tests.test_gpu_row_number import host_page_of, raw_output
    from tests.test_gpu_small_pages import retained_pages
    n = 5000
    keys = np.arange(n, dtype=np.int64) % 97
    host = Page([Block.bigint(keys), Block.double(np.arange(n, dtype=np.float64))], n)
    bounds = [0, 700, 701, 2000, n]
    build = list(range(0, 98, 2)) + [None]                               # 49 keys and a NULL
    assert len(build) == 50
    want = expected_marks(abi.BIGINT, build, keys.tolist())
    assert set(want) == {True, None}
    s, _builder = build_set(abi.BIGINT, build)
    released = []
    pages = retained_pages(host, bounds, released)
    j = HashSemiJoinOperator(s, [abi.BIGINT, abi.DOUBLE], 0, output_mem=abi.MEM_DEVICE)
    for i, p in enumerate(pages):
        lo, hi = bounds[i], bounds[i + 1]
        assert j.needsInput()
        j.addInput(p)
        assert released == list(range(i))                                # page i is still held
        out = raw_output(j)
        assert out is not None and out.mem == abi.MEM_DEVICE and out.position_count == hi - lo and out.channel_count == 3
        got = host_page_of(j, out)                                       # reads the caller's blocks: they must still be intact
        assert np.array_equal(got.blocks[0].values[:hi - lo], keys[lo:hi])
        assert np.array_equal(got.blocks[1].values[:hi - lo], np.arange(lo, hi, dtype=np.float64))
        assert got.blocks[2].to_pylist() == want[lo:hi]
        assert released == list(range(i))                                # ... while its output page is out
        j.needsInput()                                                   # the output page has been let go
        assert released == list(range(i + 1))
    j.finish()
    j.close()
    assert released == list(range(len(pages)))

    # closed while an output page is still pending: the page goes back once, at close
    released = []
    pages = retained_pages(host, bounds, released)
    j = HashSemiJoinOperator(s, [abi.BIGINT, abi.DOUBLE], 0, output_mem=abi.MEM_DEVICE)
    j.addInput(pages[0])
    assert not j.needsInput() and released == []
    j.close()
    assert released == [0]
    del j
    assert released == [0]


# ---- sharing and lifetime --------------------------------------------------------------------------------------------------------
def test_sharing_and_lifetimes(gpu):
    s = SetSupplier()
    b = SetBuilderOperator(s, [abi.BIGINT], 0)
    j1 = HashSemiJoinOperator(s, [abi.BIGINT], 0)
    assert j1.isBlocked() and not j1.needsInput()
    page = Page([Block.bigint([1, 2, 9])], 3)
    assert lib().pa_op_add_input(j1._h, C.byref(page.to_c()[0])) == abi.ERR_ILLEGAL_STATE   # the set is not built yet
    size, has_null = C.c_int64(), C.c_int32()
    assert lib().pa_channel_set_stats(s._h, C.byref(size), C.byref(has_null)) == abi.ERR_ILLEGAL_STATE
    # a second builder on the same set
    h = C.c_void_p()
    f = SetBuilderOperatorFactory([abi.BIGINT], 0)
    assert f._create(C.byref(f._desc), s._h, C.byref(h)) == abi.ERR_ILLEGAL_STATE
    to_pages(b, [Page([Block.bigint([2, 3, 9])], 3)])
    b.close()                               # builder closed before probing
    j2 = HashSemiJoinOperator(s, [abi.BIGINT], 0)
    s.destroy()                             # set handle destroyed before the probe operators close
    assert not j1.isBlocked() and j1.needsInput()
    for j in (j1, j2):
        out = to_pages(j, [page])
        assert [r[-1] for p in out for r in p.to_rows()] == [False, True, True]
        j.close()


def test_mismatched_key_types(gpu):
    s, _ = build_set(abi.BIGINT, [1])
    h = C.c_void_p()
    f = HashSemiJoinOperatorFactory([abi.INTEGER], 0)
    assert f._create(C.byref(f._desc), s._h, C.byref(h)) == abi.ERR_INVALID_ARGUMENT
    # short DECIMAL: precision and scale are part of the type (unscaled values of different scales are not comparable)
    d, _ = build_set(abi.decimal(12, 2), [100, 250])
    f = HashSemiJoinOperatorFactory([abi.decimal(12, 4)], 0)
    assert f._create(C.byref(f._desc), d._h, C.byref(h)) == abi.ERR_INVALID_ARGUMENT
    f = HashSemiJoinOperatorFactory([abi.decimal(12, 2)], 0)
    assert f._create(C.byref(f._desc), d._h, C.byref(h)) == abi.OK
    check(lib().pa_op_close(h))


# ---- seeded fuzz -----------------------------------------------------------------------------------------------------------------
FUZZ_SEEDS = int(os.environ.get("PA_FUZZ_SEEDS", "16"))
FUZZ_TYPES = [abi.BIGINT, abi.INTEGER, abi.DATE, abi.DOUBLE, abi.REAL, abi.BOOLEAN, abi.VARCHAR]


def _fuzz_values(rng, t, n, domain, null_rate):
    raw = rng.integers(-domain, domain, n)
    out = []
    for v in raw:
        if rng.random() < null_rate:
            out.append(None)
        elif t in (abi.DOUBLE, abi.REAL):
            r = rng.random()
            out.append(float("nan") if r < 0.05 else (-0.0 if r < 0.1 else float(v) / 4))
        elif t == abi.BOOLEAN:
            out.append(int(v) & 0xFF)
        elif t == abi.VARCHAR:
            out.append(("k%d" % v) * int(1 + abs(v) % 5))
        else:
            out.append(int(v))
    return out


@pytest.mark.parametrize("seed", range(FUZZ_SEEDS))
def test_fuzz(gpu, seed):
    rng = np.random.default_rng(1000 + seed)
    t = FUZZ_TYPES[int(rng.integers(0, len(FUZZ_TYPES)))]
    domain = int(rng.choice([8, 1000, 1 << 20, 1 << 40])) if t not in (abi.INTEGER, abi.DATE, abi.VARCHAR) else int(rng.choice([8, 1000, 1 << 20]))
    dup = int(rng.choice([1, 4, 64]))
    distinct = _fuzz_values(rng, t, int(rng.integers(0, 3000)), domain, float(rng.choice([0.0, 0.01, 0.3])))
    build = [v for v in distinct for _ in range(dup)]
    order = rng.permutation(len(build))
    build = [build[i] for i in order]
    probe_rate = float(rng.choice([0.0, 0.05, 0.5]))
    pages = [_fuzz_values(rng, t, int(n), domain, probe_rate) for n in rng.integers(1, 5000, int(rng.integers(1, 4)))]
    hashed = bool(rng.integers(0, 2))
    encoding = int(rng.integers(0, 3))
    s, _ = build_set(t, build, hashed=hashed, page_rows=int(rng.choice([97, 1000, 1 << 20])))
    types = [t, abi.BIGINT]
    output_mem = int(rng.integers(0, 2))
    j = HashSemiJoinOperator(s, types, 0, output_mem=output_mem)
    got, want = [], []
    for vals in pages:
        key = block(t, vals)
        if encoding == 1:   # dictionary: the page's values through a shuffled dictionary
            perm = rng.permutation(len(vals))
            key = Block.dictionary_block(block(t, [vals[i] for i in perm]), np.argsort(perm))
        elif encoding == 2:   # RLE of the page's first value
            key = Block.rle(block(t, vals[:1]), len(vals))
            vals = vals[:1] * len(vals)
        page = Page([key, Block.bigint(list(range(len(vals))))], len(vals))
        if rng.integers(0, 2):
            page = upload_page(page)
        j.addInput(page)
        got += raw_marks(j)
        want += expected_marks(t, build, vals)
    assert got == want, (seed, t)
    assert s.stats() == (expected_size(t, build), any(v is None for v in build)), (seed, t)
