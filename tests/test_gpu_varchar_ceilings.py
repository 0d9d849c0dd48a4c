"""The 2 GiB ceilings of VARCHAR columns: exact below, refused above.

A VARCHAR column on the device has 32-bit offsets, so every place that builds one from rows -- gathers by position, the dictionary / RLE
decode of the page stager, the accumulation of pages (HeldRows, the hash build), the interner's decode, the exchange -- has a ceiling of
2^31 bytes.  Each of them is driven here to just below the ceiling (the output is compared, every offset and every byte), to exactly
2^31 bytes (refused: INSUFFICIENT_RESOURCES from the call DESIGN.md's "32-bit ceilings" table names, with the site's message) and, where
the byte total multiplies, to 2^32 + L bytes, which wraps to a small positive 32-bit total that a sign check would let through.

Inputs are device pages over ONE pattern buffer of 2^31 bytes (byte j is a hash of j); string i is a window of it, so an output row is
checked against the pattern where its source row lies -- nothing near 2 GiB ever crosses to the host.  The expected rows and their order
come from plain Python over the small row lists.  The GPU tests carry the gpu mark one by one (not as a module mark): the dry run of the
comparison helper at the end of the file runs on the CPU."""
import ctypes as C

import numpy as np
import pytest
import torch

from presto_amd import abi
from presto_amd._lib import PrestoAmdError, check, lib
from presto_amd.exchange import Comm, ExchangeOperator
from presto_amd.expr import field
from presto_amd.operators import (FilterAndProjectOperator, HashAggregationOperator, HashBuilderOperator, LookupJoinOperator, LookupSourceFactory,
                                  NestedLoopBuildOperator, NestedLoopJoinBridge, NestedLoopJoinOperator, OrderByOperator, StreamingAggregationOperator,
                                  TopNRankingOperator)
from presto_amd.page import Block, DeviceBuffer, Page

on_gpu = pytest.mark.gpu

L = 65536                      # bytes of a full string
CEILING = 1 << 31              # the first byte total that 32-bit offsets cannot hold
BELOW, AT, OVER, WRAPPED = CEILING - L - 3, CEILING - 1, CEILING, (1 << 32) + L
CHUNK = 32 << 20               # bytes compared at a time (the index arithmetic of a chunk takes about 50 bytes per byte compared)
ODD = [(0, False), (1, False), (7, False), (L - 1, False), (0, True)]   # (length, is NULL): rows that keep the offsets off multiples of L

STAGER = "a dictionary / RLE VARCHAR block decodes to more than 2 GiB"
JOIN_PAGE = "a join output page holds more than 2 GiB of VARCHAR bytes"
HELD = "VARCHAR column exceeds 2 GB"
BUILD = "build VARCHAR column exceeds 2 GB"
INTERNER = "VARCHAR key column exceeds 2 GiB"
HELPERS = "do not fit one block's 32-bit offsets"
DELIVERED = "more than 2 GiB of VARCHAR bytes delivered to one rank"
RUN_KEYS = "the group keys of the runs a page closes, the carried run's among them, hold more than 2 GB"


# ---- the pattern and the comparison: torch on whatever device the pattern lives on ------------------------------------------------------------
def pattern(lo, hi, device):
    """bytes [lo, hi) of the pattern: byte j = a multiplicative hash of j (no two windows of it are equal)"""
    j = torch.arange(lo, hi, dtype=torch.int64, device=device)
    x = j * 0x9E3779B1          # (j < 2^31: the product stays below 2^63)
    return (((x >> 24) ^ (x >> 11) ^ j) & 0xFF).to(torch.uint8)


def check_varchar(offsets, values, nulls, expected, pat, chunk=CHUNK):
    """A VARCHAR column (offsets: n + 1 int32, values: its bytes, nulls: n flags or None) against `expected`: per row (where its bytes
    start in the pattern, how many) or None for NULL.  Every offset against the int64 running sum of the expected lengths, every flag,
    and every byte against the pattern, `chunk` bytes at a time.  Returns the byte total."""
    dev = pat.device
    n = len(expected)
    start = torch.tensor([0 if e is None else e[0] for e in expected], dtype=torch.int64, device=dev)
    length = torch.tensor([0 if e is None else e[1] for e in expected], dtype=torch.int64, device=dev)
    null = torch.tensor([e is None for e in expected], dtype=torch.bool, device=dev)
    want = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    want[1:] = torch.cumsum(length, 0)
    total = int(want[n])
    assert total < CEILING, "the expected column itself does not fit 32-bit offsets: %d bytes" % total
    assert offsets.numel() == n + 1, (offsets.numel(), n + 1)
    got = offsets.to(torch.int64)
    if not torch.equal(got, want):
        bad = int(torch.nonzero(got != want)[0])
        raise AssertionError("offset %d of %d is %d, expected %d" % (bad, n, int(got[bad]), int(want[bad])))
    if nulls is None:
        assert not bool(null.any()), "NULL rows expected, and the block has no flags"
    elif not torch.equal(nulls != 0, null):
        bad = int(torch.nonzero((nulls != 0) != null)[0])
        raise AssertionError("NULL flag of row %d is %d" % (bad, int(nulls[bad])))
    assert values.numel() >= total, (values.numel(), total)
    for lo in range(0, total, chunk):
        hi = min(lo + chunk, total)
        at = torch.arange(lo, hi, dtype=torch.int64, device=dev)
        row = torch.searchsorted(want, at, right=True) - 1       # want[row] <= at < want[row + 1]: rows of length 0 own no byte
        src = start[row] + (at - want[row])
        same = values[lo:hi] == pat[src]
        if not bool(same.all()):
            bad = int(torch.nonzero(~same)[0])
            raise AssertionError("byte %d (row %d, byte %d of it) is %d, expected %d"
                                 % (lo + bad, int(row[bad]), lo + bad - int(want[row[bad]]), int(values[lo + bad]), int(pat[src[bad]])))
        del at, row, src, same
    return total


# ---- device memory as torch tensors, torch tensors as blocks ---------------------------------------------------------------------------------
class _Span:
    def __init__(self, ptr, count, typestr):
        self.__cuda_array_interface__ = {"shape": (count,), "typestr": typestr, "data": (int(ptr), False), "version": 2, "strides": None}


def device_tensor(ptr, count, typestr):
    """count items at a device address as a torch tensor (a view: valid as long as the operator keeps the page)"""
    if count == 0:
        return torch.zeros(0, dtype={"|u1": torch.uint8, "<i4": torch.int32, "<i8": torch.int64}[typestr], device="cuda")
    return torch.as_tensor(_Span(ptr, count, typestr), device="cuda")


def column_tensors(page, channel):
    """(offsets, values, nulls) of a VARCHAR channel, or (values, nulls) of a BIGINT channel, of a device output page"""
    assert page.mem == abi.MEM_DEVICE
    b = page.blocks[channel]
    n = page.position_count
    nulls = device_tensor(b.nulls.ptr, n, "|u1") if b.nulls is not None else None
    if b.type == abi.VARCHAR:
        assert b.encoding == abi.VARWIDTH
        offsets = device_tensor(b.offsets.ptr, n + 1, "<i4")
        total = int(offsets[n])
        assert 0 <= total < CEILING, total
        return offsets, device_tensor(b.values.ptr, total, "|u1"), nulls
    assert b.type == abi.BIGINT and b.encoding == abi.FLAT
    return device_tensor(b.values.ptr, n, "<i8"), nulls


def buffer_of(t):
    return DeviceBuffer(t.data_ptr(), t.numel() * t.element_size(), t)


def bigint_block(values):
    t = values if torch.is_tensor(values) else torch.tensor(values, dtype=torch.int64, device="cuda")
    return Block(abi.BIGINT, abi.FLAT, t.numel(), values=buffer_of(t))


def varchar_block(P, base, rows):
    """rows (length, is NULL) as a VariableWidthBlock over the pattern from byte `base` on; its offsets start at 0"""
    lengths = [l for l, _ in rows]
    total = sum(lengths)
    assert base + total <= P.numel() and total < CEILING, (base, total)       # the input itself is a legal block
    off = torch.zeros(len(rows) + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(torch.tensor(lengths, dtype=torch.int64), 0)
    assert int(off[-1]) == total
    off = off.to(torch.int32).cuda()
    nulls = torch.tensor([1 if z else 0 for _, z in rows], dtype=torch.uint8, device="cuda") if any(z for _, z in rows) else None
    return Block(abi.VARCHAR, abi.VARWIDTH, len(rows), values=DeviceBuffer(P.data_ptr() + base, max(total, 1), P), offsets=buffer_of(off),
                 nulls=buffer_of(nulls) if nulls is not None else None)


def where(base, rows):
    """per row of varchar_block(P, base, rows): (its first byte in the pattern, its length), or None for NULL"""
    out, at = [], base
    for l, z in rows:
        out.append(None if z else (at, l))
        at += l
    return out


def ceiling_rows(total):
    """rows whose lengths sum to exactly `total`: full strings, with the odd rows at the start, the middle and the end"""
    full, rest = divmod(total - 3 * (L + 7), L)
    rows = ODD + [(L, False)] * (full // 2) + ODD + ([(rest, False)] if rest else []) + [(L, False)] * (full - full // 2) + ODD
    assert sum(l for l, _ in rows) == total
    return rows


def sort_key(i):
    return (i * 40503) % 65521     # (pairwise different below 65521 rows)


class Source:
    """`rows` as `pages` device pages [VARCHAR, BIGINT sort key, BIGINT row id, BIGINT 0] over the pattern (about a quarter of the bytes each)"""

    def __init__(self, P, rows, pages=4):
        n = len(rows)
        assert n < 65521
        self.rows, self.where, self.pages = rows, where(0, rows), []
        cuts = [n * k // pages for k in range(pages + 1)]
        base = 0
        for lo, hi in zip(cuts, cuts[1:]):
            part = rows[lo:hi]
            ids = list(range(lo, hi))
            self.pages.append(Page([varchar_block(P, base, part), bigint_block([sort_key(i) for i in ids]), bigint_block(ids),
                                    bigint_block([0] * len(ids))], hi - lo, abi.MEM_DEVICE))
            base += sum(l for l, _ in part)
        self.total = base
        torch.cuda.synchronize()       # the operators run on streams of their own


TYPES = [abi.VARCHAR, abi.BIGINT, abi.BIGINT, abi.BIGINT]


@pytest.fixture(scope="module")
def P(gpu):
    torch.cuda.set_device(0)
    p = torch.empty(CEILING, dtype=torch.uint8, device="cuda")
    for lo in range(0, CEILING, CHUNK):
        p[lo:lo + CHUNK] = pattern(lo, lo + CHUNK, "cuda")
    torch.cuda.synchronize()
    return p


@pytest.fixture(autouse=True)
def release_torch_cache(request):
    """the comparison's temporaries go back to the device after every GPU test: the operators' pool is another allocator"""
    yield
    if request.node.get_closest_marker("gpu"):
        torch.cuda.empty_cache()


def refused(call, words):
    with pytest.raises(PrestoAmdError) as e:
        call()
    assert e.value.status == abi.ERR_INSUFFICIENT_RESOURCES, e.value
    assert words in e.value.message, e.value.message
    assert words in lib().pa_last_error().decode(), lib().pa_last_error()


def check_pages(op, P, expected, ids, varchar_channel, id_channel):
    """the operator's output pages, one after the other, against `expected` (check_varchar's rows) and the row ids; returns the page count"""
    at = pages = 0
    while True:
        page = op.getOutput()
        if page is None:
            break
        check(lib().pa_device_synchronize())
        m = page.position_count
        assert m > 0 and at + m <= len(expected), (at, m, len(expected))
        check_varchar(*column_tensors(page, varchar_channel), expected[at:at + m], P)
        if id_channel is not None:
            got, nulls = column_tensors(page, id_channel)
            assert torch.equal(got, torch.tensor(ids[at:at + m], dtype=torch.int64, device="cuda"))
        at += m
        pages += 1
        del page
    assert at == len(expected), (at, len(expected))
    return pages


def host_rows(op, pages):
    out = []
    for p in pages:
        op.addInput(p)
        q = op.getOutput()
        out += q.to_rows() if q is not None else []
    op.finish()
    while True:
        q = op.getOutput()
        if q is None:
            break
        out += q.to_rows()
    op.close()
    return out


# ---- the view of device memory the comparisons rest on -----------------------------------------------------------------------------------------
@on_gpu
def test_device_views_read_the_memory_they_name(gpu, P):
    assert torch.equal(device_tensor(P.data_ptr() + 12345, 1000, "|u1"), P[12345:13345])
    assert torch.equal(P[CEILING - 4096:].cpu(), pattern(CEILING - 4096, CEILING, "cpu"))
    t = torch.arange(-5, 5, dtype=torch.int64, device="cuda")
    assert torch.equal(device_tensor(t.data_ptr(), 10, "<i8"), t)


# ---- the ABI helpers ------------------------------------------------------------------------------------------------------------------------
def gather_offsets(src_off, positions):
    k = positions.numel()
    out = torch.empty(k + 1, dtype=torch.int32, device="cuda")
    total = C.c_int64(-1)
    torch.cuda.synchronize()
    rc = lib().pa_varwidth_gather_offsets(src_off.data_ptr(), positions.data_ptr(), k, None, out.data_ptr(), C.byref(total), None)
    return rc, total.value, out


@on_gpu
def test_abi_gather_offsets(gpu, P):
    """pa_varwidth_gather_offsets with positions repeating one L-byte row: the 64-bit total comes back whatever it is, the status says
    whether the offsets hold it"""
    rows = [(L, False), (7, False), (0, False)]
    src_off = torch.tensor([0, L, L + 7, L + 7], dtype=torch.int32, device="cuda")
    src = where(0, rows)
    positions = [0] * 16000 + [1, 2] + [0] * 16767
    rc, total, out = gather_offsets(src_off, torch.tensor(positions, dtype=torch.int32, device="cuda"))
    assert rc == abi.OK and total == 32767 * L + 7 and CEILING - 2 * L < total < CEILING - 1
    values = torch.empty(total, dtype=torch.uint8, device="cuda")
    pos = torch.tensor(positions, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    check(lib().pa_varwidth_gather_bytes(P.data_ptr(), src_off.data_ptr(), pos.data_ptr(), len(positions), out.data_ptr(), values.data_ptr(), None))
    assert check_varchar(out, values, None, [src[p] for p in positions], P) == total
    del values
    for count, want in ((32768, OVER), (65537, WRAPPED)):
        rc, total, out = gather_offsets(src_off, torch.zeros(count, dtype=torch.int32, device="cuda"))
        assert total == want, (total, want)                       # the true total, not its low 32 bits
        assert rc == abi.ERR_INSUFFICIENT_RESOURCES and HELPERS in lib().pa_last_error().decode()
    rc, total, out = gather_offsets(src_off, torch.tensor([1, 0, 2, 1, 1], dtype=torch.int32, device="cuda"))   # the known answer afterwards
    assert rc == abi.OK and total == L + 21 and out.tolist() == [0, 7, L + 7, L + 7, L + 14, L + 21]


@on_gpu
def test_abi_offsets_from_lengths(gpu):
    def scan(lengths):
        t = torch.tensor(lengths, dtype=torch.int32, device="cuda")
        out = torch.empty(len(lengths) + 1, dtype=torch.int32, device="cuda")
        total = C.c_int64(-1)
        torch.cuda.synchronize()
        rc = lib().pa_offsets_from_lengths(t.data_ptr(), len(lengths), out.data_ptr(), C.byref(total), None)
        return rc, total.value, out
    lengths = [l for l, _ in ceiling_rows(AT)]
    rc, total, out = scan(lengths)
    assert rc == abi.OK and total == AT
    assert torch.equal(out.to(torch.int64).cpu(), torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(torch.tensor(lengths, dtype=torch.int64), 0)]))
    for lengths, want in (([l for l, _ in ceiling_rows(OVER)], OVER), ([L] * 65537, WRAPPED)):
        rc, total, out = scan(lengths)
        assert total == want, (total, want)
        assert rc == abi.ERR_INSUFFICIENT_RESOURCES and HELPERS in lib().pa_last_error().decode()
    rc, total, out = scan([3, 0, 4])
    assert rc == abi.OK and total == 7 and out.tolist() == [0, 3, 3, 7]


# ---- the page stager: RLE and DICTIONARY over a VARCHAR dictionary, through FilterAndProject ----------------------------------------------------
def filter_project():
    return FilterAndProjectOperator([abi.VARCHAR, abi.BIGINT], field(1, abi.BIGINT) >= 0, [field(0, abi.VARCHAR), field(1, abi.BIGINT)],
                                    output_mem=abi.MEM_DEVICE)


def filter_project_known_answer():
    op = FilterAndProjectOperator([abi.VARCHAR, abi.BIGINT], field(1, abi.BIGINT) >= 0, [field(0, abi.VARCHAR), field(1, abi.BIGINT)])
    page = Page([Block.dictionary_block(Block.varchar([b"ab", None, b""]), [0, 1, 2, 0, 0]), Block.bigint([1, 2, 3, 4, 5])])
    assert host_rows(op, [page]) == [(b"ab", 1), (None, 2), (b"", 3), (b"ab", 4), (b"ab", 5)]


def stager_leg(P, block, expected):
    """the block, with a BIGINT channel beside it, through FilterAndProject under a filter every row passes: exact when `expected` is a
    row list, refused by addInput when it is None"""
    n = block.position_count
    ids = list(range(n))
    page = Page([block, bigint_block(ids)], n, abi.MEM_DEVICE)
    torch.cuda.synchronize()
    op = filter_project()
    if expected is None:
        refused(lambda: op.addInput(page), STAGER)
        op.close()
        filter_project_known_answer()
    else:
        op.addInput(page)
        assert check_pages(op, P, expected, ids, 0, 1) == 1
        op.finish()
        op.close()


@on_gpu
@pytest.mark.parametrize("n,total", [(32767, CEILING - L), (32768, OVER), (65537, WRAPPED)], ids=["below", "over", "wrapped"])
def test_stager_rle(gpu, P, n, total):
    """One L-byte value x n positions.  (There is no `at` leg: 2^31 - 1 is prime, so only ONE position of a 2^31 - 1 byte value reaches
    it, which k_varwidth_copy would copy with a single lane; the DICTIONARY legs reach it through the same lines of the stager.)"""
    assert n * L == total
    block = Block(abi.VARCHAR, abi.RLE, n, dictionary=varchar_block(P, 4099, [(L, False)]))
    stager_leg(P, block, [(4099, L)] * n if total < CEILING else None)


def dictionary_ids(fulls, fives):
    """ids over the dictionary {L bytes, empty, 5 bytes, NULL}: mostly entry 0, the others at the start, in between and at the end"""
    ids = [1, 3, 2] + [0] * fulls + [3, 1]
    step = max(1, fulls // max(fives - 1, 1))
    for k in range(fives - 1):
        ids.insert(3 + k * (step + 1), 2)
    return ids


@on_gpu
@pytest.mark.parametrize("fulls,fives,total", [(32767, 13106, AT - 5), (32767, 13107, AT), (32768, 0, OVER), (65537, 0, WRAPPED)],
                         ids=["below", "at", "over", "wrapped"])
def test_stager_dictionary(gpu, P, fulls, fives, total):
    entries = [(L, False), (0, False), (5, False), (0, True)]
    ids = dictionary_ids(fulls, fives) if fives else [1, 3] + [0] * fulls + [3, 1]
    src = where(777, entries)
    assert sum(entries[i][0] for i in ids) == total and (total >= CEILING or CEILING - 2 * L < total <= AT)
    t = torch.tensor(ids, dtype=torch.int32, device="cuda")
    block = Block(abi.VARCHAR, abi.DICTIONARY, len(ids), ids=buffer_of(t), dictionary=varchar_block(P, 777, entries))
    stager_leg(P, block, [src[i] for i in ids] if total < CEILING else None)


# ---- LookupJoin: the output rows multiply ------------------------------------------------------------------------------------------------------
SMALL = [(L, False), (1, False), (7, False), (L - 1, False), (0, True), (0, False)]     # the string side: keys 7 .. 12
SMALL_KEYS = [7, 8, 9, 10, 11, 12]
ABSENT = 99


def big_keys(total):
    """keys of the BIGINT-only side so that the matched strings hold `total` bytes: key 7 (L bytes) for most rows, the odd ones among them"""
    fulls, rest = divmod(total, L)
    extra = {0: [], 8: [8, 9], L - 1: [10]}[rest]          # (1 + 7 bytes, or L - 1)
    keys = [12, 11, ABSENT] + [7] * (fulls // 2) + extra + [ABSENT, 11] + [7] * (fulls - fulls // 2) + [12, ABSENT]
    return keys


def joined(build_keys, probe_keys, outer):
    """(probe row, build row or None) in emission order: probe-major, a probe row's matches from the last build row to the first
    (joined_rows of test_gpu_type_matrix.py)"""
    positions = {}
    for i, k in enumerate(build_keys):
        positions.setdefault(k, []).append(i)
    out = []
    for p, k in enumerate(probe_keys):
        matches = positions.get(k, [])
        out += [(p, b) for b in reversed(matches)]
        if outer and not matches:
            out.append((p, None))
    return out


def join_known_answer():
    bridge = LookupSourceFactory()
    builder = HashBuilderOperator(bridge, [abi.BIGINT, abi.VARCHAR], [0], [1])
    builder.addInput(Page([Block.bigint([7, 8, 7]), Block.varchar([b"x", None, b"yy"])]))
    builder.finish()
    op = LookupJoinOperator(bridge, [abi.BIGINT, abi.BIGINT], [0], [0, 1], join_type=abi.JOIN_PROBE_OUTER)
    got = host_rows(op, [Page([Block.bigint([7, 9, 8, 7, 8]), Block.bigint([0, 1, 2, 3, 4])])])
    assert got == [(7, 0, b"yy"), (7, 0, b"x"), (9, 1, None), (8, 2, None), (7, 3, b"yy"), (7, 3, b"x"), (8, 4, None)]
    builder.close()
    bridge.destroy()


def join_build_multiplies(P, total, join_type, min_pages=1):
    """build: the six strings; probe: BIGINT keys and row ids.  Output: [probe row id, the build string]"""
    keys = big_keys(total)
    pairs = joined(SMALL_KEYS, keys, join_type == abi.JOIN_PROBE_OUTER)
    src = where(31, SMALL)
    expected = [None if b is None else src[b] for _, b in pairs]
    bridge = LookupSourceFactory()
    builder = HashBuilderOperator(bridge, [abi.BIGINT, abi.VARCHAR], [0], [1])
    build_page = Page([bigint_block(SMALL_KEYS), varchar_block(P, 31, SMALL)], len(SMALL), abi.MEM_DEVICE)
    probe_page = Page([bigint_block(keys), bigint_block(list(range(len(keys))))], len(keys), abi.MEM_DEVICE)
    torch.cuda.synchronize()
    builder.addInput(build_page)
    builder.finish()
    op = LookupJoinOperator(bridge, [abi.BIGINT, abi.BIGINT], [0], [1], output_mem=abi.MEM_DEVICE, join_type=join_type)
    op.addInput(probe_page)
    matched = sum(0 if e is None else e[1] for e in expected)
    assert matched == total
    if total >= CEILING and min_pages == 1:
        refused(op.getOutput, JOIN_PAGE)
    else:
        pages = check_pages(op, P, expected, [p for p, _ in pairs], 1, 0)
        assert pages >= min_pages and (min_pages > 1 or pages == 1), pages
        op.finish()
    op.close()
    builder.close()
    bridge.destroy()
    if total >= CEILING:
        join_known_answer()


@on_gpu
@pytest.mark.parametrize("total", [CEILING - L + 8, AT, OVER, WRAPPED], ids=["below", "at", "over", "wrapped"])
@pytest.mark.parametrize("join_type", [abi.JOIN_INNER, abi.JOIN_PROBE_OUTER], ids=["inner", "probe_outer"])
def test_lookup_join_build_side_multiplies(gpu, P, monkeypatch, join_type, total):
    monkeypatch.delenv("PRESTO_AMD_JOIN_MAX_OUTPUT_ROWS", raising=False)
    join_build_multiplies(P, total, join_type)


@on_gpu
def test_lookup_join_over_the_ceiling_in_bounded_pages(gpu, P, monkeypatch):
    """the input that is refused as one output page comes out exact as several pages of at most 16384 rows (1 GiB each)"""
    monkeypatch.setenv("PRESTO_AMD_JOIN_MAX_OUTPUT_ROWS", "16384")
    join_build_multiplies(P, OVER, abi.JOIN_PROBE_OUTER, min_pages=2)


@on_gpu
@pytest.mark.parametrize("total", [CEILING - L + 8, AT, OVER, WRAPPED], ids=["below", "at", "over", "wrapped"])
def test_lookup_join_probe_side_multiplies(gpu, P, monkeypatch, total):
    """probe: the six strings; build: BIGINT keys and row ids.  Output: [the probe string, build row id]"""
    monkeypatch.delenv("PRESTO_AMD_JOIN_MAX_OUTPUT_ROWS", raising=False)
    keys = big_keys(total)
    pairs = joined(keys, SMALL_KEYS, False)
    src = where(31, SMALL)
    expected = [src[p] for p, _ in pairs]
    assert sum(0 if e is None else e[1] for e in expected) == total
    bridge = LookupSourceFactory()
    builder = HashBuilderOperator(bridge, [abi.BIGINT, abi.BIGINT], [0], [1])
    build_page = Page([bigint_block(keys), bigint_block(list(range(len(keys))))], len(keys), abi.MEM_DEVICE)
    probe_page = Page([bigint_block(SMALL_KEYS), varchar_block(P, 31, SMALL)], len(SMALL), abi.MEM_DEVICE)
    torch.cuda.synchronize()
    builder.addInput(build_page)
    builder.finish()
    op = LookupJoinOperator(bridge, [abi.BIGINT, abi.VARCHAR], [0], [1], output_mem=abi.MEM_DEVICE)
    op.addInput(probe_page)
    if total >= CEILING:
        refused(op.getOutput, JOIN_PAGE)
    else:
        assert check_pages(op, P, expected, [b for _, b in pairs], 0, 1) == 1
        op.finish()
    op.close()
    builder.close()
    bridge.destroy()
    if total >= CEILING:
        join_known_answer()


# ---- NestedLoopJoin ------------------------------------------------------------------------------------------------------------------------------
def nested_loop_known_answer():
    bridge = NestedLoopJoinBridge()
    builder = NestedLoopBuildOperator(bridge, [abi.VARCHAR])
    builder.addInput(Page([Block.varchar([b"x", None, b"yy", b"", b"z"])]))
    builder.finish()
    op = NestedLoopJoinOperator(bridge, [abi.BIGINT], [0], [0])
    assert host_rows(op, [Page([Block.bigint([4])])]) == [(4, b"x"), (4, None), (4, b"yy"), (4, b""), (4, b"z")]
    builder.close()
    bridge.destroy()


@on_gpu
@pytest.mark.parametrize("total", [BELOW, AT, OVER, WRAPPED], ids=["below", "at", "over", "wrapped"])
def test_nested_loop_join_strings_on_the_build_side(gpu, P, monkeypatch, total):
    """cross join.  below / at: ONE probe row x the build rows whose strings hold the total (the product is the build side, in order);
    over / wrapped: one L-byte build row (and an empty and a NULL one) x 32768 / 65537 probe rows"""
    monkeypatch.delenv("PRESTO_AMD_JOIN_MAX_OUTPUT_ROWS", raising=False)
    bridge = NestedLoopJoinBridge()
    builder = NestedLoopBuildOperator(bridge, TYPES)
    if total < CEILING:
        source = Source(P, ceiling_rows(total))
        for page in source.pages:
            builder.addInput(page)
        probe_ids, expected, ids = [5], source.where, list(range(len(source.rows)))
    else:
        rows = [(0, False), (L, False), (0, True)]
        source = Source(P, rows, pages=1)
        builder.addInput(source.pages[0])
        probe_ids = list(range(total // L))
        expected, ids = source.where * len(probe_ids), [0, 1, 2] * len(probe_ids)
    builder.finish()
    op = NestedLoopJoinOperator(bridge, [abi.BIGINT], [0], [0, 2], output_mem=abi.MEM_DEVICE)
    probe_page = Page([bigint_block(probe_ids)], len(probe_ids), abi.MEM_DEVICE)
    torch.cuda.synchronize()
    op.addInput(probe_page)
    if total >= CEILING:
        refused(op.getOutput, JOIN_PAGE)
    else:
        assert check_pages(op, P, expected, ids, 1, 2) == 1
        op.finish()
    op.close()
    builder.close()
    bridge.destroy()
    del source
    if total >= CEILING:
        nested_loop_known_answer()


@on_gpu
@pytest.mark.parametrize("total", [AT, OVER], ids=["at", "over"])
def test_nested_loop_join_strings_on_the_probe_side(gpu, P, monkeypatch, total):
    """one build row x a probe page whose strings hold the total.  (A probe page is one block, so 2^31 bytes are reached through an RLE
    block, which the stager refuses at addInput; `at` is a plain page.)"""
    monkeypatch.delenv("PRESTO_AMD_JOIN_MAX_OUTPUT_ROWS", raising=False)
    bridge = NestedLoopJoinBridge()
    builder = NestedLoopBuildOperator(bridge, [abi.BIGINT])
    builder.addInput(Page([Block.bigint([3])]))
    builder.finish()
    op = NestedLoopJoinOperator(bridge, [abi.VARCHAR, abi.BIGINT], [0, 1], [0], output_mem=abi.MEM_DEVICE)
    if total < CEILING:
        rows = ceiling_rows(total)
        ids = list(range(len(rows)))
        page = Page([varchar_block(P, 0, rows), bigint_block(ids)], len(rows), abi.MEM_DEVICE)
        torch.cuda.synchronize()
        op.addInput(page)
        assert check_pages(op, P, where(0, rows), ids, 0, 1) == 1
        op.finish()
    else:
        n = total // L
        page = Page([Block(abi.VARCHAR, abi.RLE, n, dictionary=varchar_block(P, 0, [(L, False)])), bigint_block(list(range(n)))], n, abi.MEM_DEVICE)
        torch.cuda.synchronize()
        refused(lambda: op.addInput(page), STAGER)
    op.close()
    builder.close()
    bridge.destroy()
    if total >= CEILING:
        nested_loop_known_answer()


# ---- accumulation over pages: HeldRows (OrderBy, TopNRanking) and the hash build ------------------------------------------------------------------
def accumulate(op, source, words):
    """the pages into the operator: all of them taken, or -- words: the message -- the last one, which crosses the ceiling, refused"""
    for page in source.pages[:-1]:
        op.addInput(page)
    if words is None:
        op.addInput(source.pages[-1])
    else:
        refused(lambda: op.addInput(source.pages[-1]), words)


def order_by_known_answer():
    op = OrderByOperator([abi.VARCHAR, abi.BIGINT], [0, 1], [1], [abi.DESC_NULLS_LAST])
    got = host_rows(op, [Page([Block.varchar([b"a", None, b"ccc"]), Block.bigint([1, 5, 3])]), Page([Block.varchar([b"", b"dd"]), Block.bigint([2, 4])])])
    assert got == [(None, 5), (b"dd", 4), (b"ccc", 3), (b"", 2), (b"a", 1)]


@on_gpu
@pytest.mark.parametrize("total", [BELOW, AT, OVER], ids=["below", "at", "over"])
def test_held_rows_order_by(gpu, P, total):
    """4 pages of about 512 MiB of strings each into OrderBy (HeldRows::append_page), BIGINT key descending"""
    source = Source(P, ceiling_rows(total))
    assert source.total == total
    op = OrderByOperator(TYPES, [0, 2], [1], [abi.DESC_NULLS_LAST], output_mem=abi.MEM_DEVICE)
    accumulate(op, source, HELD if total >= CEILING else None)
    if total < CEILING:
        order = sorted(range(len(source.rows)), key=lambda i: -sort_key(i))
        op.finish()
        assert check_pages(op, P, [source.where[i] for i in order], order, 0, 1) >= 1
    op.close()
    del source
    if total >= CEILING:
        order_by_known_answer()


def topn_ranking_known_answer():
    op = TopNRankingOperator([abi.VARCHAR, abi.BIGINT, abi.BIGINT], [0, 1], [2], [1], [abi.DESC_NULLS_LAST], 100)
    got = host_rows(op, [Page([Block.varchar([b"a", None, b"ccc"]), Block.bigint([1, 5, 3]), Block.bigint([0, 0, 0])]),
                         Page([Block.varchar([b"", b"dd"]), Block.bigint([2, 4]), Block.bigint([0, 0])])])
    assert got == [(None, 5, 1), (b"dd", 4, 2), (b"ccc", 3, 3), (b"", 2, 4), (b"a", 1, 5)]


@on_gpu
@pytest.mark.parametrize("total", [BELOW, AT, OVER], ids=["below", "at", "over"])
def test_held_rows_topn_ranking(gpu, P, total):
    """the same pages into TopNRanking (HeldRows::append_positions), one partition, n above the row count: nothing is pruned"""
    source = Source(P, ceiling_rows(total))
    op = TopNRankingOperator(TYPES, [0, 2], [3], [1], [abi.DESC_NULLS_LAST], 1 << 20, output_mem=abi.MEM_DEVICE)
    accumulate(op, source, HELD if total >= CEILING else None)
    if total < CEILING:
        order = sorted(range(len(source.rows)), key=lambda i: -sort_key(i))
        op.finish()
        assert check_pages(op, P, [source.where[i] for i in order], order, 0, 1) >= 1
        assert op.topNRankingStats()[0] == 1
    op.close()
    del source
    if total >= CEILING:
        topn_ranking_known_answer()


@on_gpu
@pytest.mark.parametrize("total", [BELOW, AT, OVER], ids=["below", "at", "over"])
def test_hash_builder_build_column(gpu, P, monkeypatch, total):
    """the same pages as a build side keyed by row id; below / at: the first, the odd and the last strings are probed"""
    monkeypatch.delenv("PRESTO_AMD_JOIN_MAX_OUTPUT_ROWS", raising=False)
    source = Source(P, ceiling_rows(total))
    n = len(source.rows)
    bridge = LookupSourceFactory()
    builder = HashBuilderOperator(bridge, TYPES, [2], [0])
    accumulate(builder, source, BUILD if total >= CEILING else None)
    if total < CEILING:
        builder.finish()
        probe = [0, 1, 2, 3, 4, 5, n // 2, n - 6, n - 5, n - 4, n - 3, n - 2, n - 1, n + 7]
        probe += [i for i, (l, z) in enumerate(source.rows) if l not in (0, 1, 7, L - 1, L)]       # (the row that holds the remainder)
        op = LookupJoinOperator(bridge, [abi.BIGINT], [0], [0], output_mem=abi.MEM_DEVICE, join_type=abi.JOIN_PROBE_OUTER)
        page = Page([bigint_block(probe)], len(probe), abi.MEM_DEVICE)
        torch.cuda.synchronize()
        op.addInput(page)
        assert check_pages(op, P, [source.where[i] if i < n else None for i in probe], probe, 1, 0) == 1
        op.finish()
        op.close()
    builder.close()
    bridge.destroy()
    del source
    if total >= CEILING:
        join_known_answer()


# ---- StreamingAggregation: the carried run's key in front of the keys of the runs a page closes ------------------------------------------------
STREAM_AGGS = [(abi.AGG_COUNT_STAR, -1, None), (abi.AGG_MIN, 1, abi.BIGINT)]


def streaming_known_answer():
    op = StreamingAggregationOperator([abi.VARCHAR, abi.BIGINT], [0], STREAM_AGGS)
    got = host_rows(op, [Page([Block.varchar([b"a", b"a"]), Block.bigint([1, 2])]), Page([Block.varchar([b"a", None, b"", b"cc", b"cc"]), Block.bigint([3, 4, 5, 6, 7])])])
    assert got == [(b"a", 3, 1), (None, 1, 4), (b"", 1, 5), (b"cc", 2, 6)]


@on_gpu
@pytest.mark.parametrize("total", [BELOW, AT, OVER], ids=["below", "at", "over"])
def test_streaming_aggregation_carried_key(gpu, P, total):
    """A page of one L-byte key leaves its run open; the next page -- one block, under 2^31 bytes -- starts another key and holds a run per
    row, so it closes the carried run and all its rows but the last: the output key column is the carried key AND those rows' keys,
    `total` bytes.  Refused by the addInput that would build it."""
    rows = ceiling_rows(total - L) + [(3, False)]
    n = len(rows)
    first = Page([varchar_block(P, 5, [(L, False)]), bigint_block([-1])], 1, abi.MEM_DEVICE)
    second = Page([varchar_block(P, 0, rows), bigint_block(list(range(n)))], n, abi.MEM_DEVICE)
    src = where(0, rows)
    assert sum(l for l, _ in rows) < CEILING and L + sum(l for l, _ in rows[:-1]) == total
    torch.cuda.synchronize()
    op = StreamingAggregationOperator([abi.VARCHAR, abi.BIGINT], [0], STREAM_AGGS, output_mem=abi.MEM_DEVICE)
    op.addInput(first)
    assert op.getOutput() is None
    if total >= CEILING:
        refused(lambda: op.addInput(second), RUN_KEYS)
    else:
        op.addInput(second)
        assert check_pages(op, P, [(5, L)] + src[:-1], [-1] + list(range(n - 1)), 0, 2) == 1
        op.finish()
        assert check_pages(op, P, src[-1:], [n - 1], 0, 2) == 1
    op.close()
    if total >= CEILING:
        streaming_known_answer()


# ---- the interner's decode: the VARCHAR key column of a fused aggregation ---------------------------------------------------------------------
def aggregation_known_answer():
    op = HashAggregationOperator([abi.VARCHAR, abi.BIGINT], [0], [(abi.AGG_COUNT_STAR, -1, None), (abi.AGG_MIN, 1, abi.BIGINT)])
    got = host_rows(op, [Page([Block.varchar([b"a" * 40, None, b"b" * 40, b"a" * 40, b""]), Block.bigint([1, 2, 3, 4, 5])])])
    assert sorted(got, key=lambda r: r[2]) == [(b"a" * 40, 2, 1), (None, 1, 2), (b"b" * 40, 1, 3), (b"", 1, 5)]


@on_gpu
@pytest.mark.parametrize("total", [CEILING - L + 8, AT, OVER], ids=["below", "at", "over"])
def test_interner_decode(gpu, P, total):
    """pairwise different keys (an undeclared VARCHAR: interned) whose bytes hold the total, count(*) and min(row id): the row id says
    which input row a group is, so every group's string is compared with that row's, and the ids must be every row exactly once.
    (`over` alone does not tell a 64-bit total from a sign check of the 32-bit one; test_interner_decode_wrapped does.)"""
    fulls, rest = divmod(total, L)
    odd = {0: [(0, False), (0, True)], 8: [(0, False), (1, False), (7, False), (0, True)], L - 1: [(0, False), (L - 1, False), (0, True)]}[rest]
    rows = odd[:1] + [(L, False)] * (fulls // 2) + odd[1:-1] + [(L, False)] * (fulls - fulls // 2) + odd[-1:]
    source = Source(P, rows)
    assert source.total == total
    op = HashAggregationOperator([abi.VARCHAR, abi.BIGINT], [0], [(abi.AGG_COUNT_STAR, -1, None), (abi.AGG_MIN, 1, abi.BIGINT)],
                                 expected_groups=len(rows), output_mem=abi.MEM_DEVICE)
    for page in source.pages:
        op.addInput(Page([page.blocks[0], page.blocks[2]], page.position_count, abi.MEM_DEVICE))
    op.finish()
    if total >= CEILING:
        refused(op.getOutput, INTERNER)
    else:
        page = op.getOutput()
        check(lib().pa_device_synchronize())
        assert page.position_count == len(rows)
        counts, _ = column_tensors(page, 1)
        ids, _ = column_tensors(page, 2)
        assert bool((counts == 1).all())
        order = ids.tolist()
        assert sorted(order) == list(range(len(rows)))
        check_varchar(*column_tensors(page, 0), [source.where[i] for i in order], P)
        assert op.getOutput() is None
    op.close()
    del source
    if total >= CEILING:
        aggregation_known_answer()


@on_gpu
def test_interner_decode_wrapped(gpu, P):
    """65537 pairwise different L-byte keys, 2^32 + L bytes: the 32-bit total of their lengths is L, which a sign check passes.  Three
    pages over the pattern, each one byte further along than the one before, so that no two keys are the same window."""
    op = HashAggregationOperator([abi.VARCHAR, abi.BIGINT], [0], [(abi.AGG_COUNT_STAR, -1, None), (abi.AGG_MIN, 1, abi.BIGINT)],
                                 expected_groups=65537, output_mem=abi.MEM_DEVICE)
    at = 0
    for base, n in ((0, 32767), (1, 32767), (2, 3)):
        page = Page([varchar_block(P, base, [(L, False)] * n), bigint_block(list(range(at, at + n)))], n, abi.MEM_DEVICE)
        torch.cuda.synchronize()
        op.addInput(page)
        at += n
    assert at * L == WRAPPED
    op.finish()
    refused(op.getOutput, INTERNER)
    op.close()
    aggregation_known_answer()


# ---- the exchange on one rank ------------------------------------------------------------------------------------------------------------------
def exchange_known_answer(comm):
    ex = ExchangeOperator(comm, [abi.VARCHAR, abi.BIGINT], [1], output_mem=abi.MEM_HOST)
    ex.addInput(Page([Block.varchar([b"a", None, b"ccc", b"", b"dd"]), Block.bigint([1, 2, 3, 4, 5])]))
    ex.finish()
    out = ex.getOutput()
    assert out.to_rows() == [(b"a", 1), (None, 2), (b"ccc", 3), (b"", 4), (b"dd", 5)]
    ex.close()


@on_gpu
def test_exchange_rle_page_is_refused_at_the_sink(gpu, P):
    comm = Comm.single()
    try:
        ex = ExchangeOperator(comm, [abi.VARCHAR, abi.BIGINT], [1])
        n = 32768
        page = Page([Block(abi.VARCHAR, abi.RLE, n, dictionary=varchar_block(P, 0, [(L, False)])), bigint_block(list(range(n)))], n, abi.MEM_DEVICE)
        torch.cuda.synchronize()
        refused(lambda: ex.addInput(page), STAGER)
        ex.close()
        exchange_known_answer(comm)
    finally:
        comm.destroy()


@on_gpu
def test_exchange_delivers_over_the_ceiling_to_one_rank(gpu, P):
    """4 pages of under 2 GiB each whose strings sum to 2^31 bytes for the one destination: every page is taken by the sink, and the
    source's getOutput -- the call that performs the collective and would build the one page -- refuses"""
    comm = Comm.single()
    try:
        source = Source(P, ceiling_rows(OVER))
        ex = ExchangeOperator(comm, [abi.VARCHAR, abi.BIGINT], [1])
        for page in source.pages:
            ex.addInput(Page([page.blocks[0], page.blocks[2]], page.position_count, abi.MEM_DEVICE))
        ex.finish()
        refused(ex.getOutput, DELIVERED)
        ex.close()
        del source
        exchange_known_answer(comm)
    finally:
        comm.destroy()


# ---- the dry run of the comparison helper: torch on the CPU, a few hundred bytes -----------------------------------------------------------------
def test_the_inputs_reach_the_stated_totals():
    """the row lists of the below / at / over legs, in the helper's own arithmetic: the offsets of the exact legs fit int32 and end at the
    stated total"""
    assert CEILING - 2 * L < BELOW < AT == 32767 * L + 65535 and OVER == AT + 1 == 32768 * L and WRAPPED == 65537 * L
    for total in (BELOW, AT, OVER):
        rows = ceiling_rows(total)
        ends = np.cumsum(np.asarray([l for l, _ in rows], dtype=np.int64))
        assert int(ends[-1]) == total and (total > np.iinfo(np.int32).max) == (total >= CEILING)
        assert rows[:5] == ODD and rows[-5:] == ODD and sum(1 for r in rows if r == (0, True)) == 3
        assert [p for p in where(0, rows) if p is not None][-1] == (total - (L - 1), L - 1)
    for total in (CEILING - L + 8, AT, OVER, WRAPPED):
        keys = big_keys(total)
        lengths = dict(zip(SMALL_KEYS, (l for l, _ in SMALL)))
        assert sum(lengths.get(k, 0) for k in keys) == total
    for fulls, fives, total in ((32767, 13106, AT - 5), (32767, 13107, AT)):
        ids = dictionary_ids(fulls, fives)
        assert ids.count(0) == fulls and ids.count(2) == fives and fulls * L + 5 * fives == total and CEILING - 2 * L < total


def test_comparison_helper_dry_run():
    """check_varchar on a 600-byte pattern with 64-byte chunks: it passes the right column, and catches one wrong byte, one wrong offset,
    one wrong NULL flag and a missing flag array"""
    pat = pattern(0, 600, "cpu")
    rows = [(0, False), (1, False), (7, False), (63, False), (0, True), (64, False), (64, False), (0, False), (130, False), (0, True), (5, False)]
    src = where(11, rows)
    order = [8, 0, 4, 5, 5, 10, 3, 9, 1, 6, 2, 7, 8]              # a gather with repeats
    expected = [src[i] for i in order]
    lengths = [0 if e is None else e[1] for e in expected]
    offsets = torch.tensor(np.concatenate([[0], np.cumsum(lengths)]), dtype=torch.int32)
    values = torch.cat([pat[e[0]:e[0] + e[1]] for e in expected if e is not None])
    nulls = torch.tensor([1 if e is None else 0 for e in expected], dtype=torch.uint8)
    assert check_varchar(offsets, values, nulls, expected, pat, chunk=64) == sum(lengths) == 528
    assert check_varchar(offsets, values, nulls, expected, pat, chunk=1 << 20) == 528
    for at in (0, 63, 64, 300, 527):                                  # the first and last byte of a chunk, and of the column
        wrong = values.clone()
        wrong[at] = wrong[at] ^ 1
        with pytest.raises(AssertionError, match="byte %d " % at):
            check_varchar(offsets, wrong, nulls, expected, pat, chunk=64)
    shifted = offsets.clone()
    shifted[6] += 1                                                   # one offset off by one: the bytes alone would still match
    with pytest.raises(AssertionError, match="offset 6 "):
        check_varchar(shifted, values, nulls, expected, pat, chunk=64)
    flags = nulls.clone()
    flags[1] = 1                                                      # an empty string is not a NULL
    with pytest.raises(AssertionError, match="NULL flag of row 1 "):
        check_varchar(offsets, values, flags, expected, pat, chunk=64)
    with pytest.raises(AssertionError, match="no flags"):
        check_varchar(offsets, values, None, expected, pat, chunk=64)
    with pytest.raises(AssertionError):                               # a row too few
        check_varchar(offsets[:-1], values, nulls[:-1], expected, pat, chunk=64)
