"""GPU checks of WindowOperator (the ranking functions) against a restatement of its contract in this file (include/presto_amd.h: rows
sorted by [partition channels ASC_NULLS_LAST] + [sort channels] under SimplePageWithPositionComparator with ties in arrival order;
partitions and peer groups cut where a sorted row IS DISTINCT FROM the one before it; row_number / rank / dense_rank / percent_rank /
cume_dist / ntile from a row's place, its partition's size and its peer group): the reference's own known answers (TestWindowOperator),
all six functions in one operator, workgroup boundaries of the function pass, independence of page cuts / memory spaces / encodings, the
NULL / NaN / -0.0 edges under all four sort orders, bad ntile bucket counts, the state machine, cross-checks against operators that
exist, seeded fuzz, the C++ mirror.  Every comparison is exact: values, NULLs, order, the raw bits of the DOUBLE results.  The oracle has
no such operator: the expected rows come from `model` (rows as Python values) and `np_model` (numeric inputs) below."""
import ctypes as C
import functools
import math
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from presto_amd import abi
from presto_amd._lib import lib
from presto_amd.operators import OrderByOperator, RowNumberOperator, TopNRankingOperator, WindowOperator, download_page, to_pages, upload_page
from presto_amd.page import Block, Page

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROW_NUMBER, RANK, DENSE_RANK, PERCENT_RANK, CUME_DIST, NTILE = range(6)
ASC_NULLS_FIRST, ASC_NULLS_LAST, DESC_NULLS_FIRST, DESC_NULLS_LAST = 0, 1, 2, 3
NAN = float("nan")
# rows of one workgroup of the function pass, as the kernel header states it
BLOCK = int(re.search(r"kWindowRowsPerBlock\s*=\s*(\d+)", open(os.path.join(ROOT, "presto_amd", "csrc", "window_kernels.hpp")).read()).group(1))


# ---- the contract, restated --------------------------------------------------------------------------------------------------------
def canon(t, v):
    """IS NOT DISTINCT FROM: NULL is one value, every NaN is one value, -0.0 is +0.0, BOOLEAN zero / non-zero, VARCHAR by bytes."""
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


def double_image(v):
    """Double.compare as an integer order: -inf < ... < -0.0 < +0.0 < ... < +inf < NaN, every NaN the same."""
    if math.isnan(v):
        return 1 << 65
    bits = struct.unpack("<Q", struct.pack("<d", v))[0]
    return (bits ^ 0xFFFFFFFFFFFFFFFF) if bits >> 63 else (bits | (1 << 63))


def order_value(t, v):
    if t == abi.DOUBLE:
        return double_image(float(v))
    if t == abi.REAL:
        return double_image(float(np.float32(v)))      # Float.compare = Double.compare of the widened values
    if t == abi.BOOLEAN:
        return 1 if v != 0 else 0
    if t == abi.VARCHAR:
        return v.encode("utf-8") if isinstance(v, str) else bytes(v)   # bytes compare unsigned, a proper prefix first
    return int(v)


def comparator(sort_types, orders):
    """SimplePageWithPositionComparator over tuples of the sort channels' values."""
    def compare(a, b):
        for t, order, x, y in zip(sort_types, orders, a, b):
            if x is None or y is None:
                if x is None and y is None:
                    continue
                nulls_first = order in (ASC_NULLS_FIRST, DESC_NULLS_FIRST)
                return -1 if (x is None) == nulls_first else 1
            kx, ky = order_value(t, x), order_value(t, y)
            if kx != ky:
                r = -1 if kx < ky else 1
                return -r if order >= 2 else r
        return 0
    return compare


def ntile_bucket(i, size, buckets):
    """NTileFunction.bucket"""
    if size < buckets:
        return i
    r, q = size % buckets, size // buckets
    return i // (q + 1) if i < (q + 1) * r else (i - r) // q


class BadBuckets(Exception):
    pass


def functions_of(functions):
    return [(f, []) if isinstance(f, int) else f for f in functions]


def model(types, rows, partition, sort, orders, functions):
    """-> [(input position, [one value per function])] in output order; DOUBLE results as Python floats (one IEEE division)."""
    channels = list(partition) + list(sort)
    compare = comparator([types[c] for c in channels], [ASC_NULLS_LAST] * len(partition) + list(orders))
    key = functools.cmp_to_key(lambda i, j: compare([rows[i][c] for c in channels], [rows[j][c] for c in channels]))
    ordered = sorted(range(len(rows)), key=key)             # stable: ties in arrival order

    def distinct(i, j, over):
        return any(canon(types[c], rows[i][c]) != canon(types[c], rows[j][c]) for c in over)

    partitions = []
    for at, i in enumerate(ordered):
        if at == 0 or distinct(ordered[at - 1], i, partition):
            partitions.append([])
        partitions[-1].append(i)
    out = []
    for members in partitions:
        size = len(members)
        starts = [at for at, i in enumerate(members) if at == 0 or distinct(members[at - 1], i, sort)]
        ends = starts[1:] + [size]
        d = -1
        for at, i in enumerate(members):
            if d + 1 < len(starts) and starts[d + 1] == at:
                d += 1
            ps, pe = starts[d], ends[d]
            values = []
            for f, args in functions_of(functions):
                if f == ROW_NUMBER:
                    values.append(at + 1)
                elif f == RANK:
                    values.append(ps + 1)
                elif f == DENSE_RANK:
                    values.append(d + 1)
                elif f == PERCENT_RANK:
                    values.append(0.0 if size == 1 else float(ps) / float(size - 1))
                elif f == CUME_DIST:
                    values.append(float(pe) / float(size))
                else:
                    buckets = rows[i][args[0]]
                    if buckets is not None and buckets <= 0:
                        raise BadBuckets()
                    values.append(None if buckets is None else ntile_bucket(at, size, int(buckets)) + 1)
            out.append((i, values))
    return out


def np_model(parts, keys, functions, buckets=None):
    """The same for numeric columns without NULL / NaN / -0.0, every order ascending: the partition columns, the sort key columns and
    the ntile bucket counts (> 0) by input row -> (input positions in output order, one array per function)."""
    total = len((parts + keys + [buckets])[0])
    order = np.lexsort(tuple([np.arange(total)] + [k for k in reversed(keys)] + [p for p in reversed(parts)]))
    at = np.arange(total)
    head = np.zeros(total, bool)
    head[0] = True
    for p in parts:
        ps = p[order]
        head[1:] |= ps[1:] != ps[:-1]
    peer_head = head.copy()
    for k in keys:
        ks = k[order]
        peer_head[1:] |= ks[1:] != ks[:-1]
    first = np.maximum.accumulate(np.where(head, at, 0))
    part_id = np.cumsum(head) - 1
    size = np.bincount(part_id)[part_id]
    place = at - first
    peer_id = np.cumsum(peer_head) - 1
    ps = np.maximum.accumulate(np.where(peer_head, at, 0)) - first
    pe = ps + np.bincount(peer_id)[peer_id]
    out = []
    for f, _ in functions_of(functions):
        if f == ROW_NUMBER:
            out.append(place + 1)
        elif f == RANK:
            out.append(ps + 1)
        elif f == DENSE_RANK:
            out.append(peer_id - peer_id[first] + 1)
        elif f == PERCENT_RANK:
            out.append(np.where(size == 1, 0.0, ps.astype(np.float64) / np.maximum(size - 1, 1).astype(np.float64)))
        elif f == CUME_DIST:
            out.append(pe.astype(np.float64) / size.astype(np.float64))
        else:
            b = buckets[order].astype(np.int64)
            r, q = size % b, size // b
            out.append(np.where(size < b, place, np.where(place < (q + 1) * r, place // (q + 1), (place - r) // np.maximum(q, 1))) + 1)
    return order, out


# ---- driving the operator ------------------------------------------------------------------------------------------------------------
def block(t, values):
    """Host block of `values` (None = NULL)."""
    if t == abi.VARCHAR:
        return Block.varchar(values)
    nulls = [v is None for v in values]
    zero = 0.0 if t in (abi.DOUBLE, abi.REAL) else 0
    return Block.flat(t, [zero if v is None else v for v in values], nulls if any(nulls) else None)


def split(rows, sizes):
    """rows cut into chunks of `sizes` (0 = an empty page), the rest as a last chunk"""
    out, at = [], 0
    for s in sizes:
        out.append(rows[at:at + s])
        at += s
    if at < len(rows):
        out.append(rows[at:])
    return out


def drain(op):
    """finish, then every output page as host pages; checks the state machine on the way."""
    assert op.needsInput() and not op.isFinished() and op.getOutput() is None      # nothing comes out before finish
    op.finish()
    assert not op.needsInput()
    pages = []
    for _ in range(1 << 16):
        p = op.getOutput()
        if p is None:
            break
        pages.append(download_page(p) if p.mem == abi.MEM_DEVICE else p)
    assert op.isFinished() and op.getOutput() is None
    return pages


def bits(v):
    return struct.unpack("<Q", struct.pack("<d", v))[0]


def same_value(t, got, want):
    """Output channels are flat copies: the very value (a NaN is a NaN; -0.0 stays -0.0; a BOOLEAN byte stays non-zero)."""
    if got is None or want is None:
        return got is None and want is None
    if t in (abi.DOUBLE, abi.REAL):
        g, w = float(got), float(np.float32(want)) if t == abi.REAL else float(want)
        return (math.isnan(g) and math.isnan(w)) or (g == w and math.copysign(1, g) == math.copysign(1, w))
    if t == abi.BOOLEAN:
        return (got != 0) == (want != 0)
    if t == abi.VARCHAR:
        return bytes(got) == (want.encode("utf-8") if isinstance(want, str) else bytes(want))
    return int(got) == int(want)


def same_result(got, want):
    """a function's value: NULL, an int, or a DOUBLE compared by its bits"""
    if got is None or want is None:
        return got is None and want is None
    if isinstance(want, float):
        return isinstance(got, float) and bits(got) == bits(want)
    return not isinstance(got, float) and int(got) == want


def feed(op, types, rows, sizes=None, device_input=False):
    """rows as pages of (types..., BIGINT row index) cut by `sizes`"""
    at = 0
    for chunk in split(rows, sizes or [len(rows)]):
        m = len(chunk)
        page = Page([block(t, [r[c] for r in chunk]) for c, t in enumerate(types)] + [Block.bigint(list(range(at, at + m)))], m)
        assert op.needsInput()
        op.addInput(upload_page(page) if device_input else page)
        at += m


def run_rows(types, rows, partition, sort, orders, functions, sizes=None, output_mem=abi.MEM_HOST, device_input=False, output_channels=None):
    """rows (tuples over `types`) through a WindowOperator over (types..., BIGINT row index) pages cut by `sizes`; the concatenated output
    is compared with the restatement: which row stands where, every output value, every function value.  Returns the output rows."""
    nt = len(types)
    out_ch = list(range(nt + 1)) if output_channels is None else list(output_channels)
    assert nt in out_ch                                   # the index column identifies the rows
    op = WindowOperator(list(types) + [abi.BIGINT], out_ch, functions, partition, sort, orders, output_mem=output_mem)
    feed(op, types, rows, sizes, device_input)
    want = model(types, rows, partition, sort, orders, functions)
    pages = drain(op)
    op.close()
    got = [r for p in pages for r in p.to_rows()]
    if not rows:
        assert pages == []                                # an operator that received no rows produces no page
    assert len(got) == len(want)
    at_index = out_ch.index(nt)
    for g, (i, values) in zip(got, want):
        assert len(g) == len(out_ch) + len(values)
        assert g[at_index] == i, (g, i, values)
        for c, v in zip(out_ch, g):
            if c < nt:
                assert same_value(types[c], v, rows[i][c]), (i, c, v, rows[i][c])
        for v, w in zip(g[len(out_ch):], values):
            assert same_result(v, w), (g, i, values)
    return got


def run_numpy(columns, types, partition, sort, functions, sizes=None, device_input=True, output_mem=abi.MEM_DEVICE, orders=None):
    """numpy columns (+ a BIGINT input-position column behind them) -> (positions in output order, [one array per function])."""
    total = len(columns[0])
    op = WindowOperator(list(types) + [abi.BIGINT], [len(types)], functions, partition, sort, orders or [ASC_NULLS_LAST] * len(sort), output_mem=output_mem)
    at = 0
    sizes = list(sizes or [total])
    while at < total:
        m = min(sizes.pop(0) if sizes else total - at, total - at)
        page = Page([Block.flat(t, c[at:at + m]) for t, c in zip(types, columns)] + [Block.bigint(np.arange(at, at + m, dtype=np.int64))], m)
        op.addInput(upload_page(page) if device_input else page)
        at += m
    pages = drain(op)
    op.close()
    cols = [np.concatenate([p.blocks[c].values[:p.position_count] for p in pages]) for c in range(1 + len(functions))]
    assert all(p.blocks[c].nulls is None or not p.blocks[c].nulls.any() for p in pages for c in range(1 + len(functions)))
    return cols[0], cols[1:]


def assert_numpy(columns, types, partition, sort, functions, buckets=None, **kw):
    pos, got = run_numpy(columns, types, partition, sort, functions, **kw)
    order, want = np_model([columns[c] for c in partition], [columns[c] for c in sort], functions, buckets)
    assert np.array_equal(pos, order)
    for f, g, w in zip(functions_of(functions), got, want):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), f     # (DOUBLE results bit by bit)
    return pos, got


ALL_FUNCTIONS = [ROW_NUMBER, RANK, DENSE_RANK, PERCENT_RANK, CUME_DIST]


# ---- 1. TestWindowOperator's known answers -------------------------------------------------------------------------------------------------
def kat(types, pages, output_channels, functions, partition, sort, orders, device, output_mem):
    op = WindowOperator(types, output_channels, functions, partition, sort, orders, expected_positions=10, output_mem=output_mem)
    for rows in pages:
        page = Page([block(t, [r[c] for r in rows]) for c, t in enumerate(types)], len(rows))
        op.addInput(upload_page(page) if device else page)
    got = [r for p in drain(op) for r in p.to_rows()]
    return [tuple("NaN" if isinstance(v, float) and math.isnan(v) else v for v in r) for r in got]


MODES = [(d, m) for d in (False, True) for m in (abi.MEM_HOST, abi.MEM_DEVICE)]
PEER_PAGES = [[(1.0, 1.0), (1.0, 0.0), (1.0, NAN), (1.0, None), (2.0, 2.0), (2.0, NAN), (NAN, NAN), (NAN, NAN), (None, None), (None, 1.0), (None, None)],
              [(1.0, NAN), (1.0, None), (2.0, 2.0), (2.0, None), (NAN, 3.0), (NAN, None), (None, 2.0), (None, None)]]
PEER_ANSWER = [(1.0, 0.0, 1), (1.0, 1.0, 2), (1.0, "NaN", 3), (1.0, "NaN", 3), (1.0, None, 5), (1.0, None, 5), (2.0, 2.0, 1), (2.0, 2.0, 1),
               (2.0, "NaN", 3), (2.0, None, 4), ("NaN", 3.0, 1), ("NaN", "NaN", 2), ("NaN", "NaN", 2), ("NaN", None, 4), (None, 1.0, 1),
               (None, 2.0, 2), (None, None, 3), (None, None, 3), (None, None, 3)]


@pytest.mark.parametrize("device,output_mem", MODES)
def test_row_number_kat(gpu, device, output_mem):
    """testRowNumber: no partition, sort 0 ASC_NULLS_LAST, output channels (1, 0)."""
    got = kat([abi.BIGINT, abi.DOUBLE], [[(2, 0.3), (4, 0.2), (6, 0.1)], [(-1, -0.1), (5, 0.4)]], [1, 0], [ROW_NUMBER], [], [0], [ASC_NULLS_LAST], device, output_mem)
    assert got == [(-0.1, -1, 1), (0.3, 2, 2), (0.2, 4, 3), (0.4, 5, 4), (0.1, 6, 5)]


@pytest.mark.parametrize("device,output_mem", MODES)
def test_row_number_partition_kat(gpu, device, output_mem):
    """testRowNumberPartition: partition by a VARCHAR, sort 1 ASC_NULLS_LAST, every channel out."""
    pages = [[("b", -1, -0.1, True), ("a", 2, 0.3, False), ("a", 4, 0.2, True)], [("b", 5, 0.4, False), ("a", 6, 0.1, True)]]
    got = kat([abi.VARCHAR, abi.BIGINT, abi.DOUBLE, abi.BOOLEAN], pages, [0, 1, 2, 3], [ROW_NUMBER], [0], [1], [ASC_NULLS_LAST], device, output_mem)
    assert got == [(b"a", 2, 0.3, False, 1), (b"a", 4, 0.2, True, 2), (b"a", 6, 0.1, True, 3), (b"b", -1, -0.1, True, 1), (b"b", 5, 0.4, False, 2)]


@pytest.mark.parametrize("device,output_mem", MODES)
def test_row_number_arbitrary_kat(gpu, device, output_mem):
    """testRowNumberArbitrary: no partition, no order -- arrival order."""
    got = kat([abi.BIGINT], [[(1,), (3,), (5,), (7,)], [(2,), (4,), (6,), (8,)]], [0], [ROW_NUMBER], [], [], [], device, output_mem)
    assert got == [(1, 1), (3, 2), (5, 3), (7, 4), (2, 5), (4, 6), (6, 7), (8, 8)]


@pytest.mark.parametrize("device,output_mem", MODES)
def test_distinct_partition_and_peers_kat(gpu, device, output_mem):
    """testDistinctPartitionAndPeers: RANK over NaN / NULL partitions and peers."""
    got = kat([abi.DOUBLE, abi.DOUBLE], PEER_PAGES, [0, 1], [RANK], [0], [1], [ASC_NULLS_LAST], device, output_mem)
    assert got == PEER_ANSWER


def test_the_model_reproduces_the_known_answers():
    """(the restatement itself, against the reference answers: no GPU work)"""
    rows = [r for p in PEER_PAGES for r in p]
    got = [tuple("NaN" if isinstance(v, float) and math.isnan(v) else v for v in rows[i]) + (values[0],)
           for i, values in model([abi.DOUBLE, abi.DOUBLE], rows, [0], [1], [ASC_NULLS_LAST], [RANK])]
    assert got == PEER_ANSWER
    rows = [(2, 0.3), (4, 0.2), (6, 0.1), (-1, -0.1), (5, 0.4)]
    assert [(rows[i][0], v[0]) for i, v in model([abi.BIGINT, abi.DOUBLE], rows, [], [0], [ASC_NULLS_LAST], [ROW_NUMBER])] == [(-1, 1), (2, 2), (4, 3), (5, 4), (6, 5)]
    assert [ntile_bucket(i, 7, 3) for i in range(7)] == [0, 0, 0, 1, 1, 2, 2] and [ntile_bucket(i, 2, 5) for i in range(2)] == [0, 1]
    # the numpy restatement agrees with the row-wise one
    rng = np.random.default_rng(5)
    part, key, buckets = rng.integers(0, 7, 300), rng.integers(0, 5, 300), rng.integers(1, 9, 300)
    functions = ALL_FUNCTIONS + [(NTILE, [2])]
    order, cols = np_model([part], [key], functions, buckets)
    want = model([abi.BIGINT] * 3, list(zip(part.tolist(), key.tolist(), buckets.tolist())), [0], [1], [ASC_NULLS_LAST], functions)
    assert order.tolist() == [i for i, _ in want]
    for k in range(len(functions)):
        assert all(same_result(g, w[k]) for g, (_, w) in zip(cols[k].tolist(), want))


# ---- 2. all six functions in one operator -----------------------------------------------------------------------------------------------------
SIX_TYPES = [abi.BIGINT, abi.DOUBLE, abi.BIGINT, abi.INTEGER]      # partition, sort key, ntile buckets (BIGINT), ntile buckets (INTEGER)
SIX_ROWS = ([(1, 5.0, 3, 1)]                                                                     # a partition of one row
            + [(2, float(k), b, 1) for k, b in zip([1, 1, 2, 2, 2, 3, 4], [3, 3, 3, 3, 3, 3, 3])]   # ties; N = 7, N % 3 != 0
            + [(3, float(k), 5, 4) for k in (2, 1)]                                              # N = 2 < 5 buckets
            + [(4, float(k % 3), b, 2) for k, b in enumerate([1, 2, 3, None, 4, 5, 6, 7, None, 100, 2])]   # a NULL bucket, per-row counts
            + [(None, 1.5, 1, 1), (None, 1.5, 1, 1), (None, None, 1, 1)])                        # the NULL partition; buckets = 1


def test_all_six_functions_in_one_operator(gpu):
    """...in a non-enum order, the same function twice, ntile over a BIGINT and over an INTEGER channel."""
    functions = [CUME_DIST, (NTILE, [2]), ROW_NUMBER, PERCENT_RANK, DENSE_RANK, RANK, (NTILE, [3]), RANK, CUME_DIST]
    got = run_rows(SIX_TYPES, SIX_ROWS, [0], [1], [ASC_NULLS_LAST], functions)
    nt = len(SIX_TYPES) + 1
    assert got[0][nt:] == (1.0, 1, 1, 0.0, 1, 1, 1, 1, 1.0)                  # the partition of one row
    assert [g[nt + 1] for g in got[1:8]] == [1, 1, 1, 2, 2, 3, 3]            # ntile(3) over 7 rows
    assert [g[nt + 5] for g in got[1:8]] == [1, 1, 3, 3, 3, 6, 7]            # rank with ties
    assert [g[nt + 4] for g in got[1:8]] == [1, 1, 2, 2, 2, 3, 4]            # dense_rank
    assert [g[nt + 1] for g in got[8:10]] == [1, 2]                          # N < buckets
    assert sum(g[nt + 1] is None for g in got) == 2                          # the NULL buckets
    for device, output_mem in MODES:
        run_rows(SIX_TYPES, SIX_ROWS, [0], [1], [DESC_NULLS_FIRST], functions, sizes=[5, 0, 9], device_input=device, output_mem=output_mem)


# ---- 3. workgroup boundaries ---------------------------------------------------------------------------------------------------------------------
def boundary_columns(n, layout):
    at = np.arange(n, dtype=np.int64)
    if layout == "one_partition":
        return np.zeros(n, np.int64), at.copy()
    if layout == "all_peers":
        return np.zeros(n, np.int64), np.full(n, 7, np.int64)
    if layout == "own_partitions":
        return at.copy(), np.zeros(n, np.int64)
    # a partition [BLOCK / 2, 2.5 BLOCK) and, inside it, a peer group [BLOCK / 2 + 7, 2.5 BLOCK - 5): each starts in one block and ends two later
    lo = BLOCK // 2
    return np.digitize(at, [lo, lo + 2 * BLOCK]).astype(np.int64), np.digitize(at, [lo + 7, lo + 2 * BLOCK - 5]).astype(np.int64)


@pytest.mark.parametrize("layout", ["one_partition", "all_peers", "own_partitions", "spanning"])
@pytest.mark.parametrize("n", [1, BLOCK - 1, BLOCK, BLOCK + 1, 4 * BLOCK + 3])
def test_workgroup_boundaries(gpu, n, layout):
    part, key = boundary_columns(n, layout)
    buckets = (np.arange(n, dtype=np.int64) % 5) + 1
    shuffle = np.random.default_rng(n).permutation(n)          # the sort has work to do; sorted place = the value
    columns = [part[shuffle], key[shuffle], buckets[shuffle]]
    assert_numpy(columns, [abi.BIGINT] * 3, [0], [1], ALL_FUNCTIONS + [(NTILE, [2])], columns[2])


# ---- 4. page cuts, memory spaces, encodings -------------------------------------------------------------------------------------------------------
def test_page_cuts_and_memory_spaces_do_not_change_the_output(gpu):
    rng = np.random.default_rng(11)
    rows = [(int(rng.integers(0, 6)), "s%d" % int(rng.integers(0, 4)), float(rng.integers(0, 5)) / 2, int(rng.integers(1, 6))) for _ in range(60)]
    types = [abi.BIGINT, abi.VARCHAR, abi.DOUBLE, abi.BIGINT]
    functions = ALL_FUNCTIONS + [(NTILE, [3])]
    outputs = []
    for sizes in ([60], [7, 0, 40], [1] * 60):
        for device, output_mem in MODES:
            outputs.append(run_rows(types, rows, [0], [1, 2], [DESC_NULLS_LAST, ASC_NULLS_FIRST], functions, sizes=sizes, device_input=device, output_mem=output_mem))
    assert all(o == outputs[0] for o in outputs)


def test_dictionary_and_rle_blocks(gpu):
    """dictionary and RLE blocks in partition, sort, argument and output channels, from host and from device pages"""
    part = Block.dictionary_block(Block.flat(abi.BIGINT, [5, 4, 0], [0, 0, 1]), [0, 1, 2, 2, 0, 1, 0, 0])
    key = Block.dictionary_block(Block.varchar(["x", "yy", None]), [1, 1, 2, 0, 2, 0, 0, 1])
    rle = Block.rle(Block.double([2.5]), 8)
    buckets = Block.rle(Block.bigint([2]), 8)
    types = [abi.BIGINT, abi.VARCHAR, abi.DOUBLE, abi.BIGINT]
    rows = list(zip(part.to_pylist(), key.to_pylist(), rle.to_pylist(), buckets.to_pylist()))
    functions = ALL_FUNCTIONS + [(NTILE, [3])]
    for partition, sort in (([0], [1]), ([1], [0]), ([2], [1, 0]), ([0], [2])):
        for device in (False, True):
            op = WindowOperator(types + [abi.BIGINT], [0, 1, 2, 4], functions, partition, sort, [ASC_NULLS_FIRST] * len(sort))
            all_rows = []
            for rep in range(3):
                page = Page([part, key, rle, buckets, Block.bigint(list(range(8 * rep, 8 * rep + 8)))], 8)
                op.addInput(upload_page(page) if device else page)
                all_rows += rows
            got = [r for p in drain(op) for r in p.to_rows()]
            want = model(types, all_rows, partition, sort, [ASC_NULLS_FIRST] * len(sort), functions)
            assert [g[3] for g in got] == [i for i, _ in want]
            for g, (i, values) in zip(got, want):
                assert all(same_value(t, v, w) for t, v, w in zip(types[:3], g, all_rows[i]))
                assert all(same_result(v, w) for v, w in zip(g[4:], values))


# ---- 5. edges ---------------------------------------------------------------------------------------------------------------------------------------
EDGE_VALUES = [-0.0, 0.0, NAN, None, 1.5, -0.0, float("-inf"), NAN, 0.0, None, float("inf"), -2.0]


@pytest.mark.parametrize("t", [abi.DOUBLE, abi.REAL])
@pytest.mark.parametrize("order", [ASC_NULLS_FIRST, ASC_NULLS_LAST, DESC_NULLS_FIRST, DESC_NULLS_LAST])
def test_zeros_nan_and_null_as_partition_and_sort_values(gpu, t, order):
    rows = [(a, b, k) for k, (a, b) in enumerate((a, b) for a in EDGE_VALUES[:8] for b in EDGE_VALUES)]
    got = run_rows([t, t, abi.BIGINT], rows, [0], [1], [order], ALL_FUNCTIONS, sizes=[31, 40])
    # both zeros land in one partition and, inside it, in one peer group
    zero_partition = [g for g in got if g[0] is not None and g[0] == 0.0]
    assert len(zero_partition) == 3 * len(EDGE_VALUES) and [g[4] for g in zero_partition] == list(range(1, len(zero_partition) + 1))
    # ... and, as sort values of one partition, in one peer group (in the zero partition the comparator keeps the rows of -0.0 and of
    # +0.0 apart, so their peer groups are cut by adjacency there: the restatement above says how)
    peers = [g for g in got if g[0] == 1.5 and g[1] is not None and g[1] == 0.0]
    assert len(peers) == 4 and len({g[5] for g in peers}) == 1 and len({g[6] for g in peers}) == 1
    # the other way round: the edge values as the sort channel's partner, sorted as a second sort channel
    run_rows([t, t, abi.BIGINT], rows, [], [0, 1], [order, DESC_NULLS_LAST ^ (order & 1)], ALL_FUNCTIONS)


def test_varchar_partition_and_sort_channels(gpu):
    """...including the empty string, a proper prefix and a NULL; strings longer than one 8-byte chunk"""
    words = ["", "a", "ab", "abc", None, "b", "a", "", "abcdefgh", "abcdefghi", "abcdefgh", None, "ab"]
    rows = [(w, v, k % 4 + 1) for k, (w, v) in enumerate((w, v) for w in words for v in words)]
    for order in (ASC_NULLS_FIRST, DESC_NULLS_LAST):
        run_rows([abi.VARCHAR, abi.VARCHAR, abi.BIGINT], rows, [0], [1], [order], ALL_FUNCTIONS + [(NTILE, [2])], sizes=[50, 60])


def test_two_partition_channels(gpu):
    rng = np.random.default_rng(12)
    rows = [(None if rng.random() < 0.1 else int(rng.integers(0, 3)), ["x", "y", None][int(rng.integers(0, 3))], int(rng.integers(0, 4))) for _ in range(200)]
    run_rows([abi.INTEGER, abi.VARCHAR, abi.BIGINT], rows, [0, 1], [2], [DESC_NULLS_FIRST], ALL_FUNCTIONS, sizes=[64, 64])
    run_rows([abi.INTEGER, abi.VARCHAR, abi.BIGINT], rows, [1, 0], [2], [ASC_NULLS_LAST], ALL_FUNCTIONS, device_input=True, output_mem=abi.MEM_DEVICE)


def test_no_sort_channels(gpu):
    """the whole partition is one peer group: rank = dense_rank = 1, percent_rank 0.0, cume_dist 1.0; arrival order inside a partition"""
    rows = [(k % 3, k) for k in range(40)]
    got = run_rows([abi.BIGINT, abi.BIGINT], rows, [0], [], [], ALL_FUNCTIONS)
    assert all(g[4:] == (1, 1, 0.0, 1.0) for g in got)
    assert [g[1] for g in got] == [k for p in range(3) for k in range(40) if k % 3 == p]


def test_other_types(gpu):
    """short DECIMAL and BOOLEAN partition channels, a DATE sort channel"""
    rows = [(k % 3, (k * 7) % 5, k % 2) for k in range(30)]
    op = WindowOperator([abi.decimal(12, 2), abi.DATE, abi.BOOLEAN, abi.BIGINT], [3], [RANK, ROW_NUMBER], [0, 2], [1], [DESC_NULLS_LAST])
    op.addInput(Page([Block.decimal([r[0] for r in rows]), Block.date([r[1] for r in rows]), block(abi.BOOLEAN, [r[2] for r in rows]),
                      Block.bigint(list(range(30)))], 30))
    got = [r for p in drain(op) for r in p.to_rows()]
    want = model([abi.BIGINT, abi.DATE, abi.BOOLEAN], rows, [0, 2], [1], [DESC_NULLS_LAST], [RANK, ROW_NUMBER])
    assert [tuple(g) for g in got] == [(i, v[0], v[1]) for i, v in want]


# ---- 6. ntile with a bad bucket count -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [0, -1])
@pytest.mark.parametrize("t", [abi.BIGINT, abi.INTEGER])
def test_ntile_bad_bucket_count(gpu, bad, t):
    """get_output fails with INVALID_ARGUMENT, nothing is emitted, and the operator can still be closed and destroyed"""
    n = 2 * BLOCK + 5
    buckets = np.full(n, 3, np.int64)
    buckets[n - 2] = bad
    op = WindowOperator([abi.BIGINT, t], [0], [ROW_NUMBER, (NTILE, [1])], [0], [0], [ASC_NULLS_LAST])
    op.addInput(Page([Block.bigint(np.arange(n) % 7), Block.flat(t, buckets)], n))
    op.finish()
    out = abi.pa_page()
    assert lib().pa_op_get_output(op._h, C.byref(out)) == abi.ERR_INVALID_ARGUMENT
    assert b"Buckets must be greater than 0" in lib().pa_last_error()
    assert op.getOutput() is None and op.isFinished()
    op.close()
    with pytest.raises(BadBuckets):
        model([abi.BIGINT, t], [(1, bad)], [0], [0], [ASC_NULLS_LAST], [(NTILE, [1])])
    # a NULL in front of a bad count is not one
    op = WindowOperator([abi.BIGINT, t], [0], [(NTILE, [1])], [], [0], [ASC_NULLS_LAST])
    op.addInput(Page([Block.bigint([1, 2]), Block.flat(t, [bad, 2], [1, 0])], 2))
    assert [r for p in drain(op) for r in p.to_rows()] == [(1, None), (2, 2)]
    op.close()


# ---- 7. the state machine ----------------------------------------------------------------------------------------------------------------------------
def test_state_machine_and_memory_bytes(gpu):
    op = WindowOperator([abi.BIGINT, abi.VARCHAR], [0, 1], [RANK], [0], [1], [ASC_NULLS_LAST])
    assert op.needsInput() and not op.isFinished() and op.getOutput() is None
    empty = Page([Block.bigint([]), Block.varchar([])], 0)
    op.addInput(empty)                                        # empty pages are accepted
    before = op.memoryBytes()
    op.addInput(Page([Block.bigint([3, 1, 3]), Block.varchar(["b", "a", "a"])], 3))
    assert op.memoryBytes() > before and op.memoryBytes() > 0        # rows are held
    assert op.needsInput() and op.getOutput() is None and not op.isFinished()
    op.addInput(empty)
    op.finish()
    assert not op.needsInput() and not op.isFinished()
    cpage, _keep = Page([Block.bigint([1]), Block.varchar(["x"])], 1).to_c()
    assert lib().pa_op_add_input(op._h, C.byref(cpage)) == abi.ERR_ILLEGAL_STATE
    page = op.getOutput()
    assert page.to_rows() == [(1, b"a", 1), (3, b"a", 1), (3, b"b", 2)]
    assert op.memoryBytes() > 0
    assert op.isFinished() and op.getOutput() is None and not op.needsInput()
    op.finish()                                               # idempotent
    assert op.isFinished()
    op.close()
    # no rows at all: no page
    op = WindowOperator([abi.BIGINT], [0], [ROW_NUMBER], [], [], [])
    op.addInput(Page([Block.bigint([])], 0))
    assert drain(op) == []
    op.close()
    op = WindowOperator([abi.BIGINT], [0], [ROW_NUMBER], [0], [0], [ASC_NULLS_LAST])
    op.finish()
    assert op.isFinished() and op.getOutput() is None
    op.close()


# ---- 8. cross-checks against operators that exist -----------------------------------------------------------------------------------------------------
def cross_input(seed):
    rng = np.random.default_rng(seed)
    total = 60_000
    part = rng.integers(0, 1500, total).astype(np.int64)
    key = rng.integers(0, 50, total).astype(np.float64) * 0.5
    return part, key, np.arange(total, dtype=np.int64)


def columns_of(pages):
    return [np.concatenate([p.blocks[c].values[:p.position_count] for p in pages]) for c in range(len(pages[0].blocks))]


def test_the_payload_order_is_order_by(gpu):
    part, key, pos = cross_input(60)
    types = [abi.BIGINT, abi.DOUBLE, abi.BIGINT]
    page = Page([Block.bigint(part), Block.double(key), Block.bigint(pos)], len(part))
    sorted_ = columns_of(to_pages(OrderByOperator(types, [0, 1, 2], [0, 1], [ASC_NULLS_LAST, DESC_NULLS_FIRST]), [page]))
    got, _ = run_numpy([part, key], types[:2], [0], [1], [ROW_NUMBER], sizes=[25_000] * 3, orders=[DESC_NULLS_FIRST])
    assert np.array_equal(got, sorted_[2])


@pytest.mark.parametrize("ranking,function", [(abi.RANKING_ROW_NUMBER, ROW_NUMBER), (abi.RANKING_RANK, RANK)])
def test_filtered_to_n_it_is_topn_ranking(gpu, ranking, function):
    part, key, pos = cross_input(61)
    n = 5
    got_pos, (got_value,) = run_numpy([part, key], [abi.BIGINT, abi.DOUBLE], [0], [1], [function], sizes=[20_000] * 3)
    keep = got_value <= n
    op = TopNRankingOperator([abi.BIGINT, abi.DOUBLE, abi.BIGINT], [0, 2], [0], [1], [ASC_NULLS_LAST], n, ranking_type=ranking)
    op.addInput(Page([Block.bigint(part), Block.double(key), Block.bigint(pos)], len(part)))
    topn = columns_of(drain(op))
    # TopNRanking emits partitions in first-seen order, the window in key order: regroup by partition, keep the order inside
    regroup = np.argsort(topn[0], kind="stable")
    assert np.array_equal(got_pos[keep], topn[1][regroup]) and np.array_equal(got_value[keep], topn[2][regroup])


def test_without_partition_and_order_it_is_row_number(gpu):
    part, _, pos = cross_input(62)
    types = [abi.BIGINT, abi.BIGINT]
    pages = [Page([Block.bigint(part[a:a + 20_000]), Block.bigint(pos[a:a + 20_000])], 20_000) for a in (0, 20_000, 40_000)]
    numbered = columns_of(to_pages(RowNumberOperator(types, [1], []), pages))
    op = WindowOperator(types, [1], [ROW_NUMBER], [], [], [])
    for p in pages:
        op.addInput(p)
    got = columns_of(drain(op))
    assert np.array_equal(got[0], numbered[0]) and np.array_equal(got[1], numbered[1])


# ---- 9. seeded fuzz -------------------------------------------------------------------------------------------------------------------------------
FUZZ_SEEDS = int(os.environ.get("PA_FUZZ_SEEDS", "6"))


@pytest.mark.parametrize("seed", range(FUZZ_SEEDS))
def test_fuzz_window(gpu, seed):
    rng = np.random.default_rng(7000 + seed)
    total = int(rng.integers(1, 20_001))
    partitions = int(rng.choice([1, 3, 200, 5000]))
    part = rng.integers(0, partitions, total).astype(np.int64)
    part2 = rng.integers(0, 2, total).astype(np.int32)
    key = rng.integers(0, int(rng.choice([1, 3, 40])), total).astype(np.float64) / 4        # a heavy-tie sort key
    key2 = rng.integers(0, 3, total).astype(np.int64)
    buckets = rng.integers(1, int(rng.choice([2, 10, 40_000])), total).astype(np.int64)
    columns, types = [part, part2, key, key2, buckets], [abi.BIGINT, abi.INTEGER, abi.DOUBLE, abi.BIGINT, abi.BIGINT]
    partition = [[0], [0, 1], []][int(rng.integers(0, 3))]
    sort = [[2], [2, 3], []][int(rng.integers(0, 3))]
    picks = [int(f) for f in rng.permutation(6)[:int(rng.integers(1, 7))]]
    functions = [(NTILE, [4]) if f == NTILE else f for f in picks]
    sizes = [int(s) for s in rng.integers(1, max(2, total // 2), int(rng.integers(1, 6)))]
    assert_numpy(columns, types, partition, sort, functions, buckets, sizes=sizes, device_input=bool(rng.integers(0, 2)), output_mem=int(rng.integers(0, 2)))


# ---- 10. the C++ mirror -------------------------------------------------------------------------------------------------------------------------------
def test_cpp_mirror(gpu):
    """tests/cpp/test_window.cpp: the operator through the C++ host mirror's runDriver."""
    exe = os.path.join(ROOT, "tests", "cpp", "test_window")
    src = exe + ".cpp"
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-L" + os.path.join(ROOT, "presto_amd"),
                               "-lpresto_amd", "-Wl,-rpath,$ORIGIN/../../presto_amd", "-Wl,--allow-shlib-undefined", "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode == 0, r.stdout.decode()[-2000:]
    assert "window ok" in r.stdout.decode()
