"""GPU checks of RowNumberOperator against a restatement of the reference's loops in this file (RowNumberOperator.java:289-342:
getRowsWithRowNumber / getSelectedRows over GroupByHash.getGroupIds, which compares by IS NOT DISTINCT FROM): the reference's own
known-answer cases (TestRowNumberOperator), order independence inside a page and across page cuts, the NULL / NaN / -0.0 edges, every
key type, encodings and memory spaces, the cap, the state machine, growth, two cross-checks against operators that exist, seeded fuzz.
Every comparison is exact, row by row and page by page.  The oracle has no such operator: the expected numbers come from `Model` below.

Order independence: the cases under that heading are built so that a ranking by atomics in arrival order could not pass.  While the
kernels were written none of them was seen failing: the rank pass was designed without a carry between workgroups from the start."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from presto_amd import abi
from presto_amd._lib import check, lib
from presto_amd.operators import (HashAggregationOperator, MarkDistinctOperator, RowNumberOperator, RowNumberOperatorFactory,  # noqa: F401
                                  device_page_from_c, download, download_page, to_pages, upload_page)
from presto_amd.page import Block, DeviceBuffer, Page, page_from_c

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the contract, restated (RowNumberOperator.java:289-342) ---------------------------------------------------------------------
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


class Model:
    """partitionRowCount of the reference: a count per partition, carried over pages; `cap` = maxRowsPerPartition or None."""

    def __init__(self, key_types, cap=None):
        self.key_types, self.cap, self.counts = key_types, cap, {}

    def page(self, keys):
        """keys: the partition key tuple of each row of one page, in order -> [(position, row number)] of the rows that go out."""
        out = []
        for i, k in enumerate(keys):
            k = key_of(self.key_types, k)
            c = self.counts.setdefault(k, 0)      # (getGroupIds has seen the partition even when the row is dropped)
            if self.cap is not None and c >= self.cap:
                continue
            self.counts[k] = c + 1
            out.append((i, c + 1))
        return out


def block(t, values):
    """Host block of `values` (None = NULL)."""
    if t == abi.VARCHAR:
        return Block.varchar(values)
    nulls = [v is None for v in values]
    zero = 0.0 if t in (abi.DOUBLE, abi.REAL) else 0
    return Block.flat(t, [zero if v is None else v for v in values], nulls if any(nulls) else None)


def hash_block(n):
    """A $hashvalue channel: the operator never reads it, so any BIGINT values must give the same result."""
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


def raw_output(op):
    """The operator's next output page as the C struct, or None."""
    out = abi.pa_page()
    if not check(lib().pa_op_get_output(op._h, C.byref(out))):
        return None
    return out


def rn_of(out):
    """The row number column of a C output page (a device page may carry the input's dictionary / RLE blocks in front of it, which the
    Python page view does not decode): BIGINT, flat, no nulls."""
    n = out.position_count
    col = out.columns[out.channel_count - 1]
    assert col.type == abi.BIGINT and col.encoding == abi.FLAT and not col.nulls
    if out.mem == abi.MEM_DEVICE:
        return download(DeviceBuffer(col.values, 8 * n), np.int64, n)
    return np.frombuffer(C.string_at(col.values, 8 * n), np.int64).copy() if n else np.zeros(0, np.int64)


def host_page_of(op, out):
    return page_from_c(out) if out.mem == abi.MEM_HOST else download_page(device_page_from_c(out, owner=op))


def run_rows(types, rows, partition, cap=None, sizes=None, hashed=False, output_mem=abi.MEM_HOST, device_input=False, expected_positions=0,
             output_channels=None):
    """rows (tuples over `types`) through a RowNumberOperator over (types..., BIGINT row index, [$hashvalue]) pages cut by `sizes`.  Follows
    the state machine call by call and compares every output page with the restatement: which rows went out (by their index column), in
    which order, with which number, and the values of every output channel.  Returns the operator."""
    nt = len(types)
    page_types = list(types) + [abi.BIGINT] + ([abi.BIGINT] if hashed else [])
    out_ch = list(range(len(page_types))) if output_channels is None else list(output_channels)
    assert nt in out_ch                                   # the index column identifies the rows
    op = RowNumberOperator(page_types, out_ch, partition, cap, hash_channel=len(page_types) - 1 if hashed else -1, output_mem=output_mem,
                           expected_positions=expected_positions)
    key_types = [types[c] for c in partition]
    model = Model(key_types, cap)
    single_cap = cap is not None and not partition
    at = 0
    for chunk in split(rows, sizes or [len(rows)]):
        n = len(chunk)
        if single_cap and model.counts.get((), 0) >= cap:
            assert not op.needsInput() and op.isFinished()
            break
        assert op.needsInput() and not op.isFinished()
        blocks = [block(t, [r[c] for r in chunk]) for c, t in enumerate(types)] + [Block.bigint(list(range(at, at + n)))]
        blocks += [hash_block(n)] if hashed else []
        hashes = hash_block(n).to_pylist()
        page = Page(blocks, n)
        op.addInput(upload_page(page) if device_input else page)
        want = model.page([[r[c] for c in partition] for r in chunk])
        out = raw_output(op)
        if not want:
            assert out is None                           # a page that keeps no row produces no page
        else:
            assert out is not None and out.mem == output_mem
            assert out.position_count == len(want) and out.channel_count == len(out_ch) + 1
            assert rn_of(out).tolist() == [rn for _, rn in want]
            got = host_page_of(op, out).to_rows()
            for (i, rn), g in zip(want, got):
                full = list(chunk[i]) + [at + i] + ([hashes[i]] if hashed else [])
                for c, v in zip(out_ch, g[:-1]):
                    assert canon(page_types[c], v) == canon(page_types[c], full[c]), (i, c, v, full[c])
                assert g[-1] == rn
        assert raw_output(op) is None
        at += n
    count, capacity = op.rowNumberStats()
    if partition:
        assert count == len(model.counts)
        assert capacity >= 2 * count and capacity & (capacity - 1) == 0
    else:
        assert (count, capacity) == (1, 0)
    op.finish()
    assert op.isFinished() and not op.needsInput() and raw_output(op) is None
    return op


# ---- TestRowNumberOperator (core/trino-main/src/test/java/io/trino/operator/TestRowNumberOperator.java) --------------------------
KAT_TYPES = [abi.BIGINT, abi.DOUBLE]
KAT_PAGES = [[(1, 0.3), (2, 0.2), (3, 0.1), (3, 0.19)], [(1, 0.4)], [(1, 0.5), (1, 0.6), (2, 0.7), (2, 0.8), (2, 0.9)]]


def kat_pages(hashed):
    return [Page([Block.bigint([r[0] for r in rows]), Block.double([r[1] for r in rows])] + ([hash_block(len(rows))] if hashed else []), len(rows))
            for rows in KAT_PAGES]


def drive(op, pages):
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
    assert op.getOutput() is None
    assert op.isFinished()
    return out


def test_row_number_unpartitioned_kat(gpu):
    """testRowNumberUnpartitioned: output channels (1, 0), no partition channels, no cap -> 1 .. 10 over the three pages."""
    op = RowNumberOperator(KAT_TYPES, [1, 0], [], expected_positions=10)
    out = drive(op, kat_pages(False))
    assert [p.position_count for p in out] == [4, 1, 5]
    rows = [r for p in out for r in p.to_rows()]
    assert rows == [(v, k, i + 1) for i, (k, v) in enumerate(r for page in KAT_PAGES for r in page)]


@pytest.mark.parametrize("hashed", [False, True])
def test_row_number_partitioned_kat(gpu, hashed):
    """testRowNumberPartitioned: partition by channel 0, cap 10 -> all ten rows, numbered 1 .. 4 / 1 .. 4 / 1 .. 2 in arrival order."""
    types = KAT_TYPES + ([abi.BIGINT] if hashed else [])
    op = RowNumberOperator(types, [1, 0], [0], 10, hash_channel=2 if hashed else -1, expected_positions=10)
    rows = [r for p in drive(op, kat_pages(hashed)) for r in p.to_rows()]
    assert rows == [(0.3, 1, 1), (0.2, 2, 1), (0.1, 3, 1), (0.19, 3, 2), (0.4, 1, 2), (0.5, 1, 3), (0.6, 1, 4), (0.7, 2, 2), (0.8, 2, 3), (0.9, 2, 4)]
    assert op.rowNumberStats()[0] == 3


@pytest.mark.parametrize("hashed", [False, True])
def test_row_number_partitioned_limit_kat(gpu, hashed):
    """testRowNumberPartitionedLimit: cap 3 -> 8 rows, 3 / 3 / 2 per partition, every number <= 3."""
    types = KAT_TYPES + ([abi.BIGINT] if hashed else [])
    op = RowNumberOperator(types, [1, 0], [0], 3, hash_channel=2 if hashed else -1, expected_positions=10)
    out = drive(op, kat_pages(hashed))
    rows = [r for p in out for r in p.to_rows()]
    assert rows == [(0.3, 1, 1), (0.2, 2, 1), (0.1, 3, 1), (0.19, 3, 2), (0.4, 1, 2), (0.5, 1, 3), (0.7, 2, 2), (0.8, 2, 3)]
    assert [p.position_count for p in out] == [4, 1, 3]


def test_row_number_unpartitioned_limit_kat(gpu):
    """testRowNumberUnpartitionedLimit: cap 3 without partition channels -> exactly the first three rows, then finished."""
    op = RowNumberOperator(KAT_TYPES, [1, 0], [], 3, expected_positions=10)
    pages = kat_pages(False)
    assert op.needsInput() and not op.isFinished()
    op.addInput(pages[0])
    assert not op.needsInput() and not op.isFinished()          # a page is pending
    out = op.getOutput()
    assert out.to_rows() == [(0.3, 1, 1), (0.2, 2, 2), (0.1, 3, 3)]
    assert not op.needsInput() and op.isFinished()               # the cap is reached: finished without finish()
    assert lib().pa_op_add_input(op._h, C.byref(pages[1].to_c()[0])) == abi.ERR_ILLEGAL_STATE
    assert op.getOutput() is None


@pytest.mark.parametrize("t", [abi.BIGINT, abi.VARCHAR])
def test_pages_of_new_keys_only(gpu, t):
    """testMemoryReservationYield's shape: 6 000 pages of 600 rows, every key new, one expected position: every row number is 1 and the
    table grew."""
    pages, rows_per_page = 6000, 600
    if t == abi.VARCHAR:
        pages = 300             # (interning a string column per page is host-driven work: the same shape, fewer pages)
    op = RowNumberOperator([t], [0], [0], expected_positions=1)
    before = op.rowNumberStats()[1]
    assert before <= 64
    ids = np.arange(pages * rows_per_page, dtype=np.int64)
    keys = ids * 1000003 - 7
    fed = 0
    for p in range(pages):
        part = keys[fed:fed + rows_per_page]
        key = Block.bigint(part) if t == abi.BIGINT else Block.varchar(["key-%d" % i for i in part])
        op.addInput(Page([key], rows_per_page))
        out = raw_output(op)
        assert out.position_count == rows_per_page and out.channel_count == 2
        rn = rn_of(out)
        assert rn.dtype == np.int64 and bool((rn == 1).all())
        fed += rows_per_page
    count, capacity = op.rowNumberStats()
    assert count == fed
    assert capacity > before and capacity >= 2 * fed and capacity & (capacity - 1) == 0
    assert op.memoryBytes() >= capacity * 8 + fed * 16            # slots, stored keys and the counts


# ---- numpy restatement for the large cases -----------------------------------------------------------------------------------------
def numpy_row_numbers(keys):
    """1 + the number of earlier rows with the same key, for an int64 key array."""
    order = np.argsort(keys, kind="stable")
    sk = keys[order]
    head = np.ones(len(keys), bool)
    head[1:] = sk[1:] != sk[:-1]
    start = np.maximum.accumulate(np.where(head, np.arange(len(keys)), 0))
    rn = np.empty(len(keys), np.int64)
    rn[order] = np.arange(len(keys)) - start + 1
    return rn


def run_numpy(keys, sizes, device=True, cap=None, expected_positions=0):
    """int64 keys through RowNumberOperator([BIGINT], [0], [0]) in pages of `sizes` (the last size repeats) -> (row numbers by input
    position or, under a cap, (kept positions, row numbers); raw bytes of every row number column; operator)."""
    op = RowNumberOperator([abi.BIGINT, abi.BIGINT], [1], [0], cap, output_mem=abi.MEM_DEVICE if device else abi.MEM_HOST, expected_positions=expected_positions)
    got, kept, at, i = [], [], 0, 0
    while at < len(keys):
        n = sizes[min(i, len(sizes) - 1)]
        part = keys[at:at + n]
        page = Page([Block.bigint(part), Block.bigint(np.arange(at, at + len(part), dtype=np.int64))], len(part))
        assert op.needsInput()
        op.addInput(upload_page(page) if device else page)
        out = raw_output(op)
        if out is not None:
            got.append(rn_of(out))
            if cap is not None:
                kept.append(host_page_of(op, out).blocks[0].values[:out.position_count].astype(np.int64))
        else:
            assert cap is not None
        at += n
        i += 1
    rn = np.concatenate(got) if got else np.zeros(0, np.int64)
    if cap is not None:
        return (np.concatenate(kept) if kept else np.zeros(0, np.int64), rn), op
    return rn, op


# ---- order independence --------------------------------------------------------------------------------------------------------------
def test_one_key_on_every_row_of_a_large_page(gpu):
    """2^22 rows, one key: exactly 1 .. n -- the run crosses every workgroup of the rank pass."""
    n = 1 << 22
    rn, op = run_numpy(np.full(n, 42, np.int64), [n])
    assert np.array_equal(rn, np.arange(1, n + 1, dtype=np.int64))
    assert op.rowNumberStats()[0] == 1
    # ... and the count carries: a second page of the same key goes on at n + 1
    page = upload_page(Page([Block.bigint(np.full(1000, 42, np.int64)), Block.bigint(np.arange(1000, dtype=np.int64))], 1000))
    op.addInput(page)
    assert np.array_equal(rn_of(raw_output(op)), np.arange(n + 1, n + 1001, dtype=np.int64))


def test_long_runs_that_start_at_odd_offsets(gpu):
    """Runs longer than a workgroup's 1024 pairs whose heads fall at odd places of the sorted order: 3 rows of key 0, then runs of
    1025, 4097, 1, 2049, 9999 and 65537 rows, scattered over the page."""
    rng = np.random.default_rng(21)
    lengths = [3, 1025, 4097, 1, 2049, 9999, 65537, 1023, 5]
    keys = np.concatenate([np.full(c, k, np.int64) for k, c in enumerate(lengths)])
    for layout in ("sorted", "shuffled", "reversed"):
        ks = keys if layout == "sorted" else (keys[rng.permutation(len(keys))] if layout == "shuffled" else keys[::-1].copy())
        rn, _ = run_numpy(ks, [len(ks)])
        assert np.array_equal(rn, numpy_row_numbers(ks)), layout


def test_a_run_crosses_every_block_boundary(gpu):
    """Keys laid out so that in the sorted order a run ends one pair behind every multiple of 1024 -- every workgroup of the rank pass
    starts inside a run that began in the workgroup before it -- and, second layout, exactly on every multiple (no run crosses)."""
    blocks = 300
    for shift in (1, 0, 513):
        lengths = [1024 + shift] + [1024] * (blocks - 1) if shift else [1024] * blocks
        keys = np.concatenate([np.full(c, k, np.int64) for k, c in enumerate(lengths)])
        keys = keys[np.random.default_rng(22 + shift).permutation(len(keys))]
        rn, _ = run_numpy(keys, [len(keys)])
        assert np.array_equal(rn, numpy_row_numbers(keys)), shift


def test_page_cuts_do_not_change_the_numbers(gpu):
    rng = np.random.default_rng(23)
    n = 200_000
    keys = rng.integers(0, 3000, n).astype(np.int64)
    keys[50_000:60_000] = 7                                           # a long run in the middle
    want = numpy_row_numbers(keys)
    whole, op = run_numpy(keys, [n])
    assert np.array_equal(whole, want)
    assert op.rowNumberStats()[0] == len(np.unique(keys))
    for size in (1024, 1025):
        got, _ = run_numpy(keys, [size])
        assert np.array_equal(got, want), size
    # pages of 1 and 7 rows over a prefix (a page per row is host time), then the rest in one page
    for small in (1, 7):
        sizes = [small] * (2100 // small) + [n]
        got, _ = run_numpy(keys, sizes, device=(small == 7))
        assert np.array_equal(got, want), small


def test_the_same_input_twice_gives_identical_bytes(gpu):
    rng = np.random.default_rng(24)
    half = 1 << 19
    keys = np.concatenate([np.arange(half), np.arange(half), np.zeros(1000, np.int64)]).astype(np.int64) * 2654435761
    keys = keys[rng.permutation(len(keys))]
    want = numpy_row_numbers(keys)
    first, _ = run_numpy(keys, [len(keys)])
    second, _ = run_numpy(keys, [len(keys)])
    assert np.array_equal(first, want)
    assert first.tobytes() == second.tobytes()
    (kept1, rn1), _ = run_numpy(keys, [1 << 18], cap=1)
    (kept2, rn2), _ = run_numpy(keys, [1 << 18], cap=1)
    assert np.array_equal(kept1, np.flatnonzero(want == 1)) and bool((rn1 == 1).all())
    assert kept1.tobytes() == kept2.tobytes() and rn1.tobytes() == rn2.tobytes()


# ---- edges ---------------------------------------------------------------------------------------------------------------------------
def test_null_keys(gpu):
    run_rows([abi.BIGINT], [(None,), (1,), (None,), (0,), (1,), (None,)], [0])
    run_rows([abi.BIGINT], [(None,), (None,), (5,)], [0], sizes=[1, 1, 1])
    run_rows([abi.VARCHAR], [(None,), ("",), (None,), ("",), ("a",)], [0])        # the empty string is not NULL
    run_rows([abi.BIGINT], [(None,), (1,), (None,), (0,), (1,), (None,)], [0], cap=2)


@pytest.mark.parametrize("t", [abi.DOUBLE, abi.REAL])
def test_nan_and_signed_zero(gpu, t):
    nan, other_nan = float("nan"), np.frombuffer(np.uint64(0x7FF0000000000123).tobytes(), np.float64)[0]
    third_nan = np.frombuffer(np.uint64(0xFFF8000000000001).tobytes(), np.float64)[0]
    if t == abi.REAL:
        other_nan = np.frombuffer(np.uint32(0x7FC01234).tobytes(), np.float32)[0]
        third_nan = np.frombuffer(np.uint32(0xFFC00001).tobytes(), np.float32)[0]
    rows = [(nan,), (-0.0,), (other_nan,), (0.0,), (1.5,), (-1.5,), (None,), (nan,), (-0.0,), (1.5,), (None,), (third_nan,)]
    run_rows([t], rows, [0])
    run_rows([t], rows, [0], sizes=[3, 1, 4])
    run_rows([t], list(reversed(rows)), [0], device_input=True, output_mem=abi.MEM_DEVICE)
    run_rows([t], rows, [0], cap=2, device_input=True)


def test_boolean_bytes_other_than_0_and_1(gpu):
    run_rows([abi.BOOLEAN], [(2,), (1,), (0,), (255,), (None,), (0,), (7,)], [0])
    run_rows([abi.BOOLEAN, abi.BOOLEAN], [(2, 0), (1, 0), (1, 3), (9, 1), (0, 0), (None, 0), (0, None)], [0, 1])


def test_every_supported_key_type(gpu):
    run_rows([abi.REAL], [(1.25,), (1.25,), (-1.25,), (3.0e38,), (1.0e-40,), (3.0e38,)], [0])
    run_rows([abi.INTEGER], [(5,), (-5,), (5,), (None,), (2**31 - 1,), (-2**31,), (5,)], [0])
    run_rows([abi.DATE, abi.INTEGER], [(1, -1), (1, -1), (2, -1), (1, 1)], [0, 1])
    run_rows([abi.BIGINT], [(2**63 - 1,), (-2**63,), (0,), (2**63 - 1,), (-2**63,)], [0])
    t = abi.decimal(12, 2)
    op = RowNumberOperator([t, abi.BIGINT], [0, 1], [0])
    out = to_pages(op, [Page([Block.decimal([12345, -5, 0, 12345, 5, -5]), Block.bigint(list(range(6)))], 6)])
    assert [r[-1] for p in out for r in p.to_rows()] == [1, 1, 1, 2, 1, 2]


def test_varchar_lengths(gpu):
    rows = [(b"",), (b"a",), (b"abcdefghijklmnop",), (b"abcdefghijklmnoq",), (b"abcdefghX",), (b"abcdefghY",), (b"abcdefgh",), (b"x" * 100,),
            (b"x" * 99,), (None,), (b"abcdefghY",), (b"x" * 100,), (b"",), (None,), (b"abcdefghijklmnop",)]
    run_rows([abi.VARCHAR], rows, [0])
    run_rows([abi.VARCHAR], rows, [0], sizes=[4, 4, 4], device_input=True)
    run_rows([abi.VARCHAR], rows * 3, [0], sizes=[7], cap=2, device_input=True, output_mem=abi.MEM_DEVICE)


def test_two_to_eight_partition_channels(gpu):
    types = [abi.BIGINT, abi.DOUBLE, abi.VARCHAR]
    rows = [(None, 1.0, "a"), (None, 2.0, "a"), (1, None, "a"), (1, 1.0, None), (None, None, None), (None, 1.0, "a"), (1, None, "a"),
            (0, 0.0, ""), (None, 0.0, ""), (0, None, ""), (0, -0.0, ""), (None, None, None), (1, 1.0, "a"), (1, 1.0, "b"), (1, 1.0, "a")]
    run_rows(types, rows, [0, 1, 2])
    run_rows(types, rows, [2, 0], sizes=[5, 5], hashed=True)
    run_rows(types, rows, [1, 2, 0], cap=1, hashed=True, output_channels=[3, 2, 4])
    # (NULL, 1) and (NULL, 2) are different partitions; (NULL, 1) and (0, 1) too
    run_rows([abi.BIGINT, abi.BIGINT], [(None, 1), (None, 2), (0, 1), (None, 1), (0, None), (0, 0), (0, None)], [0, 1])
    eight = [abi.BIGINT, abi.INTEGER, abi.DATE, abi.DOUBLE, abi.REAL, abi.BOOLEAN, abi.VARCHAR, abi.BIGINT]
    base = (1, 2, 3, 4.0, 5.0, 1, "s", 8)
    rows8 = [base, base] + [tuple(None if c == i else v for c, v in enumerate(base)) for i in range(8)] + [base, tuple([None] * 8), tuple([None] * 8)]
    for k in range(2, 9):
        run_rows(eight, rows8, list(range(k)))
    run_rows(eight, rows8, [7, 6, 5, 4, 3, 2, 1, 0], cap=2)


# ---- encodings and memory spaces -------------------------------------------------------------------------------------------------------
def test_dictionary_and_rle_key_channels(gpu):
    key = Block.dictionary_block(Block.flat(abi.BIGINT, [5, 4, 0], [0, 0, 1]), [0, 1, 2, 2, 0, 1])
    rle = Block.rle(Block.bigint([4]), 6)
    strings = Block.dictionary_block(Block.varchar(["x", "yy", None]), [1, 1, 2, 0, 2, 0])
    for output_mem in (abi.MEM_HOST, abi.MEM_DEVICE):
        for cap in (None, 3):
            for t, k in ((abi.BIGINT, key), (abi.BIGINT, rle), (abi.VARCHAR, strings)):
                op = RowNumberOperator([t, abi.BIGINT], [0, 1], [0], cap, output_mem=output_mem)
                model = Model([t], cap)
                for page in (Page([k, Block.bigint(list(range(6)))], 6), upload_page(Page([k, Block.bigint(list(range(6)))], 6))):
                    want = model.page([(v,) for v in k.to_pylist()])
                    op.addInput(page)
                    out = raw_output(op)
                    if not want:                                            # (the RLE page under the cap, second time round)
                        assert out is None
                        continue
                    assert rn_of(out).tolist() == [rn for _, rn in want], (output_mem, cap, k.encoding)
                    if cap is not None or out.mem == abi.MEM_HOST:      # flat copies / a decoded host page
                        got = host_page_of(op, out).to_rows()
                        assert [g[1] for g in got] == [i for i, _ in want]
                        assert [canon(t, g[0]) for g in got] == [canon(t, k.to_pylist()[i]) for i, _ in want]
                op.close()


def test_host_and_device_input_and_output(gpu):
    types = [abi.VARCHAR, abi.BIGINT, abi.DOUBLE]
    rows = [("a", 1, 0.5), (None, 5, -1.0), ("ccc", 3, None), ("a", 1, 3.0), ("a", 2, 3.0), (None, 5, 1.0)]
    for device_input in (False, True):
        for output_mem in (abi.MEM_HOST, abi.MEM_DEVICE):
            for cap in (None, 1):
                run_rows(types, rows, [0, 1], cap=cap, device_input=device_input, output_mem=output_mem, sizes=[4])
                run_rows(types, rows, [], cap=cap if cap is None else 5, device_input=device_input, output_mem=output_mem, sizes=[4])


def test_zero_copy_output_carries_the_callers_blocks(gpu):
    """device -> device without a cap: the input blocks themselves for the output channels, in descriptor order, encodings included; only
    the row number column is new, and it has no nulls."""
    names = Block.varchar(["a", None, "ccc", "a"])
    dic = Block.dictionary_block(Block.varchar(["x", "yy"]), [1, 0, 0, 1])
    types = [abi.VARCHAR, abi.BIGINT, abi.VARCHAR, abi.DOUBLE]
    host = Page([names, Block.bigint([1, 5, 3, 1]), dic, Block.double([0.5, -1.0, 2.0, 3.0])], 4)
    dev = upload_page(host)
    order = [2, 0, 3, 1]
    op = RowNumberOperator(types, order, [0, 1], output_mem=abi.MEM_DEVICE)
    cpage, _keep = dev.to_c()
    check(lib().pa_op_add_input(op._h, C.byref(cpage)))
    out = abi.pa_page()
    assert check(lib().pa_op_get_output(op._h, C.byref(out))) == 1
    assert out.channel_count == 5 and out.position_count == 4 and out.mem == abi.MEM_DEVICE
    for o, c in enumerate(order):
        assert out.columns[o].type == cpage.columns[c].type
        assert out.columns[o].encoding == cpage.columns[c].encoding
        assert out.columns[o].values == cpage.columns[c].values
        assert out.columns[o].offsets == cpage.columns[c].offsets
        assert out.columns[o].nulls == cpage.columns[c].nulls
        assert out.columns[o].ids == cpage.columns[c].ids
    assert out.columns[0].encoding == abi.DICTIONARY
    assert out.columns[0].dictionary[0].values == cpage.columns[2].dictionary[0].values
    assert rn_of(out).tolist() == [1, 1, 1, 2]
    op.close()
    # host in -> host out / device out: the same values, decoded
    for output_mem in (abi.MEM_HOST, abi.MEM_DEVICE):
        op = RowNumberOperator(types, order, [0, 1], output_mem=output_mem)
        op.addInput(host)
        out = raw_output(op)
        assert out.mem == output_mem
        got = host_page_of(op, out).to_rows()
        assert [r[:-1] for r in got] == [tuple(row[c] for c in order) for row in host.to_rows()]
        assert [r[-1] for r in got] == [1, 1, 1, 2]


# ---- the cap -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [0, 1, 3, 1000])
def test_cap_values(gpu, cap):
    rng = np.random.default_rng(30 + cap)
    rows = [(int(k), "payload-%d" % i if i % 7 else None, float(i) if i % 5 else None) for i, k in enumerate(rng.integers(0, 40, 3000))]
    types = [abi.BIGINT, abi.VARCHAR, abi.DOUBLE]           # VARCHAR and nullable payload columns go through the compaction
    for device in (False, True):
        op = run_rows(types, rows, [0], cap=cap, sizes=[500, 1, 999], device_input=device, output_mem=abi.MEM_DEVICE if device else abi.MEM_HOST)
        assert op.rowNumberStats()[0] == 40
    run_rows(types, rows[:700], [], cap=cap, sizes=[300])


def test_counts_saturate_at_the_cap(gpu):
    """A partition that stands at m stays at m: later pages of its rows produce no page, whatever their length, and a new partition
    still gets its m rows."""
    n = 1 << 16
    (kept, rn), op = run_numpy(np.concatenate([np.full(3 * n, 9, np.int64), np.array([9, 4, 9, 4, 4, 4, 9], np.int64)]), [n, n, n, 7], cap=3)
    assert kept.tolist() == [0, 1, 2, 3 * n + 1, 3 * n + 3, 3 * n + 4] and rn.tolist() == [1, 2, 3, 1, 2, 3]
    assert op.rowNumberStats()[0] == 2
    # cap 0 with partitions keeps nothing, ever
    (kept, rn), op = run_numpy(np.arange(5000, dtype=np.int64) % 11, [1000], cap=0)
    assert len(kept) == 0 and len(rn) == 0 and op.rowNumberStats()[0] == 11
    assert op.needsInput() and not op.isFinished()


def test_cap_inside_large_pages(gpu):
    rng = np.random.default_rng(31)
    n = 1 << 20
    keys = rng.integers(0, 50000, n).astype(np.int64)
    want = numpy_row_numbers(keys)
    for cap in (1, 5, 40):
        (kept, rn), _ = run_numpy(keys, [1 << 18], cap=cap)
        sel = np.flatnonzero(want <= cap)
        assert np.array_equal(kept, sel) and np.array_equal(rn, want[sel]), cap


# ---- the state machine -----------------------------------------------------------------------------------------------------------------
def test_state_machine_partitioned(gpu):
    for cap in (None, 2):
        op = RowNumberOperator([abi.BIGINT], [0], [0], cap)
        assert op.needsInput() and not op.isFinished() and op.getOutput() is None
        empty = Page([Block.bigint([])], 0)
        check(lib().pa_op_add_input(op._h, C.byref(empty.to_c()[0])))                              # a page of zero rows: nothing
        assert op.getOutput() is None and op.needsInput()
        page = Page([Block.bigint([1, 1, 1])], 3)
        op.addInput(page)
        assert not op.needsInput() and not op.isFinished()
        assert lib().pa_op_add_input(op._h, C.byref(page.to_c()[0])) == abi.ERR_ILLEGAL_STATE      # a page is pending
        op.finish()
        assert not op.isFinished()                                                                # finishing, but a page is pending
        assert rn_of(raw_output(op)).tolist() == ([1, 2, 3] if cap is None else [1, 2])
        assert op.isFinished() and not op.needsInput() and op.getOutput() is None
        assert lib().pa_op_add_input(op._h, C.byref(page.to_c()[0])) == abi.ERR_ILLEGAL_STATE
        op.close()
    op = RowNumberOperator([abi.BIGINT], [0], [0], 2)
    op.addInput(Page([Block.bigint([1, 1])], 2))
    assert op.getOutput().position_count == 2
    op.addInput(Page([Block.bigint([1, 1, 1])], 3))                                                # keeps nothing: no page, input wanted
    assert op.needsInput() and op.getOutput() is None and not op.isFinished()
    count, capacity = C.c_int64(), C.c_int64()
    agg = HashAggregationOperator([abi.BIGINT], [0], [(abi.AGG_COUNT_STAR, -1, None)])
    assert lib().pa_row_number_stats(agg._h, C.byref(count), C.byref(capacity)) == abi.ERR_INVALID_ARGUMENT
    assert lib().pa_distinct_stats(op._h, C.byref(count), C.byref(capacity)) == abi.ERR_INVALID_ARGUMENT
    assert op.kernelName() == "k_distinct_insert_ids"
    ms, launches = op.kernelTime()
    assert launches == 2 and ms > 0


def test_state_machine_single_partition(gpu):
    # without a cap: never finished before finish()
    op = RowNumberOperator([abi.BIGINT], [0], [])
    for start in (0, 5):
        assert op.needsInput() and not op.isFinished()
        op.addInput(Page([Block.bigint([7] * 5)], 5))
        assert not op.needsInput()
        assert op.getOutput().to_rows() == [(7, start + i + 1) for i in range(5)]
    op.finish()
    assert op.isFinished() and op.getOutput() is None
    # with a cap: finished as soon as the count equals it and nothing is pending
    op = RowNumberOperator([abi.BIGINT], [0], [], 7)
    page = Page([Block.bigint([1, 2, 3, 4, 5])], 5)
    op.addInput(page)
    assert op.getOutput().to_rows() == [(i + 1, i + 1) for i in range(5)]
    assert op.needsInput() and not op.isFinished()
    op.addInput(upload_page(page))
    assert not op.needsInput() and not op.isFinished()                   # the cap is reached, but a page is pending
    assert op.getOutput().to_rows() == [(1, 6), (2, 7)]
    assert not op.needsInput() and op.isFinished()
    assert lib().pa_op_add_input(op._h, C.byref(page.to_c()[0])) == abi.ERR_ILLEGAL_STATE
    # cap 0: finished at creation
    op = RowNumberOperator([abi.BIGINT], [0], [], 0)
    assert not op.needsInput() and op.isFinished() and op.getOutput() is None
    assert lib().pa_op_add_input(op._h, C.byref(page.to_c()[0])) == abi.ERR_ILLEGAL_STATE
    assert op.rowNumberStats() == (1, 0)


def test_retained_pages_are_released_exactly_once(gpu):
    """A PA_PAGE_RETAINED page is released once its output page has been let go -- not before (the zero-copy output page IS the input's
    blocks: the release callback scribbles over them), and exactly once whatever the mode."""
    from tests.test_gpu_small_pages import retained_pages
    n = 40_000
    keys = np.arange(n, dtype=np.int64) % 977
    host = Page([Block.bigint(keys), Block.double(np.arange(n, dtype=np.float64))], n)
    bounds = [0, 7000, 7001, 20_000, n]
    want = numpy_row_numbers(keys)
    for cap, partition in ((None, [0]), (2, [0]), (None, []), (9000, [])):
        released = []
        pages = retained_pages(host, bounds, released)
        op = RowNumberOperator([abi.BIGINT, abi.DOUBLE], [1, 0], partition, cap, output_mem=abi.MEM_DEVICE)
        for i, p in enumerate(pages):
            if not op.needsInput():
                break
            op.addInput(p)
            assert released == list(range(i))                            # page i is still held
            out = raw_output(op)
            if out is not None and cap is None:
                lo, hi = bounds[i], bounds[i + 1]
                got = host_page_of(op, out)                                  # reads the caller's blocks: they must still be intact
                assert np.array_equal(got.blocks[1].values[:hi - lo], keys[lo:hi])
                assert np.array_equal(got.blocks[0].values[:hi - lo], np.arange(lo, hi, dtype=np.float64))
                if partition:
                    assert np.array_equal(got.blocks[2].values[:hi - lo], want[lo:hi])
            # (a page that produced nothing is let go as soon as the operator is asked for output)
            assert released == list(range(i + 1 if out is None else i))
            op.needsInput()                                                  # the output page has been let go
            assert released == list(range(i + 1))
        op.finish()
        op.close()
        fed = len(released)
        assert released == list(range(fed)) and fed >= (2 if cap == 9000 else len(pages))


# ---- growth ------------------------------------------------------------------------------------------------------------------------------
def test_growth_from_one_expected_position(gpu):
    """From expected_positions = 1 to more than 2^20 partitions: the counts survive every rehash, memory grows with the table."""
    rng = np.random.default_rng(33)
    total = (1 << 20) + 50_000
    keys = rng.permutation(total).astype(np.int64) * 7 - 3
    keys = np.concatenate([keys[:1000], keys[:1000], keys[1000:300_000], keys[:300_000], keys[300_000:], keys[:5]])
    op = RowNumberOperator([abi.BIGINT], [0], [0], expected_positions=1, output_mem=abi.MEM_DEVICE)
    capacities, memory = [op.rowNumberStats()[1]], [op.memoryBytes()]
    assert capacities[0] <= 64
    got, at = [], 0
    sizes = [1, 10, 100, 889, 1000, 8000, 40000, 50000, 200_000, 299_000, 400_000, 400_000]
    sizes.append(len(keys) - sum(sizes))
    for n in sizes:
        op.addInput(upload_page(Page([Block.bigint(keys[at:at + n])], n)))
        got.append(rn_of(raw_output(op)))
        at += n
        count, capacity = op.rowNumberStats()
        assert count == len(np.unique(keys[:at]))
        assert capacity & (capacity - 1) == 0 and capacity >= 2 * count
        capacities.append(capacity)
        memory.append(op.memoryBytes())
    assert at == len(keys)
    assert np.array_equal(np.concatenate(got), numpy_row_numbers(keys))
    assert op.rowNumberStats()[0] == total > (1 << 20)
    assert capacities == sorted(capacities) and len(set(capacities)) >= 8       # several rehashes
    assert memory[-1] > memory[0] and memory[-1] >= capacities[-1] * 8 + total * 16


def test_growth_with_varchar_and_two_channels(gpu):
    rng = np.random.default_rng(34)
    rows = [("s%d" % v, int(v) % 3 if v % 5 else None) for v in rng.integers(0, 20000, 30000)]
    run_rows([abi.VARCHAR, abi.BIGINT], rows, [0, 1], sizes=[10, 100, 1000, 5000, 10000], expected_positions=1)
    run_rows([abi.VARCHAR, abi.BIGINT], rows, [0, 1], sizes=[10, 100, 1000, 5000, 10000], expected_positions=1, cap=2)


def test_memory_limit_applies_to_growth(gpu):
    L = lib()
    op = RowNumberOperator([abi.BIGINT], [0], [0], expected_positions=1)
    op.addInput(Page([Block.bigint([1, 2, 3])], 3))
    assert op.getOutput().position_count == 3
    n = 1 << 22
    page = upload_page(Page([Block.bigint(np.arange(n, dtype=np.int64))], n))
    cpage, _keep = page.to_c()
    L.pa_memory_set_limit(32 << 20)             # the table for 4 Mi more keys alone is 64 MiB
    try:
        assert L.pa_op_add_input(op._h, C.byref(cpage)) == abi.ERR_INSUFFICIENT_RESOURCES
    finally:
        L.pa_memory_set_limit(0)
    op.close()


# ---- cross-checks against operators that exist ---------------------------------------------------------------------------------------------
def cross_pages(seed, device):
    rng = np.random.default_rng(seed)
    n, pages = 50_000, 4
    g = rng.integers(0, 4000, n * pages).astype(np.int64)
    x = rng.integers(-3, 3, n * pages).astype(np.float64) * 0.5          # -0.0 among them
    src = []
    for p in range(pages):
        page = Page([Block.bigint(g[p * n:(p + 1) * n]), Block.double(x[p * n:(p + 1) * n])], n)
        src.append(upload_page(page) if device else page)
    return g, x, src


@pytest.mark.parametrize("device", [False, True])
def test_first_rows_are_mark_distincts_marks(gpu, device):
    """rn == 1 exactly where MarkDistinctOperator marks the row, page by page."""
    _, _, src = cross_pages(40, device)
    mem = abi.MEM_DEVICE if device else abi.MEM_HOST
    rn_op = RowNumberOperator([abi.BIGINT, abi.DOUBLE], [0, 1], [0, 1], output_mem=mem)
    mark_op = MarkDistinctOperator([abi.BIGINT, abi.DOUBLE], [0, 1], output_mem=mem)
    for page in src:
        rn_op.addInput(page)
        mark_op.addInput(page)
        rn = rn_of(raw_output(rn_op))
        out = abi.pa_page()
        assert check(lib().pa_op_get_output(mark_op._h, C.byref(out))) == 1
        col = out.columns[out.channel_count - 1]
        n = out.position_count
        marks = download(DeviceBuffer(col.values, n), np.uint8, n) if out.mem == abi.MEM_DEVICE else np.frombuffer(C.string_at(col.values, n), np.uint8)
        assert np.array_equal(rn == 1, marks == 1)
    assert rn_op.rowNumberStats()[0] == mark_op.distinctStats()[0]


@pytest.mark.parametrize("device", [False, True])
def test_largest_row_number_is_the_aggregations_count(gpu, device):
    """max(rn) per key == count(*) GROUP BY the key (HashAggregationOperator)."""
    g, x, src = cross_pages(41, device)
    mem = abi.MEM_DEVICE if device else abi.MEM_HOST
    rn_op = RowNumberOperator([abi.BIGINT, abi.DOUBLE], [0, 1], [0], output_mem=mem)
    largest = {}
    at = 0
    for page in src:
        rn_op.addInput(page)
        rn = rn_of(raw_output(rn_op))
        keys = g[at:at + len(rn)]
        top = np.zeros(4000, np.int64)
        np.maximum.at(top, keys, rn)
        for k in np.flatnonzero(top):
            largest[int(k)] = max(largest.get(int(k), 0), int(top[k]))
        at += len(rn)
    agg = HashAggregationOperator([abi.BIGINT, abi.DOUBLE], [0], [(abi.AGG_COUNT_STAR, -1, None)])
    counts = {r[0]: r[1] for p in to_pages(agg, [Page([Block.bigint(g), Block.double(x)], len(g))]) for r in p.to_rows()}
    assert largest == counts


# ---- seeded fuzz ---------------------------------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("seed", range(FUZZ_SEEDS))
def test_fuzz_row_number(gpu, seed):
    rng = np.random.default_rng(3000 + seed)
    nt = int(rng.integers(1, 5))
    types = [FUZZ_TYPES[int(rng.integers(0, len(FUZZ_TYPES)))] for _ in range(nt)]
    n = int(rng.integers(1, 9000))
    domain = int(rng.choice([1, 2, 30, 1000, 1 << 30]))     # cardinality from 1 to all-distinct: the per-channel domain
    cols = [_fuzz_column(rng, t, n, domain if t != abi.VARCHAR else min(domain, 1 << 20), float(rng.choice([0.0, 0.02, 0.4]))) for t in types]
    rows = list(zip(*cols))
    sizes = [int(s) for s in rng.integers(1, max(2, n // 2), int(rng.integers(1, 6)))]
    nk = int(rng.integers(0, nt + 1))                       # 0: the single partition
    partition = [int(c) for c in rng.permutation(nt)[:nk]]
    cap = [None, 0, 1, 3, 50, 10**9][int(rng.integers(0, 6))]
    device = bool(rng.integers(0, 2))
    run_rows(types, rows, partition, cap=cap, sizes=sizes, hashed=bool(rng.integers(0, 2)), output_mem=int(rng.integers(0, 2)), device_input=device,
             expected_positions=int(rng.choice([0, 1, 100])))


# ---- a scrubbed pool, in a child process ---------------------------------------------------------------------------------------------------
def test_on_a_scrubbed_pool(gpu):
    """Growth, VARCHAR keys and the cap once more with every recycled HBM block overwritten before it is handed out
    (PRESTO_AMD_POOL_SCRUB, pool.cpp): counts, a table or a store that relied on what a block's previous owner left behind fail here."""
    env = dict(os.environ, PRESTO_AMD_POOL_SCRUB="0xA5", PA_FUZZ_SEEDS="4")
    picks = ["test_growth_with_varchar_and_two_channels", "test_cap_values", "test_fuzz_row_number", "test_two_to_eight_partition_channels",
             "test_page_cuts_do_not_change_the_numbers", "test_counts_saturate_at_the_cap"]
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider", "tests/test_gpu_row_number.py", "-k",
                        " or ".join(picks)], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    tail = r.stdout.decode()[-3000:]
    assert r.returncode == 0, tail
    assert " passed" in tail and "failed" not in tail


# ---- the C++ mirror (include/presto_amd.hpp) -------------------------------------------------------------------------------------------------
def test_cpp_mirror(gpu):
    """tests/cpp/test_row_number.cpp: the operator through the C++ host mirror's runDriver."""
    exe = os.path.join(ROOT, "tests", "cpp", "test_row_number")
    src = exe + ".cpp"
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-L" + os.path.join(ROOT, "presto_amd"),
                               "-lpresto_amd", "-Wl,-rpath,$ORIGIN/../../presto_amd", "-Wl,--allow-shlib-undefined", "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode == 0, r.stdout.decode()[-2000:]
    assert "row number ok" in r.stdout.decode()
