"""GPU checks of TopNRankingOperator against a restatement of its contract in this file (include/presto_amd.h: partitions under IS NOT
DISTINCT FROM in first-seen order, SimplePageWithPositionComparator inside a partition, ties in arrival order, row_number / rank <= n):
the reference's own known answers (TestTopNRankingOperator), independence of page cuts and of when the operator prunes, ties across
prunes, the NULL / NaN / -0.0 edges under all four sort orders, encodings and memory spaces, the state machine, bounded state, cross-checks
against operators that exist, seeded fuzz.  Every comparison is exact: values, order, ranking column.  The oracle has no such operator:
the expected rows come from `model` (rows as Python values) and `np_model` (large numeric inputs) below."""
import ctypes as C
import functools
import math
import os
import struct
import subprocess
import sys
from contextlib import contextmanager

import numpy as np
import pytest

from presto_amd import abi
from presto_amd._lib import check, lib
from presto_amd.operators import (HashAggregationOperator, OrderByOperator, RowNumberOperator, TopNOperator, TopNRankingOperator, download_page,
                                  to_pages, upload_page)
from presto_amd.page import Block, Page

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROW_NUMBER, RANK = abi.RANKING_ROW_NUMBER, abi.RANKING_RANK
ASC_NULLS_FIRST, ASC_NULLS_LAST, DESC_NULLS_FIRST, DESC_NULLS_LAST = 0, 1, 2, 3
PRUNE_ENV = "PRESTO_AMD_TOPN_RANKING_PRUNE_ROWS"
DEFAULT_PRUNE_ROWS = 1 << 22
NAN = float("nan")


# ---- the contract, restated --------------------------------------------------------------------------------------------------------
def canon(t, v):
    """Partition equality: IS NOT DISTINCT FROM (NaN matches NaN, -0.0 matches +0.0; BOOLEAN: any non-zero byte is true; NULL is one value)."""
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


def model(types, rows, partition, sort, orders, n, ranking=ROW_NUMBER):
    """-> [(input position, row number / rank)] in output order."""
    groups = {}
    for i, r in enumerate(rows):
        groups.setdefault(tuple(canon(types[c], r[c]) for c in partition), []).append(i)      # first-seen order (dict order)
    compare = comparator([types[c] for c in sort], orders)
    key = functools.cmp_to_key(lambda i, j: compare([rows[i][c] for c in sort], [rows[j][c] for c in sort]))
    out = []
    for members in groups.values():
        ordered = sorted(members, key=key)                                                  # stable: ties in arrival order
        value = 0
        for place, i in enumerate(ordered, 1):
            if ranking == ROW_NUMBER or place == 1 or key(ordered[place - 2]) != key(i):
                value = place                                                                # rank: 1 + the rows strictly smaller
            if value <= n:
                out.append((i, value))
    return out


def np_model(part, keys, n, ranking=ROW_NUMBER):
    """The same for numeric columns without NULL / NaN / -0.0, ascending: part (or None) and the list of sort key arrays ->
    (input positions in output order, row number / rank)."""
    total = len(keys[0])
    if part is None:
        gid = np.zeros(total, np.int64)
    else:
        uniq, first, inverse = np.unique(part, return_index=True, return_inverse=True)
        seen_rank = np.empty(len(uniq), np.int64)
        seen_rank[np.argsort(first, kind="stable")] = np.arange(len(uniq))
        gid = seen_rank[inverse]
    order = np.lexsort(tuple([np.arange(total)] + list(reversed(keys)) + [gid]))
    g = gid[order]
    at = np.arange(total)
    head = np.r_[True, g[1:] != g[:-1]]
    run_start = np.maximum.accumulate(np.where(head, at, 0))
    value = at - run_start + 1
    if ranking == RANK:
        peer_head = head.copy()
        for k in keys:
            ks = k[order]
            peer_head |= np.r_[True, ks[1:] != ks[:-1]]
        value = np.maximum.accumulate(np.where(peer_head, at, 0)) - run_start + 1
    keep = value <= n
    return order[keep], value[keep]


# ---- driving the operator ------------------------------------------------------------------------------------------------------------
@contextmanager
def prune_rows(value):
    """The prune threshold is read when an operator is created."""
    old = os.environ.get(PRUNE_ENV)
    if value is None:
        os.environ.pop(PRUNE_ENV, None)
    else:
        os.environ[PRUNE_ENV] = str(value)
    try:
        yield
    finally:
        if old is None:
            os.environ.pop(PRUNE_ENV, None)
        else:
            os.environ[PRUNE_ENV] = old


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


def run_rows(types, rows, partition, sort, orders, n, ranking=ROW_NUMBER, partial=False, sizes=None, hashed=False, output_mem=abi.MEM_HOST,
             device_input=False, expected_positions=0, output_channels=None, prune=None):
    """rows (tuples over `types`) through a TopNRankingOperator over (types..., BIGINT row index, [$hashvalue]) pages cut by `sizes`; the
    concatenated output is compared with the restatement: which rows, in which order, with which ranking, every output value.  Returns
    (the output as (input position, ranking) pairs, the operator)."""
    nt = len(types)
    page_types = list(types) + [abi.BIGINT] + ([abi.BIGINT] if hashed else [])
    out_ch = list(range(nt + 1)) if output_channels is None else list(output_channels)
    assert nt in out_ch                                   # the index column identifies the rows
    with prune_rows(prune):
        op = TopNRankingOperator(page_types, out_ch, partition, sort, orders, n, ranking_type=ranking, partial=partial,
                                 hash_channel=len(page_types) - 1 if hashed else -1, expected_positions=expected_positions, output_mem=output_mem)
    at = 0
    for chunk in split(rows, sizes or [max(len(rows), 1)]):
        m = len(chunk)
        blocks = [block(t, [r[c] for r in chunk]) for c, t in enumerate(types)] + [Block.bigint(list(range(at, at + m)))]
        blocks += [hash_block(m)] if hashed else []
        page = Page(blocks, m)
        assert op.needsInput()
        op.addInput(upload_page(page) if device_input else page)
        at += m
    want = model(types, rows, partition, sort, orders, n, ranking)
    pages = drain(op)
    got = [r for p in pages for r in p.to_rows()]
    if not want:
        assert pages == []                                # an operator that kept nothing produces no page
    assert len(got) == len(want)
    width = len(out_ch) + (0 if partial else 1)
    at_index = out_ch.index(nt)
    for g, (i, value) in zip(got, want):
        assert len(g) == width
        assert g[at_index] == i, (g, i, value)
        for c, v in zip(out_ch, g):
            if c < nt:
                assert same_value(types[c], v, rows[i][c]), (i, c, v, rows[i][c])
        if not partial:
            assert g[-1] == value, (g, i, value)
    partitions, capacity, held = op.topNRankingStats()
    assert held == len(want)
    if partition:
        assert partitions == len({tuple(canon(types[c], r[c]) for c in partition) for r in rows})
        assert capacity >= 2 * partitions and capacity & (capacity - 1) == 0
    else:
        assert (partitions, capacity) == (1, 0)
    return [(g[at_index], None if partial else g[-1]) for g in got], op


def run_numpy(columns, types, partition, sort, orders, n, ranking=ROW_NUMBER, sizes=None, prune=None, device_input=True, output_mem=abi.MEM_DEVICE,
              expected_positions=0):
    """numpy columns (+ a BIGINT input-position column behind them) -> (positions in output order, ranking column, raw bytes of the output)."""
    total = len(columns[0])
    page_types = list(types) + [abi.BIGINT]
    with prune_rows(prune):
        op = TopNRankingOperator(page_types, [len(types)], partition, sort, orders, n, ranking_type=ranking, output_mem=output_mem,
                                 expected_positions=expected_positions)
    at = 0
    sizes = list(sizes or [total])
    while at < total:
        m = min(sizes.pop(0) if sizes else total - at, total - at)
        page = Page([Block.flat(t, c[at:at + m]) for t, c in zip(types, columns)] + [Block.bigint(np.arange(at, at + m, dtype=np.int64))], m)
        op.addInput(upload_page(page) if device_input else page)
        at += m
    pages = drain(op)
    pos = np.concatenate([p.blocks[0].values[:p.position_count] for p in pages]) if pages else np.zeros(0, np.int64)
    val = np.concatenate([p.blocks[1].values[:p.position_count] for p in pages]) if pages else np.zeros(0, np.int64)
    return pos, val, pos.tobytes() + val.tobytes(), op


# ---- 1. TestTopNRankingOperator ----------------------------------------------------------------------------------------------------------
KAT_TYPES = [abi.VARCHAR, abi.DOUBLE]
KAT_PAGES = [[("a", 0.3), ("b", 0.2), ("c", 0.1), ("c", 0.91)], [("a", 0.4)], [("a", 0.5), ("a", 0.6), ("b", 0.7), ("b", 0.8)], [("b", 0.9)]]
RANK_PAGES = [[("a", None), ("b", 0.2), ("b", NAN), ("c", 0.1), ("c", 0.91)], [("a", 0.4)],
              [("a", 0.5), ("a", None), ("a", 0.6), ("b", 0.7), ("b", NAN)]]


def kat(pages, partition, orders, ranking, partial, hashed, device, output_mem):
    types = KAT_TYPES + ([abi.BIGINT] if hashed else [])
    op = TopNRankingOperator(types, [1, 0], partition, [1], orders, 3, ranking_type=ranking, partial=partial, hash_channel=2 if hashed else -1,
                             expected_positions=10, output_mem=output_mem)
    for rows in pages:
        page = Page([block(abi.VARCHAR, [r[0] for r in rows]), block(abi.DOUBLE, [r[1] for r in rows])] + ([hash_block(len(rows))] if hashed else []),
                    len(rows))
        op.addInput(upload_page(page) if device else page)
    got = [r for p in drain(op) for r in p.to_rows()]
    return [tuple("NaN" if isinstance(v, float) and math.isnan(v) else v for v in r) for r in got]


MODES = [(h, d, m) for h in (False, True) for d in (False, True) for m in (abi.MEM_HOST, abi.MEM_DEVICE)]


@pytest.mark.parametrize("hashed,device,output_mem", MODES)
def test_partitioned_kat(gpu, hashed, device, output_mem):
    """testPartitioned: output channels (1, 0), partition 0, sort 1 ASC_NULLS_LAST, n = 3, four pages."""
    got = kat(KAT_PAGES, [0], [ASC_NULLS_LAST], ROW_NUMBER, False, hashed, device, output_mem)
    assert got == [(0.3, b"a", 1), (0.4, b"a", 2), (0.5, b"a", 3), (0.2, b"b", 1), (0.7, b"b", 2), (0.8, b"b", 3), (0.1, b"c", 1), (0.91, b"c", 2)]


@pytest.mark.parametrize("hashed,device,output_mem", MODES)
def test_unpartitioned_kat(gpu, hashed, device, output_mem):
    """testUnPartitioned, partial and not."""
    assert kat(KAT_PAGES, [], [ASC_NULLS_LAST], ROW_NUMBER, False, hashed, device, output_mem) == [(0.1, b"c", 1), (0.2, b"b", 2), (0.3, b"a", 3)]
    assert kat(KAT_PAGES, [], [ASC_NULLS_LAST], ROW_NUMBER, True, hashed, device, output_mem) == [(0.1, b"c"), (0.2, b"b"), (0.3, b"a")]


@pytest.mark.parametrize("hashed,device,output_mem", MODES)
def test_rank_null_and_nan_kat(gpu, hashed, device, output_mem):
    """testRankNullAndNan: RANK, ASC_NULLS_FIRST, n = 3 -- NULL ties with NULL, NaN with NaN; partition b keeps four rows."""
    got = kat(RANK_PAGES, [0], [ASC_NULLS_FIRST], RANK, False, hashed, device, output_mem)
    assert got == [(None, b"a", 1), (None, b"a", 1), (0.4, b"a", 3), (0.2, b"b", 1), (0.7, b"b", 2), ("NaN", b"b", 3), ("NaN", b"b", 3),
                   (0.1, b"c", 1), (0.91, b"c", 2)]


def test_the_model_reproduces_the_known_answers():
    """(the restatement itself, against the three reference answers: no GPU work)"""
    rows = [r for p in KAT_PAGES for r in p]
    assert [(rows[i][1], rows[i][0], v) for i, v in model(KAT_TYPES, rows, [0], [1], [ASC_NULLS_LAST], 3)] == [
        (0.3, "a", 1), (0.4, "a", 2), (0.5, "a", 3), (0.2, "b", 1), (0.7, "b", 2), (0.8, "b", 3), (0.1, "c", 1), (0.91, "c", 2)]
    assert [(rows[i][1], rows[i][0], v) for i, v in model(KAT_TYPES, rows, [], [1], [ASC_NULLS_LAST], 3)] == [(0.1, "c", 1), (0.2, "b", 2), (0.3, "a", 3)]
    rows = [r for p in RANK_PAGES for r in p]
    got = [(rows[i][0], v) for i, v in model(KAT_TYPES, rows, [0], [1], [ASC_NULLS_FIRST], 3, RANK)]
    assert got == [("a", 1), ("a", 1), ("a", 3), ("b", 1), ("b", 2), ("b", 3), ("b", 3), ("c", 1), ("c", 2)]


# ---- 2. testMemoryReservationYield's shape ---------------------------------------------------------------------------------------------------
def test_every_key_new(gpu):
    """1 000 pages of 500 rows, every key new, n = 3, sort = the key: 500 000 rows out, every row number 1; the table grew from 10."""
    op = TopNRankingOperator([abi.BIGINT], [0], [0], [0], [ASC_NULLS_LAST], 3, expected_positions=10, output_mem=abi.MEM_DEVICE)
    assert op.topNRankingStats()[1] <= 64
    keys = np.random.default_rng(5).permutation(500_000).astype(np.int64)
    for p in range(1000):
        op.addInput(Page([Block.bigint(keys[p * 500:(p + 1) * 500])], 500))
    pages = drain(op)
    got = np.concatenate([p.blocks[0].values[:p.position_count] for p in pages])
    rn = np.concatenate([p.blocks[1].values[:p.position_count] for p in pages])
    assert np.array_equal(got, keys) and np.all(rn == 1)                  # first-seen order
    partitions, capacity, held = op.topNRankingStats()
    assert partitions == held == 500_000 and capacity >= 1_000_000


# ---- 3. independence of cuts and of pruning --------------------------------------------------------------------------------------------------
def big_input(seed=11, total=260_000):
    rng = np.random.default_rng(seed)
    part = rng.integers(0, 3000, total).astype(np.int64)
    part[rng.random(total) < 0.25] = 7_000_000                            # one long partition
    key = rng.integers(0, 40, total).astype(np.int64)                     # many exact ties: the payload shows their order
    return part, key


@pytest.mark.parametrize("ranking", [ROW_NUMBER, RANK])
def test_cuts_and_prunes_do_not_change_the_output(gpu, ranking):
    part, key = big_input()
    total = len(part)
    want_pos, want_val = np_model(part, [key], 5, ranking)
    outputs = []
    cuts = [None, [1024] * (total // 1024 + 1), [1025] * (total // 1025 + 1), [1, 7] * 40 + [total]]
    for sizes in cuts:
        for prune in (1000, None):
            pos, val, raw, op = run_numpy([part, key], [abi.BIGINT, abi.BIGINT], [0], [1], [ASC_NULLS_LAST], 5, ranking, sizes=sizes, prune=prune)
            assert np.array_equal(pos, want_pos) and np.array_equal(val, want_val), (sizes and sizes[0], prune)
            outputs.append(raw)
    pos, val, raw, _ = run_numpy([part, key], [abi.BIGINT, abi.BIGINT], [0], [1], [ASC_NULLS_LAST], 5, ranking, sizes=cuts[1], prune=1000)
    outputs.append(raw)                                                   # the same input twice
    assert len(set(outputs)) == 1


def test_host_pages_and_host_output_give_the_same_bytes(gpu):
    part, key = big_input(12, 60_000)
    a = run_numpy([part, key], [abi.BIGINT, abi.BIGINT], [0], [1], [DESC_NULLS_FIRST], 4, sizes=[4096] * 20, prune=1000)[2]
    b = run_numpy([part, key], [abi.BIGINT, abi.BIGINT], [0], [1], [DESC_NULLS_FIRST], 4, sizes=[5000] * 20, device_input=False, output_mem=abi.MEM_HOST)[2]
    want_pos, want_val = np_model(part, [-key], 4)
    assert a == b == want_pos.tobytes() + want_val.tobytes()


# ---- 4. ties across prunes ---------------------------------------------------------------------------------------------------------------------
def test_ties_at_place_n_across_prunes(gpu):
    """Partition 1's third place is tied by rows that arrive before and after several prunes (threshold 4 rows, pages of 3): ROW_NUMBER
    keeps the earliest arrivals, RANK keeps every one of them."""
    rows = []
    for i in range(60):
        rows.append((1, 5 if i % 3 else 1 + (i % 2)))      # keys 1 and 2 in front, then a long tie at 5
        rows.append((2, i % 4))
    rows = [(1, 5), (1, 5)] + rows
    for ranking in (ROW_NUMBER, RANK):
        for prune in (4, None):
            got, _ = run_rows([abi.BIGINT, abi.BIGINT], rows, [0], [1], [ASC_NULLS_LAST], 3, ranking, sizes=[3] * 50, prune=prune)
            assert got == model([abi.BIGINT, abi.BIGINT], rows, [0], [1], [ASC_NULLS_LAST], 3, ranking)
    tie = [(7, 9)] * 40
    got, _ = run_rows([abi.BIGINT, abi.BIGINT], tie, [0], [1], [ASC_NULLS_LAST], 3, ROW_NUMBER, sizes=[3] * 20, prune=4)
    assert got == [(0, 1), (1, 2), (2, 3)]                  # the earliest arrivals
    got, _ = run_rows([abi.BIGINT, abi.BIGINT], tie, [0], [1], [ASC_NULLS_LAST], 3, RANK, sizes=[3] * 20, prune=4)
    assert got == [(i, 1) for i in range(40)]               # all peers


def test_the_second_sort_channel_decides_a_tie_on_the_first(gpu):
    """Once partition 0 holds n rows with first key 5, every later row ties the bound on the first channel: the arrival filter must let
    them through to the exact comparison, where the second channel (descending) puts them in front."""
    rows = [(0, 5, v) for v in range(20)] + [(0, 4, 0)] + [(0, 5, 100 + v) for v in range(20)] + [(0, 6, 1000)]
    types = [abi.BIGINT, abi.BIGINT, abi.BIGINT]
    for ranking in (ROW_NUMBER, RANK):
        got, _ = run_rows(types, rows, [0], [1, 2], [ASC_NULLS_LAST, DESC_NULLS_LAST], 4, ranking, sizes=[5] * 10, prune=6)
        assert [i for i, _ in got] == [20, 40, 39, 38]


def test_varchar_images_are_not_injective(gpu):
    """A VARCHAR first sort channel whose strings share their first 8 bytes: the difference is behind byte 8, or in the length only."""
    words = ["prefix__b", "prefix__a", "prefix__", "prefix__aa", "prefix__a\x00", "prefix_", "prefix__b", "prefix__\xff", "prefix__a"]
    rows = [(i % 2, words[i % len(words)]) for i in range(90)]
    for orders in ([ASC_NULLS_LAST], [DESC_NULLS_FIRST]):
        for ranking in (ROW_NUMBER, RANK):
            run_rows([abi.BIGINT, abi.VARCHAR], rows, [0], [1], orders, 4, ranking, sizes=[7] * 20, prune=10)


# ---- 5. edges ------------------------------------------------------------------------------------------------------------------------------------
NANS = [NAN, struct.unpack("<d", struct.pack("<Q", 0xFFF8000000000001))[0], struct.unpack("<d", struct.pack("<Q", 0x7FF0000000000001))[0]]


@pytest.mark.parametrize("order", [0, 1, 2, 3])
def test_nulls_in_partition_and_sort_channels(gpu, order):
    rows = [(None if i % 3 == 0 else i % 2, None if i % 5 < 2 else (i * 7) % 6, None if i % 7 == 0 else "s%d" % (i % 4)) for i in range(120)]
    types = [abi.BIGINT, abi.INTEGER, abi.VARCHAR]
    for ranking in (ROW_NUMBER, RANK):
        run_rows(types, rows, [0], [1], [order], 3, ranking, sizes=[11] * 20, prune=16)
        run_rows(types, rows, [0], [2, 1], [order, 3 - order], 5, ranking, sizes=[13] * 20, prune=16, device_input=True)
        run_rows(types, rows, [], [1, 2], [order, order], 7, ranking, sizes=[17] * 20, prune=16)


@pytest.mark.parametrize("t", [abi.DOUBLE, abi.REAL])
@pytest.mark.parametrize("order", [0, 1, 2, 3])
def test_float_sort_channels(gpu, t, order):
    """Double.compare / Float.compare order: NaN (several bit patterns) largest and equal to itself, -0.0 before +0.0, infinities."""
    values = [0.0, -0.0, 1.5, -1.5, math.inf, -math.inf, None, 1e-300 if t == abi.DOUBLE else 1e-30, 3.0] + NANS
    rows = [(i % 3, values[(i * 5) % len(values)]) for i in range(150)]
    run_rows([abi.BIGINT, t], rows, [0], [1], [order], 6, ROW_NUMBER, sizes=[9] * 30, prune=12)
    run_rows([abi.BIGINT, t], rows, [0], [1], [order], 50, ROW_NUMBER, sizes=[9] * 30, prune=12, device_input=True, output_mem=abi.MEM_DEVICE)
    # RANK: NaN and NULL peers; -0.0 stays out of the sort channel (include/presto_amd.h: the one deviation from the reference)
    rank_rows = [(g, None if v is None else (0.0 if v == 0 else v)) for g, v in rows]
    run_rows([abi.BIGINT, t], rank_rows, [0], [1], [order], 6, RANK, sizes=[9] * 30, prune=12)
    run_rows([abi.BIGINT, t], rank_rows, [], [1], [order], 4, RANK, sizes=[9] * 30, prune=12)


def test_booleans_integer_extremes_and_strings(gpu):
    rows = [(i % 2, [0, 1, 2, 255, None][i % 5], [-2**63, 2**63 - 1, 0, -1, None][i % 5], ["", "x" * 100, "x" * 99 + "y", "x", None][(i * 3) % 5])
            for i in range(100)]
    types = [abi.BIGINT, abi.BOOLEAN, abi.BIGINT, abi.VARCHAR]
    for ranking in (ROW_NUMBER, RANK):
        for order in (ASC_NULLS_FIRST, DESC_NULLS_LAST):
            run_rows(types, rows, [0], [1], [order], 30, ranking, sizes=[8] * 20, prune=10)
            run_rows(types, rows, [0], [2], [order], 3, ranking, sizes=[8] * 20, prune=10)
            run_rows(types, rows, [1], [3, 2], [order, order], 3, ranking, sizes=[8] * 20, prune=10)      # a BOOLEAN partition key: 2 -> true


def test_two_to_eight_partition_channels(gpu):
    types = [abi.BIGINT, abi.INTEGER, abi.DATE, abi.DOUBLE, abi.REAL, abi.BOOLEAN, abi.VARCHAR, abi.BIGINT, abi.BIGINT]
    rng = np.random.default_rng(8)
    rows = []
    for _ in range(400):
        v = [int(x) for x in rng.integers(0, 2, 8)]
        rows.append((v[0], v[1], v[2], [0.0, -0.0][v[3]], [1.5, NAN][v[4]], [0, 7][v[5]], ["a", None][v[6]], v[7], int(rng.integers(0, 5))))
    for k in range(2, 9):
        run_rows(types, rows, list(range(k)), [8], [ASC_NULLS_LAST], 2, sizes=[37] * 20, prune=50)
    run_rows(types, rows, list(range(8)), [8], [DESC_NULLS_LAST], 2, RANK, sizes=[37] * 20, prune=50, device_input=True)


def test_one_to_four_sort_channels_of_mixed_types_and_orders(gpu):
    rng = np.random.default_rng(9)
    types = [abi.BIGINT, abi.VARCHAR, abi.DOUBLE, abi.DATE, abi.BOOLEAN]
    rows = [(int(rng.integers(0, 4)), ["b", "a", "ab", None][int(rng.integers(0, 4))], [0.5, -0.0, 0.0, None, NAN][int(rng.integers(0, 5))],
             int(rng.integers(-2, 2)), int(rng.integers(0, 2))) for _ in range(500)]
    for k in range(1, 5):
        sort = [1, 2, 3, 4][:k]
        orders = [DESC_NULLS_FIRST, ASC_NULLS_LAST, DESC_NULLS_LAST, ASC_NULLS_FIRST][:k]
        run_rows(types, rows, [0], sort, orders, 6, ROW_NUMBER, sizes=[41] * 20, prune=60)
    # a sort channel that is also the partition channel
    run_rows(types, rows, [0], [0, 3], [ASC_NULLS_LAST, DESC_NULLS_LAST], 5, RANK, sizes=[41] * 20, prune=60)
    run_rows(types, rows, [3], [3, 1], [ASC_NULLS_LAST, DESC_NULLS_LAST], 5, ROW_NUMBER, sizes=[41] * 20, prune=60)


@pytest.mark.parametrize("n", [1, 2, 1000, 2**31 - 1])
def test_n_values(gpu, n):
    rows = [(i % 5, (i * 13) % 17) for i in range(300)]
    for ranking in (ROW_NUMBER, RANK):
        got, _ = run_rows([abi.BIGINT, abi.BIGINT], rows, [0], [1], [ASC_NULLS_LAST], n, ranking, sizes=[32] * 10, prune=50)
        if n >= 1000:
            assert len(got) == len(rows)                    # n larger than any partition keeps everything
    run_rows([abi.BIGINT, abi.BIGINT], rows, [0], [1], [ASC_NULLS_LAST], n, partial=True, sizes=[32] * 10)
    run_rows([abi.BIGINT, abi.BIGINT], rows, [0], [1], [ASC_NULLS_LAST], n, output_channels=[2, 0], sizes=[32] * 10)


def test_dictionary_and_rle_blocks(gpu):
    """dictionary and RLE blocks in partition, sort and output channels, from host and from device pages"""
    part = Block.dictionary_block(Block.flat(abi.BIGINT, [5, 4, 0], [0, 0, 1]), [0, 1, 2, 2, 0, 1, 0, 0])
    key = Block.dictionary_block(Block.varchar(["x", "yy", None]), [1, 1, 2, 0, 2, 0, 0, 1])
    rle = Block.rle(Block.double([2.5]), 8)
    types = [abi.BIGINT, abi.VARCHAR, abi.DOUBLE]
    rows = list(zip(part.to_pylist(), key.to_pylist(), rle.to_pylist()))
    for ranking in (ROW_NUMBER, RANK):
        for partition, sort in (([0], [1]), ([1], [0]), ([2], [1, 0]), ([0], [2])):
            for device in (False, True):
                op = TopNRankingOperator(types + [abi.BIGINT], [0, 1, 2, 3], partition, sort, [ASC_NULLS_FIRST] * len(sort), 2, ranking_type=ranking)
                all_rows = []
                for rep in range(3):
                    page = Page([part, key, rle, Block.bigint(list(range(8 * rep, 8 * rep + 8)))], 8)
                    op.addInput(upload_page(page) if device else page)
                    all_rows += rows
                got = [r for p in drain(op) for r in p.to_rows()]
                want = model(types, all_rows, partition, sort, [ASC_NULLS_FIRST] * len(sort), 2, ranking)
                assert [(g[3], g[4]) for g in got] == want
                for g, (i, _) in zip(got, want):
                    assert all(same_value(t, v, w) for t, v, w in zip(types, g, all_rows[i]))


def test_short_decimal_partition_and_output_channels(gpu):
    rows = [((i * 3) % 4, i % 7) for i in range(50)]
    op = TopNRankingOperator([abi.decimal(12, 2), abi.BIGINT], [0, 1], [0], [1], [DESC_NULLS_LAST], 2)
    op.addInput(Page([Block.decimal([r[0] for r in rows]), Block.bigint([r[1] for r in rows])], len(rows)))
    got = [r for p in drain(op) for r in p.to_rows()]
    want = model([abi.BIGINT, abi.BIGINT], rows, [0], [1], [DESC_NULLS_LAST], 2)
    assert [(int(g[0]), g[1], g[2]) for g in got] == [(rows[i][0], rows[i][1], v) for i, v in want]


# ---- 6. the state machine ----------------------------------------------------------------------------------------------------------------------
def test_state_machine(gpu):
    for partition in ([0], []):
        op = TopNRankingOperator([abi.BIGINT], [0], partition, [0], [ASC_NULLS_LAST], 2)
        assert op.needsInput() and not op.isFinished() and op.getOutput() is None
        empty = Page([Block.bigint([])], 0)
        check(lib().pa_op_add_input(op._h, C.byref(empty.to_c()[0])))                              # a page of zero rows: nothing
        page = Page([Block.bigint([3, 1, 2])], 3)
        op.addInput(page)
        assert op.needsInput() and not op.isFinished() and op.getOutput() is None                 # no output before finish
        op.addInput(upload_page(page))
        assert op.topNRankingStats()[2] == 6
        op.finish()
        assert not op.needsInput() and not op.isFinished()
        assert lib().pa_op_add_input(op._h, C.byref(page.to_c()[0])) == abi.ERR_ILLEGAL_STATE
        out = op.getOutput()
        want = [(3, 1), (3, 2), (1, 1), (1, 2), (2, 1), (2, 2)] if partition else [(1, 1), (1, 2)]     # partitions in first-seen order
        assert out.to_rows() == want
        assert op.isFinished() and op.getOutput() is None and not op.needsInput()
        assert lib().pa_op_add_input(op._h, C.byref(page.to_c()[0])) == abi.ERR_ILLEGAL_STATE
        assert op.kernelName() == "k_topn_ranking_filter"
        ms, launches = op.kernelTime()
        assert launches == 2 and ms > 0
        op.close()
    # an operator that saw no rows finishes without a page
    op = TopNRankingOperator([abi.BIGINT], [0], [0], [0], [ASC_NULLS_LAST], 2)
    check(lib().pa_op_add_input(op._h, C.byref(Page([Block.bigint([])], 0).to_c()[0])))
    op.finish()
    assert op.isFinished() and op.getOutput() is None and op.isFinished()
    # close with rows held
    op = TopNRankingOperator([abi.BIGINT, abi.VARCHAR], [0, 1], [0], [1], [ASC_NULLS_LAST], 2)
    op.addInput(Page([Block.bigint([1, 2, 3]), Block.varchar(["a", "b", None])], 3))
    assert op.topNRankingStats()[2] == 3 and op.memoryBytes() > 0
    op.close()
    # stats of a foreign operator
    a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
    agg = HashAggregationOperator([abi.BIGINT], [0], [(abi.AGG_COUNT_STAR, -1, None)])
    assert lib().pa_topn_ranking_stats(agg._h, C.byref(a), C.byref(b), C.byref(c)) == abi.ERR_INVALID_ARGUMENT
    op = TopNRankingOperator([abi.BIGINT], [0], [0], [0], [ASC_NULLS_LAST], 2)
    assert lib().pa_row_number_stats(op._h, C.byref(a), C.byref(b)) == abi.ERR_INVALID_ARGUMENT


def test_retained_pages_are_released_exactly_once(gpu):
    """A PA_PAGE_RETAINED page is handed back once the call that read it has drained -- its release scribbles over the buffers, so a
    later read of them would show in the result -- and exactly once."""
    from tests.test_gpu_small_pages import retained_pages
    total = 40_000
    part = (np.arange(total, dtype=np.int64) * 31) % 977
    key = (np.arange(total, dtype=np.int64) * 17) % 101
    host = Page([Block.bigint(part), Block.bigint(key), Block.bigint(np.arange(total, dtype=np.int64))], total)
    bounds = [0, 7000, 7001, 20_000, total]
    want_pos, want_val = np_model(part, [key], 3)
    for prune in (1000, None):
        released = []
        pages = retained_pages(host, bounds, released)
        with prune_rows(prune):
            op = TopNRankingOperator([abi.BIGINT] * 3, [2], [0], [1], [ASC_NULLS_LAST], 3, output_mem=abi.MEM_DEVICE)
        for i, p in enumerate(pages):
            op.addInput(p)
            assert released == list(range(i + 1))
        out = drain(op)
        assert np.array_equal(np.concatenate([p.blocks[0].values for p in out]), want_pos)
        assert np.array_equal(np.concatenate([p.blocks[1].values for p in out]), want_val)
        op.close()
        assert released == list(range(len(pages)))


# ---- 7. bounded state --------------------------------------------------------------------------------------------------------------------------
def test_state_is_bounded_by_what_can_still_matter(gpu):
    """64 pages of 2^20 rows over 1 000 partitions, n = 10, random sort keys, under a memory limit that holding every row could not meet."""
    L = lib()
    pages, page_rows, partitions, n = 64, 1 << 20, 1000, 10
    threshold = DEFAULT_PRUNE_ROWS
    # What the operator may hold at once: rows retained by the last prune (<= n per partition) + the prune threshold + one page.  Per
    # held row, at a prune: the held columns (BIGINT + DOUBLE + the group id = 24 B, arrays grow by doubling: 48), their fresh copies
    # (24), the sort's permutations, images, pairs and scratch, the sorted ids, rankings, flags and positions (<= 184): 256 B; on top
    # the table (1 000 keys), a page of staging and per-page scratch (2^20 rows x 64 B).
    bound_rows = n * partitions + threshold + page_rows
    limit = bound_rows * 256 + page_rows * 64
    hold_everything = pages * page_rows * 24                         # (the bare columns of every row, nothing to sort them with)
    assert limit < hold_everything
    rng = np.random.default_rng(77)
    with prune_rows(None):
        op = TopNRankingOperator([abi.BIGINT, abi.DOUBLE], [0, 1], [0], [1], [ASC_NULLS_LAST], n, output_mem=abi.MEM_DEVICE)
    cand_part, cand_key = np.zeros(0, np.int64), np.zeros(0, np.float64)
    retained, last_held, peak_memory, first_seen = 0, 0, 0, None
    L.pa_memory_set_limit(limit)
    try:
        for _ in range(pages):
            part = rng.integers(0, partitions, page_rows).astype(np.int64)
            key = rng.random(page_rows)
            if first_seen is None:
                _, first = np.unique(part, return_index=True)
                first_seen = part[np.sort(first)]
                assert len(first_seen) == partitions                  # (every partition shows up in the first page)
            page = upload_page(Page([Block.bigint(part), Block.double(key)], page_rows))
            op.addInput(page)
            del page
            held = op.topNRankingStats()[2]
            if held < last_held:                                      # a prune ran inside this call
                retained = held
            assert held <= retained + max(threshold, retained) + page_rows
            last_held = held
            peak_memory = max(peak_memory, op.memoryBytes())
            # the restatement, streaming: the n smallest keys per partition so far
            cand_part, cand_key = np.concatenate([cand_part, part]), np.concatenate([cand_key, key])
            order = np.lexsort((cand_key, cand_part))
            cand_part, cand_key = cand_part[order], cand_key[order]
            head = np.r_[True, cand_part[1:] != cand_part[:-1]]
            at = np.arange(len(cand_part))
            keep = at - np.maximum.accumulate(np.where(head, at, 0)) < n
            cand_part, cand_key = cand_part[keep], cand_key[keep]
        out = drain(op)
    finally:
        L.pa_memory_set_limit(0)
    assert op.topNRankingStats() == (partitions, op.topNRankingStats()[1], n * partitions)
    end_memory = op.memoryBytes()
    assert end_memory < peak_memory and end_memory * 8 < pages * page_rows * 16
    got_part = np.concatenate([p.blocks[0].values for p in out])
    got_key = np.concatenate([p.blocks[1].values for p in out])
    got_rn = np.concatenate([p.blocks[2].values for p in out])
    # partitions in first-seen order, keys ascending inside, numbered 1 .. n
    assert np.array_equal(got_part, np.repeat(first_seen, n))
    assert np.array_equal(got_rn, np.tile(np.arange(1, n + 1), partitions))
    position = {int(p): i for i, p in enumerate(first_seen)}
    want_key = np.empty(n * partitions)
    for p in range(partitions):
        want_key[position[p] * n:(position[p] + 1) * n] = cand_key[cand_part == p]
    assert np.array_equal(got_key, want_key)


def test_memory_limit_applies_to_growth(gpu):
    L = lib()
    op = TopNRankingOperator([abi.BIGINT], [0], [0], [0], [ASC_NULLS_LAST], 3, expected_positions=1)
    op.addInput(Page([Block.bigint([1, 2, 3])], 3))
    rows = 1 << 22
    page = upload_page(Page([Block.bigint(np.arange(rows, dtype=np.int64))], rows))
    cpage, _keep = page.to_c()
    L.pa_memory_set_limit(32 << 20)             # the table for 4 Mi more keys alone is 64 MiB
    try:
        assert L.pa_op_add_input(op._h, C.byref(cpage)) == abi.ERR_INSUFFICIENT_RESOURCES
    finally:
        L.pa_memory_set_limit(0)
    op.close()


# ---- 8. cross-checks against operators that exist ------------------------------------------------------------------------------------------------
def cross_input(seed, ties=True):
    rng = np.random.default_rng(seed)
    total = 120_000
    part = rng.integers(0, 2500, total).astype(np.int64)
    key = rng.integers(0, 50, total).astype(np.float64) * 0.5 if ties else rng.permutation(total).astype(np.float64)
    return part, key, np.arange(total, dtype=np.int64)


def columns_of(pages):
    return [np.concatenate([p.blocks[c].values[:p.position_count] for p in pages]) for c in range(len(pages[0].blocks))]


def test_order_by_then_row_number_gives_the_same_rows(gpu):
    """(a) OrderBy by (partition, sort key) on the whole input, then RowNumber partitioned by the key with cap n: the same rows and
    numbers, as sets per partition and in order inside each."""
    part, key, pos = cross_input(50)
    types = [abi.BIGINT, abi.DOUBLE, abi.BIGINT]
    page = Page([Block.bigint(part), Block.double(key), Block.bigint(pos)], len(part))
    order_by = OrderByOperator(types, [0, 1, 2], [0, 1], [ASC_NULLS_LAST, DESC_NULLS_LAST])
    row_number = RowNumberOperator(types, [0, 1, 2], [0], 7)
    composed = columns_of([p for s in to_pages(order_by, [page]) for p in to_pages(row_number, [s])])
    got = run_numpy([part, key], [abi.BIGINT, abi.DOUBLE], [0], [1], [DESC_NULLS_LAST], 7, sizes=[30_000] * 4, prune=20_000)
    # the composition emits partitions in key order, the operator in first-seen order: regroup by partition, keep the order inside
    by_partition = np.argsort(part[got[0]], kind="stable")
    assert np.array_equal(got[0][by_partition], composed[2]) and np.array_equal(got[1][by_partition], composed[3])


def test_without_partition_channels_it_is_topn(gpu):
    """(b) no partition channels: the rows of TopNOperator(n) in its order, numbered 1 .. n."""
    part, key, pos = cross_input(51)
    types = [abi.BIGINT, abi.DOUBLE, abi.BIGINT]
    page = Page([Block.bigint(part), Block.double(key), Block.bigint(pos)], len(part))
    topn = columns_of(to_pages(TopNOperator(types, 100, [1, 0], [ASC_NULLS_LAST, DESC_NULLS_LAST]), [page]))
    op = TopNRankingOperator(types, [2], [], [1, 0], [ASC_NULLS_LAST, DESC_NULLS_LAST], 100)
    op.addInput(page)
    got = columns_of(drain(op))
    assert np.array_equal(got[0], topn[2]) and np.array_equal(got[1], np.arange(1, 101))


def test_a_constant_sort_key_is_row_number_with_a_cap(gpu):
    """(c) with the sort key constant, ROW_NUMBER = RowNumberOperator with cap n (arrival order), regrouped by partition."""
    part, _, pos = cross_input(52)
    types = [abi.BIGINT, abi.BIGINT, abi.BIGINT]
    pages = [Page([Block.bigint(part[a:a + 40_000]), Block.bigint(np.full(40_000, 3)), Block.bigint(pos[a:a + 40_000])], 40_000) for a in (0, 40_000, 80_000)]
    capped = columns_of(to_pages(RowNumberOperator(types, [0, 2], [0], 4), pages))
    got = run_numpy([part, np.full(len(part), 3, np.int64)], [abi.BIGINT, abi.BIGINT], [0], [1], [ASC_NULLS_FIRST], 4, sizes=[40_000] * 3, prune=30_000)
    _, first = np.unique(part, return_index=True)
    seen_rank = {int(p): i for i, p in enumerate(part[np.sort(first)])}
    regroup = np.argsort(np.array([seen_rank[int(p)] for p in capped[0]]), kind="stable")
    assert np.array_equal(got[0], capped[1][regroup]) and np.array_equal(got[1], capped[2][regroup])


def test_rank_without_ties_is_row_number(gpu):
    """(d)"""
    part, key, _ = cross_input(53, ties=False)
    a = run_numpy([part, key], [abi.BIGINT, abi.DOUBLE], [0], [1], [ASC_NULLS_LAST], 5, ROW_NUMBER, sizes=[50_000] * 3, prune=25_000)[2]
    b = run_numpy([part, key], [abi.BIGINT, abi.DOUBLE], [0], [1], [ASC_NULLS_LAST], 5, RANK, sizes=[33_333] * 4)[2]
    assert a == b


# ---- 9. seeded fuzz ------------------------------------------------------------------------------------------------------------------------------
FUZZ_SEEDS = int(os.environ.get("PA_FUZZ_SEEDS", "16"))
FUZZ_TYPES = [abi.BIGINT, abi.INTEGER, abi.DATE, abi.DOUBLE, abi.REAL, abi.BOOLEAN, abi.VARCHAR]


def _fuzz_column(rng, t, n, domain, null_rate, zeros):
    out = []
    for v in rng.integers(-domain, domain, n):
        v = int(v)
        if rng.random() < null_rate:
            out.append(None)
        elif t in (abi.DOUBLE, abi.REAL):
            r = rng.random()
            out.append(NAN if r < 0.05 else (-0.0 if r < 0.1 and zeros else float(v) / 4))
        elif t == abi.BOOLEAN:
            out.append(v & 0xFF)
        elif t == abi.VARCHAR:
            out.append(("k%d" % v) * (1 + abs(v) % 5))
        else:
            out.append(v)
    return out


@pytest.mark.parametrize("seed", range(FUZZ_SEEDS))
def test_fuzz_topn_ranking(gpu, seed):
    rng = np.random.default_rng(9000 + seed)
    nt = int(rng.integers(1, 6))
    types = [FUZZ_TYPES[int(rng.integers(0, len(FUZZ_TYPES)))] for _ in range(nt)]
    total = int(rng.integers(1, 6000))
    ranking = RANK if rng.integers(0, 2) else ROW_NUMBER
    domain = int(rng.choice([1, 2, 30, 1000, 1 << 30]))     # from one value to all-distinct
    cols = [_fuzz_column(rng, t, total, domain if t != abi.VARCHAR else min(domain, 1 << 20), float(rng.choice([0.0, 0.02, 0.4])), ranking == ROW_NUMBER)
            for t in types]
    rows = list(zip(*cols))
    sizes = [int(s) for s in rng.integers(1, max(2, total // 2), int(rng.integers(1, 8)))]
    partition = [int(c) for c in rng.permutation(nt)[:int(rng.integers(0, min(nt, 4) + 1))]]
    sort = [int(c) for c in rng.permutation(nt)[:int(rng.integers(1, min(nt, 3) + 1))]]
    orders = [int(o) for o in rng.integers(0, 4, len(sort))]
    run_rows(types, rows, partition, sort, orders, [1, 3, 50, 10**9][int(rng.integers(0, 4))], ranking, partial=bool(rng.integers(0, 2)), sizes=sizes,
             hashed=bool(rng.integers(0, 2)), output_mem=int(rng.integers(0, 2)), device_input=bool(rng.integers(0, 2)),
             expected_positions=int(rng.choice([0, 1, 100])), prune=[None, 1, 50, 700][int(rng.integers(0, 4))])


# ---- 10. a scrubbed pool, in a child process; the C++ mirror -----------------------------------------------------------------------------------------
def test_on_a_scrubbed_pool(gpu):
    """The picks that matter once more with every recycled HBM block overwritten before it is handed out (PRESTO_AMD_POOL_SCRUB,
    pool.cpp): bounds, run starts or held columns that relied on what a block's previous owner left behind fail here."""
    env = dict(os.environ, PRESTO_AMD_POOL_SCRUB="0xA5", PA_FUZZ_SEEDS="4")
    picks = ["test_cuts_and_prunes_do_not_change_the_output", "test_ties_at_place_n_across_prunes", "test_fuzz_topn_ranking",
             "test_two_to_eight_partition_channels", "test_varchar_images_are_not_injective", "test_nulls_in_partition_and_sort_channels",
             "test_rank_null_and_nan_kat"]
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider", "tests/test_gpu_topn_ranking.py", "-k",
                        " or ".join(picks)], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    tail = r.stdout.decode()[-3000:]
    assert r.returncode == 0, tail
    assert " passed" in tail and "failed" not in tail


def test_cpp_mirror(gpu):
    """tests/cpp/test_topn_ranking.cpp: the operator through the C++ host mirror's runDriver."""
    exe = os.path.join(ROOT, "tests", "cpp", "test_topn_ranking")
    src = exe + ".cpp"
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-L" + os.path.join(ROOT, "presto_amd"),
                               "-lpresto_amd", "-Wl,-rpath,$ORIGIN/../../presto_amd", "-Wl,--allow-shlib-undefined", "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode == 0, r.stdout.decode()[-2000:]
    assert "topn ranking ok" in r.stdout.decode()
