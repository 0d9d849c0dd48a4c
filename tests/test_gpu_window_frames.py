"""GPU checks of WindowOperator through the framed descriptor (pa_framed_window_create): count(*) / count / sum / min / max over the frames
UNBOUNDED PRECEDING .. CURRENT ROW (ROWS; RANGE = GROUPS) and UNBOUNDED PRECEDING .. UNBOUNDED FOLLOWING, next to the ranking functions.
Order, partitions, peers and the ranking functions are the restatement of tests/test_gpu_window.py, imported; this file adds only the
sequential aggregate rules of include/presto_amd.h (`running`).  Every comparison is exact: integers by value, DOUBLE / REAL by their
bits with any NaN equal to any NaN.  Known answers by hand, the ranking columns bit for bit against WindowOperator, identities that need
no model, the tile boundaries of the scans, segment hygiene, every argument type, sum overflow, page cuts, the state machine, fuzz, the
C++ mirror."""
import ctypes as C
import math
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from presto_amd import abi
from presto_amd._lib import lib
from presto_amd.operators import FramedWindowOperator, WindowOperator, upload_page
from presto_amd.page import Block, Page
from tests.test_gpu_window import (ASC_NULLS_FIRST, ASC_NULLS_LAST, DESC_NULLS_FIRST, DESC_NULLS_LAST, CUME_DIST, DENSE_RANK, MODES, NAN, NTILE,
                                   PERCENT_RANK, RANK, ROW_NUMBER, block, drain, model, np_model, order_value, same_value, split)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNT_STAR, COUNT, SUM, MIN, MAX = abi.WINDOW_COUNT_STAR, abi.WINDOW_COUNT, abi.WINDOW_SUM, abi.WINDOW_MIN, abi.WINDOW_MAX
UP, CR, UF = abi.BOUND_UNBOUNDED_PRECEDING, abi.BOUND_CURRENT_ROW, abi.BOUND_UNBOUNDED_FOLLOWING
ROWS, RANGE, GROUPS, WHOLE = (abi.FRAME_ROWS, UP, CR), (abi.FRAME_RANGE, UP, CR), (abi.FRAME_GROUPS, UP, CR), (abi.FRAME_ROWS, UP, UF)
FRAMES = [ROWS, RANGE, GROUPS, WHOLE, (abi.FRAME_RANGE, UP, UF), (abi.FRAME_GROUPS, UP, UF)]
INT64_MAX, INT64_MIN = (1 << 63) - 1, -(1 << 63)
# rows of one workgroup of the aggregate scans, as the kernel header states it
T = int(re.search(r"kWindowScanTile\s*=\s*(\d+)", open(os.path.join(ROOT, "presto_amd", "csrc", "window_kernels.hpp")).read()).group(1))
RANKING = [ROW_NUMBER, RANK, DENSE_RANK, PERCENT_RANK, CUME_DIST]
MIN_MAX_TYPES = [abi.BIGINT, abi.INTEGER, abi.DATE, abi.BOOLEAN, abi.decimal(12, 2), abi.DOUBLE, abi.REAL]


# ---- the contract of the aggregates, restated -----------------------------------------------------------------------------------------
def framed(functions):
    """-> [(id, [argument channels], (frame_type, start_type, end_type))]; no frame = the SQL default"""
    out = []
    for f in functions:
        f = (f, []) if isinstance(f, int) else tuple(f)
        out.append((f[0], list(f[1]), tuple(f[2]) if len(f) > 2 else RANGE))
    return out


def frame_end(frame, place, pe, size):
    """the last place of the frame 0 .. e"""
    if frame[2] == UF:
        return size - 1
    return place if frame[0] == abi.FRAME_ROWS else pe - 1


class SumOverflow(Exception):
    pass


def better(t, function, value, held):
    """MinMaxCompare: min by the type's comparison (Double.compare order); max over DOUBLE / REAL: value > held || isNaN(held)"""
    if function == MIN:
        return order_value(t, value) < order_value(t, held)
    if t in (abi.DOUBLE, abi.REAL):
        v, h = (float(np.float32(value)), float(np.float32(held))) if t == abi.REAL else (float(value), float(held))
        return v > h or math.isnan(h)
    return order_value(t, value) > order_value(t, held)


def running(t, function, values):
    """The state of count / sum / min / max after each of `values` (one partition in sorted order): the aggregates are sequential."""
    out, count, held = [], 0, None
    for v in values:
        if v is not None:
            count += 1
            if function == SUM:
                held = int(v) if held is None else held + int(v)
                if not INT64_MIN <= held <= INT64_MAX:          # Math.addExact
                    raise SumOverflow()
            elif function in (MIN, MAX) and (held is None or better(t, function, v, held)):
                held = v
        out.append(count if function == COUNT else held)
    return out


def frame_model(types, rows, partition, sort, orders, functions):
    """-> [(input position, [one value per function])] in output order.  Partitions and peer groups are read off the imported model's
    row_number and rank columns."""
    fs = framed(functions)
    base = model(types, rows, partition, sort, orders, [ROW_NUMBER, RANK] + [(f, a) for f, a, _ in fs if f <= NTILE])
    out, at, total = [], 0, len(base)
    while at < total:
        end = at + 1
        while end < total and base[end][1][0] != 1:
            end += 1
        members = base[at:end]
        size = end - at
        ranks = [v[1] for _, v in members]
        states = {(f, a[0]): running(types[a[0]], f, [rows[i][a[0]] for i, _ in members]) for f, a, _ in fs if f in (COUNT, SUM, MIN, MAX)}
        ends = [size] * size                                  # where the peer group of each place ends: the rows of its rank
        for place in range(size - 2, -1, -1):
            ends[place] = ends[place + 1] if ranks[place] == ranks[place + 1] else place + 1
        for place, (i, values) in enumerate(members):
            pe = ends[place]
            ranking = iter(values[2:])
            result = []
            for f, a, frame in fs:
                e = frame_end(frame, place, pe, size)
                result.append(next(ranking) if f <= NTILE else e + 1 if f == COUNT_STAR else states[(f, a[0])][e])
            out.append((i, result))
        at = end
    return out


def result_type(types, f, args):
    return types[args[0]] if f in (MIN, MAX) else abi.DOUBLE if f in (PERCENT_RANK, CUME_DIST) else abi.BIGINT


def float_bits(t, v):
    return struct.unpack("<I", struct.pack("<f", v))[0] if t == abi.REAL else struct.unpack("<Q", struct.pack("<d", v))[0]


def same_out(t, got, want):
    """a function's value: NULL, an integer by value, a DOUBLE / REAL by its bits (any NaN is any NaN), a BOOLEAN as true / false"""
    if got is None or want is None:
        return got is None and want is None
    if t in (abi.DOUBLE, abi.REAL):
        g, w = float(got), float(np.float32(want)) if t == abi.REAL else float(want)
        return isinstance(got, float) and ((math.isnan(g) and math.isnan(w)) or float_bits(t, g) == float_bits(t, w))
    if t == abi.BOOLEAN:
        return bool(got) == bool(want)
    return not isinstance(got, float) and int(got) == int(want)


# ---- driving the operator ---------------------------------------------------------------------------------------------------------------
def typed_block(t, values):
    if t == abi.LONG_DECIMAL:
        return Block.long_decimal(values)
    return block(t, values)


def feed_typed(op, types, rows, sizes=None, device_input=False):
    """test_gpu_window.feed with long decimal blocks: rows as pages of (types..., BIGINT row index) cut by `sizes` (0 = an empty page)"""
    at = 0
    for chunk in split(rows, sizes or [len(rows)]):
        m = len(chunk)
        page = Page([typed_block(t, [r[c] for r in chunk]) for c, t in enumerate(types)] + [Block.bigint(list(range(at, at + m)))], m)
        op.addInput(upload_page(page) if device_input else page)
        at += m


def run_framed(types, rows, partition, sort, orders, functions, sizes=None, output_mem=abi.MEM_HOST, device_input=False, output_channels=None, want=None):
    """rows through a FramedWindowOperator over (types..., BIGINT row index) pages; the output is compared with frame_model: which row
    stands where, every output channel value, every function value.  Returns the output rows."""
    nt = len(types)
    out_ch = list(range(nt + 1)) if output_channels is None else list(output_channels)
    assert nt in out_ch
    op = FramedWindowOperator(list(types) + [abi.BIGINT], out_ch, functions, partition, sort, orders, output_mem=output_mem)
    feed_typed(op, types, rows, sizes, device_input)
    want = frame_model(types, rows, partition, sort, orders, functions) if want is None else want
    pages = drain(op)
    op.close()
    got = [r for p in pages for r in p.to_rows()]
    assert len(got) == len(want)
    at_index = out_ch.index(nt)
    fs = framed(functions)
    for g, (i, values) in zip(got, want):
        assert len(g) == len(out_ch) + len(values)
        assert g[at_index] == i, (g, i, values)
        for c, v in zip(out_ch, g):
            if c < nt:
                assert same_value(types[c], v, rows[i][c]), (i, c, v, rows[i][c])
        for (f, a, _), v, w in zip(fs, g[len(out_ch):], values):
            assert same_out(result_type(types, f, a), v, w), (g, i, f, values)
    return got


# ---- 1. known answers by hand -------------------------------------------------------------------------------------------------------------
KAT_TYPES = [abi.BIGINT, abi.BIGINT, abi.BIGINT]       # partition key, sort key, argument
KAT_ROWS = [(2, 6, 4), (1, 30, 7), (1, 10, 5), (2, 5, None), (1, 20, -3), (1, 10, None), (1, 30, 2), (2, 5, None)]
# sorted: partition 1: x = 5, NULL | -3 | 7, 2 (peers share a sort key); partition 2: NULL, NULL | 4
KAT_ORDER = [2, 5, 4, 1, 6, 3, 7, 0]
N_ = None
KAT = {
    (COUNT_STAR, ROWS): [1, 2, 3, 4, 5, 1, 2, 3], (COUNT_STAR, RANGE): [2, 2, 3, 5, 5, 2, 2, 3], (COUNT_STAR, WHOLE): [5, 5, 5, 5, 5, 3, 3, 3],
    (COUNT, ROWS): [1, 1, 2, 3, 4, 0, 0, 1], (COUNT, RANGE): [1, 1, 2, 4, 4, 0, 0, 1], (COUNT, WHOLE): [4, 4, 4, 4, 4, 1, 1, 1],
    (SUM, ROWS): [5, 5, 2, 9, 11, N_, N_, 4], (SUM, RANGE): [5, 5, 2, 11, 11, N_, N_, 4], (SUM, WHOLE): [11, 11, 11, 11, 11, 4, 4, 4],
    (MIN, ROWS): [5, 5, -3, -3, -3, N_, N_, 4], (MIN, RANGE): [5, 5, -3, -3, -3, N_, N_, 4], (MIN, WHOLE): [-3, -3, -3, -3, -3, 4, 4, 4],
    (MAX, ROWS): [5, 5, 5, 7, 7, N_, N_, 4], (MAX, RANGE): [5, 5, 5, 7, 7, N_, N_, 4], (MAX, WHOLE): [7, 7, 7, 7, 7, 4, 4, 4],
}
KAT_FUNCTIONS = [(f, [] if f == COUNT_STAR else [2], frame) for f, frame in KAT]


def kat_want():
    return [(i, [KAT[key][at] for key in KAT]) for at, i in enumerate(KAT_ORDER)]


def test_the_model_reproduces_the_known_answers():
    """(the restatement itself against the answers worked out by hand: no GPU work)"""
    assert frame_model(KAT_TYPES, KAT_ROWS, [0], [1], [ASC_NULLS_LAST], KAT_FUNCTIONS) == kat_want()
    # ROWS and RANGE differ exactly where peers are tied
    assert KAT[(SUM, ROWS)] != KAT[(SUM, RANGE)] and KAT[(COUNT_STAR, ROWS)] != KAT[(COUNT_STAR, RANGE)]
    assert running(abi.DOUBLE, MAX, [-0.0, 0.0, NAN]) == [-0.0, -0.0, -0.0] and math.copysign(1, running(abi.DOUBLE, MAX, [-0.0, 0.0])[1]) == -1
    assert math.copysign(1, running(abi.DOUBLE, MIN, [0.0, -0.0])[1]) == -1 and math.isnan(running(abi.DOUBLE, MAX, [NAN, NAN])[1])
    assert running(abi.DOUBLE, MAX, [NAN, -math.inf])[1] == -math.inf and running(abi.DOUBLE, MIN, [NAN, -math.inf])[1] == -math.inf
    with pytest.raises(SumOverflow):
        running(abi.BIGINT, SUM, [INT64_MAX, 1, -5])


@pytest.mark.parametrize("device,output_mem", MODES)
def test_known_answers(gpu, device, output_mem):
    """each function x ROWS / RANGE / the whole partition, over partitions with ties in the sort key; host and device input and output"""
    got = run_framed(KAT_TYPES, KAT_ROWS, [0], [1], [ASC_NULLS_LAST], KAT_FUNCTIONS, sizes=[3, 0, 4], device_input=device, output_mem=output_mem, want=kat_want())
    assert [g[3] for g in got] == KAT_ORDER
    assert [list(g[4:]) for g in got] == [w for _, w in kat_want()]
    # GROUPS .. CURRENT ROW is RANGE .. CURRENT ROW; the default frame is RANGE
    groups = [(f, a, GROUPS if frame == RANGE else frame) for f, a, frame in KAT_FUNCTIONS]
    assert run_framed(KAT_TYPES, KAT_ROWS, [0], [1], [ASC_NULLS_LAST], groups, device_input=device, output_mem=output_mem, want=kat_want()) == got
    default = [(f, a) if frame == RANGE else (f, a, frame) for f, a, frame in KAT_FUNCTIONS]
    assert run_framed(KAT_TYPES, KAT_ROWS, [0], [1], [ASC_NULLS_LAST], default, device_input=device, output_mem=output_mem, want=kat_want()) == got


# ---- 2. the ranking functions through the framed entry point ----------------------------------------------------------------------------------
def raw_columns(pages):
    """every block of the output pages as (type, values bytes, nulls bytes)"""
    out = []
    for c in range(len(pages[0].blocks)):
        blocks = [p.blocks[c] for p in pages]
        values = b"".join(np.asarray(b.values[:p.position_count] if b.offsets is None else b.values).tobytes() for b, p in zip(blocks, pages))
        nulls = b"".join((np.zeros(p.position_count, np.uint8) if b.nulls is None else np.asarray(b.nulls[:p.position_count], np.uint8)).tobytes()
                         for b, p in zip(blocks, pages))
        out.append((int(blocks[0].type), values, nulls))
    return out


def test_ranking_functions_are_bit_for_bit_those_of_the_unframed_operator(gpu):
    """the six through pa_framed_window_create, alone and mixed with aggregates in one operator, against pa_window_create"""
    rng = np.random.default_rng(21)
    total = 3 * T + 17
    part = rng.integers(0, 40, total).astype(np.int64)
    key = rng.integers(0, 9, total).astype(np.float64) / 2
    buckets = rng.integers(1, 9, total).astype(np.int64)
    x = rng.integers(-1000, 1000, total).astype(np.int64)
    x_nulls = rng.random(total) < 0.2
    types = [abi.BIGINT, abi.DOUBLE, abi.BIGINT, abi.BIGINT]
    six = RANKING + [(NTILE, [2])]

    def pages_of(op):
        for a in range(0, total, 1500):
            b = min(a + 1500, total)
            op.addInput(Page([Block.bigint(part[a:b]), Block.double(key[a:b]), Block.bigint(buckets[a:b]), Block.bigint(x[a:b], x_nulls[a:b])], b - a))
        return drain(op)

    plain = raw_columns(pages_of(WindowOperator(types, [0, 3], six, [0], [1], [DESC_NULLS_FIRST])))
    odd_frame = (abi.FRAME_ROWS, abi.BOUND_PRECEDING, abi.BOUND_FOLLOWING, 2, 2, 0)           # range-checked and otherwise ignored
    alone = raw_columns(pages_of(FramedWindowOperator(types, [0, 3], [(f, [], odd_frame) for f in RANKING] + [(NTILE, [2])], [0], [1], [DESC_NULLS_FIRST])))
    assert alone == plain
    mixed_functions = [(SUM, [3], ROWS), ROW_NUMBER, (MIN, [3]), RANK, DENSE_RANK, (COUNT, [3], WHOLE), PERCENT_RANK, CUME_DIST, COUNT_STAR, (NTILE, [2]), (MAX, [3], ROWS)]
    mixed = raw_columns(pages_of(FramedWindowOperator(types, [0, 3], mixed_functions, [0], [1], [DESC_NULLS_FIRST])))
    assert [mixed[k] for k in (0, 1, 3, 5, 6, 8, 9, 11)] == plain
    rows = [(int(p), float(k), int(b), None if nl else int(v)) for p, k, b, v, nl in zip(part, key, buckets, x, x_nulls)]
    run_framed(types, rows[:700], [0], [1], [DESC_NULLS_FIRST], mixed_functions)


# ---- 3. identities that need no model -------------------------------------------------------------------------------------------------------
def run_numpy(columns, nulls, types, partition, sort, functions, sizes=None, device_input=True, output_mem=abi.MEM_DEVICE, orders=None):
    """numpy columns (nulls[c]: a bool array or None) + a BIGINT input-position column behind them ->
    (positions in output order, [(values, nulls or None) per function])."""
    total = len(columns[0])
    op = FramedWindowOperator(list(types) + [abi.BIGINT], [len(types)], functions, partition, sort, orders or [ASC_NULLS_LAST] * len(sort), output_mem=output_mem)
    at = 0
    sizes = list(sizes or [total])
    while at < total:
        m = min(sizes.pop(0) if sizes else total - at, total - at)
        blocks = [Block.flat(t, c[at:at + m], None if nl is None else nl[at:at + m]) for t, c, nl in zip(types, columns, nulls)]
        page = Page(blocks + [Block.bigint(np.arange(at, at + m, dtype=np.int64))], m)
        op.addInput(upload_page(page) if device_input else page)
        at += m
    pages = drain(op)
    op.close()
    out = []
    for c in range(1 + len(functions)):
        values = np.concatenate([p.blocks[c].values[:p.position_count] for p in pages])
        has = any(p.blocks[c].nulls is not None for p in pages)
        out.append((values, np.concatenate([np.zeros(p.position_count, np.uint8) if p.blocks[c].nulls is None else p.blocks[c].nulls[:p.position_count]
                                            for p in pages]).astype(bool) if has else None))
    assert out[0][1] is None
    return out[0][0], out[1:]


def test_identities(gpu):
    rng = np.random.default_rng(31)
    total = 2 * T + 301
    part = rng.integers(0, 25, total).astype(np.int64)
    key = rng.integers(0, 12, total).astype(np.int64)
    functions = [(COUNT_STAR, [], ROWS), ROW_NUMBER, (COUNT_STAR, [], RANGE), RANK, CUME_DIST, (COUNT_STAR, [], WHOLE), (COUNT_STAR, [], GROUPS),
                 (COUNT, [1], ROWS), (COUNT, [1], RANGE), (SUM, [1], GROUPS), (SUM, [1], RANGE)]
    _, cols = run_numpy([part, key], [None, None], [abi.BIGINT, abi.BIGINT], [0], [1], functions, sizes=[1000, 1000])
    assert all(nl is None for _, nl in cols)
    v = [c for c, _ in cols]
    assert np.array_equal(v[0], v[1])                                             # count(*) ROWS = row_number()
    size = v[5]
    # count(*) RANGE = rank() + peers - 1 = cume_dist * N: the peers of a row are those with its rank
    starts = np.flatnonzero(v[1] == 1)
    part_id = np.cumsum(v[1] == 1) - 1
    peers = np.zeros(total, np.int64)
    for p in range(len(starts)):
        sel = part_id == p
        ranks, counts = np.unique(v[3][sel], return_counts=True)
        peers[sel] = counts[np.searchsorted(ranks, v[3][sel])]
    assert np.array_equal(v[2], v[3] + peers - 1)
    assert np.array_equal(v[2].astype(np.float64) / size.astype(np.float64), v[4]) and np.array_equal(np.rint(v[4] * size).astype(np.int64), v[2])
    assert np.array_equal(size, np.bincount(part_id)[part_id])                    # count(*) over the whole partition = N
    assert np.array_equal(v[6], v[2])                                             # GROUPS .. CURRENT ROW = RANGE .. CURRENT ROW
    assert np.array_equal(v[7], v[0]) and np.array_equal(v[8], v[2])              # count(x) without NULLs = count(*)
    assert np.array_equal(v[9], v[10])
    # no sort channels: the partition is one peer group, and ROWS alone still counts up
    functions = [(f, a, frame) for f, a in ((COUNT_STAR, []), (SUM, [1]), (MAX, [1])) for frame in (RANGE, GROUPS, WHOLE, ROWS)]
    _, cols = run_numpy([part, key], [None, None], [abi.BIGINT, abi.BIGINT], [0], [], functions)
    v = [c for c, _ in cols]
    for k in (0, 4, 8):
        assert np.array_equal(v[k], v[k + 1]) and np.array_equal(v[k], v[k + 2])
    assert not np.array_equal(v[0], v[3])


# ---- 4. the tile boundaries of the scans ------------------------------------------------------------------------------------------------------
def np_frame_model(part, key, x, x_null, functions):
    """numeric columns without NaN / -0.0, everything ascending, |x| < 2^31 -> (input positions in output order, [(values, nulls)])"""
    total = len(part)
    order, (row_number, rank) = np_model([part], [key], [ROW_NUMBER, RANK])
    at = np.arange(total)
    place, ps = row_number - 1, rank - 1
    first = at - place
    part_id = np.cumsum(place == 0) - 1
    size = np.bincount(part_id)[part_id]
    peer_head = (place == 0) | (np.concatenate([[0], ps[:-1]]) != ps)
    peer_id = np.cumsum(peer_head) - 1
    pe = ps + np.bincount(peer_id)[peer_id]
    xs, valid = x[order].astype(np.int64), ~x_null[order]
    big = np.int64(1) << 33
    count = np.cumsum(valid)
    count = count - (count - valid)[first]
    total_sum = np.cumsum(np.where(valid, xs, 0))
    total_sum = total_sum - (total_sum - np.where(valid, xs, 0))[first]
    low = np.minimum.accumulate(np.where(valid, xs, big // 2 - 1) - part_id * big) + part_id * big
    high = np.maximum.accumulate(np.where(valid, xs, -(big // 2 - 1)) + part_id * big) - part_id * big
    out = []
    for f, _, frame in framed(functions):
        e = first + (size - 1 if frame[2] == UF else place if frame[0] == abi.FRAME_ROWS else pe - 1)
        if f == ROW_NUMBER:
            out.append((row_number, None))
        elif f == COUNT_STAR:
            out.append((e - first + 1, None))
        elif f == COUNT:
            out.append((count[e], None))
        else:
            state = {SUM: total_sum, MIN: low, MAX: high}[f][e]
            out.append((np.where(count[e] > 0, state, 0), count[e] == 0))
    return order, out


def test_the_numpy_model_agrees_with_the_row_model():
    rng = np.random.default_rng(41)
    total = 400
    part, key = rng.integers(0, 9, total).astype(np.int64), rng.integers(0, 5, total).astype(np.int64)
    x, x_null = rng.integers(-50, 50, total).astype(np.int64), rng.random(total) < 0.4
    functions = [(f, [] if f == COUNT_STAR else [2], frame) for f in (COUNT_STAR, COUNT, SUM, MIN, MAX) for frame in (ROWS, RANGE, WHOLE)] + [ROW_NUMBER]
    order, cols = np_frame_model(part, key, x, x_null, functions)
    rows = [(int(p), int(k), None if nl else int(v)) for p, k, v, nl in zip(part, key, x, x_null)]
    want = frame_model([abi.BIGINT] * 3, rows, [0], [1], [ASC_NULLS_LAST], functions)
    assert order.tolist() == [i for i, _ in want]
    for k, (values, nulls) in enumerate(cols):
        got = [None if nulls is not None and nulls[j] else int(values[j]) for j in range(total)]
        assert got == [w[k] for _, w in want], functions[k]


BOUNDARY_FUNCTIONS = [(COUNT_STAR, [], RANGE), (COUNT, [2], ROWS), (SUM, [2], ROWS), (SUM, [2], RANGE), (SUM, [2], WHOLE), (MIN, [2], ROWS), (MAX, [2], RANGE),
                      ROW_NUMBER]


def boundary_columns(n, layout):
    """partition and sort key by sorted place"""
    at = np.arange(n, dtype=np.int64)
    if layout == "one_partition":
        return np.zeros(n, np.int64), at.copy()
    if layout == "tile_starts":                  # every partition starts exactly where a tile starts
        return at // T, at.copy()
    if layout == "spanning":                     # one-row partitions around a partition of more than three tiles: [5, 5 + 3 T + 7)
        return np.where(at < 5, at, np.where(at < 5 + 3 * T + 7, 5, at - 3 * T - 1)), at.copy()
    if layout == "own_partitions":
        return at.copy(), np.zeros(n, np.int64)
    # peer groups of 7 rows that straddle every tile boundary they meet: [T - 3, T + 4) is one; RANGE reads a state in the next tile
    return at // (5 * T), (at - (T - 3)) // 7


@pytest.mark.parametrize("layout", ["one_partition", "tile_starts", "spanning", "own_partitions", "straddling_peers"])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 2 * T + 1, T * T + 1])
def test_scan_boundaries(gpu, n, layout):
    """the last size makes the scan of the tile states itself take more than one tile"""
    part, key = boundary_columns(n, layout)
    rng = np.random.default_rng(n)
    x = rng.integers(-1000, 1000, n).astype(np.int64)
    x_null = rng.random(n) < 0.1
    shuffle = rng.permutation(n)                 # the sort has work to do
    part, key, x, x_null = part[shuffle], key[shuffle], x[shuffle], x_null[shuffle]
    pos, got = run_numpy([part, key, x], [None, None, x_null], [abi.BIGINT] * 3, [0], [1], BOUNDARY_FUNCTIONS)
    order, want = np_frame_model(part, key, x, x_null, BOUNDARY_FUNCTIONS)
    assert np.array_equal(pos, order)
    for f, (g, g_null), (w, w_null) in zip(BOUNDARY_FUNCTIONS, got, want):
        if w_null is None or not w_null.any():
            assert g_null is None or not g_null.any(), f
        else:
            assert g_null is not None and np.array_equal(g_null, w_null), f
            g = np.where(g_null, 0, g)
        assert g.dtype == np.int64 and np.array_equal(g, w), f


# ---- 5. segment hygiene ---------------------------------------------------------------------------------------------------------------------------
def test_nothing_leaks_across_a_partition_start(gpu):
    """an all-NULL partition behind a partition with values: NULL sum / min / max and count 0; leading NULLs inside a partition"""
    functions = [(f, [1], frame) for f in (COUNT, SUM, MIN, MAX) for frame in (ROWS, RANGE, WHOLE)]
    rows = [(1, 5, 1), (1, 9, 2), (2, None, 1), (2, None, 2), (2, None, 2), (3, None, 1), (3, None, 2), (3, 4, 3), (3, None, 4), (4, -1, 1)]
    got = run_framed([abi.BIGINT, abi.BIGINT, abi.BIGINT], rows, [0], [2], [ASC_NULLS_LAST], functions)
    for g in got[2:5]:
        assert g[4:] == (0, 0, 0) + (None,) * 9
    assert got[5][4:] == (0, 0, 1) + (None, None, 4) * 3 and got[7][4:] == (1, 1, 1) + (4,) * 9
    # the same over tiles: a partition of T + 9 values, then T + 9 NULLs, then values again
    n = T + 9
    rows = [(1, k, k) for k in range(n)] + [(2, None, k) for k in range(n)] + [(3, 7, k) for k in range(n)]
    got = run_framed([abi.BIGINT, abi.BIGINT, abi.BIGINT], rows, [0], [2], [ASC_NULLS_LAST], functions)
    assert all(g[4:] == (0, 0, 0) + (None,) * 9 for g in got[n:2 * n])


@pytest.mark.parametrize("order", [ASC_NULLS_FIRST, ASC_NULLS_LAST, DESC_NULLS_FIRST, DESC_NULLS_LAST])
def test_nulls_first_and_last_under_each_sort_order(gpu, order):
    """the argument is the sort channel: its NULLs open or close every partition"""
    rng = np.random.default_rng(51)
    rows = [(int(rng.integers(0, 4)), None if rng.random() < 0.3 else int(rng.integers(-5, 6))) for _ in range(300)]
    functions = [(f, [1], frame) for f in (COUNT, SUM, MIN, MAX) for frame in (ROWS, RANGE, WHOLE)] + [(COUNT_STAR, [], RANGE)]
    run_framed([abi.BIGINT, abi.BIGINT], rows, [0], [1], [order], functions, sizes=[100, 100])


# ---- 6. types ---------------------------------------------------------------------------------------------------------------------------------------
def values_of(t, rng, total):
    if t in (abi.DOUBLE, abi.REAL):
        pool = [NAN, -0.0, 0.0, math.inf, -math.inf, 1.5, -2.25, 1e30, -1e-30, 3.0]
        return [pool[int(k)] for k in rng.integers(0, len(pool), total)]
    if t == abi.BOOLEAN:
        return [bool(k) for k in rng.integers(0, 2, total)]
    if t == abi.BIGINT or t == abi.DECIMAL:
        return [int(k) for k in rng.integers(-(1 << 40), 1 << 40, total)]
    return [int(k) for k in rng.integers(-100000, 100000, total)]


@pytest.mark.parametrize("t", MIN_MAX_TYPES, ids=lambda t: abi.TYPE_NAMES[int(t)])
def test_min_max_over_every_accepted_type(gpu, t):
    rng = np.random.default_rng(61 + int(t))
    total = 2 * T + 50
    values = values_of(t, rng, total)
    rows = [(int(rng.integers(0, 6)), None if rng.random() < 0.25 else v, int(rng.integers(0, 30))) for v in values]
    functions = [(f, [1], frame) for f in (MIN, MAX) for frame in (ROWS, RANGE, WHOLE)] + [(COUNT, [1], ROWS)]
    run_framed([abi.BIGINT, t, abi.BIGINT], rows, [0], [2], [ASC_NULLS_LAST], functions, sizes=[1000, 700], device_input=True, output_mem=abi.MEM_DEVICE)


@pytest.mark.parametrize("t", [abi.DOUBLE, abi.REAL])
def test_floating_point_edges(gpu, t):
    """NaN, both zeros, both infinities; an all-NaN partition; max of {-0.0, +0.0} in both arrival orders"""
    partitions = [[NAN, NAN, NAN], [-0.0, 0.0], [0.0, -0.0], [NAN, -math.inf], [-math.inf, NAN], [math.inf, NAN, -math.inf, 0.0, -0.0, NAN, 2.5],
                  [None, NAN, None, 1.0], [1.0, NAN, 2.0], [NAN, None], [-0.0, -0.0, 0.0], [0.0, 0.0, -0.0]]
    rows = [(p, v, k) for p, values in enumerate(partitions) for k, v in enumerate(values)]
    functions = [(f, [1], frame) for f in (MIN, MAX) for frame in (ROWS, WHOLE)]
    got = run_framed([abi.BIGINT, t, abi.BIGINT], rows, [0], [2], [ASC_NULLS_LAST], functions)
    by_partition = {p: [g for g in got if g[0] == p] for p in range(len(partitions))}
    assert all(math.isnan(v) for g in by_partition[0] for v in g[4:])                           # all NaN: NaN
    sign = lambda v: math.copysign(1, v)
    assert [sign(g[7]) for g in by_partition[1]] == [-1, -1] and [sign(g[7]) for g in by_partition[2]] == [1, 1]    # max: the zeros tie, the first stays
    assert [sign(g[5]) for g in by_partition[1]] == [-1, -1] and [sign(g[5]) for g in by_partition[2]] == [-1, -1]  # min: -0.0 before +0.0
    assert by_partition[3][0][7] == -math.inf and by_partition[4][0][7] == -math.inf            # max: NaN loses to everything
    assert by_partition[3][0][5] == -math.inf and by_partition[4][0][5] == -math.inf            # min: NaN largest


def test_count_over_varchar_and_long_decimal(gpu):
    rng = np.random.default_rng(71)
    words = ["", "a", None, "abcdefghij", None, "b"]
    rows = [(int(rng.integers(0, 5)), words[int(rng.integers(0, 6))], None if rng.random() < 0.5 else int(rng.integers(-9, 9)) * 10 ** 25, int(rng.integers(0, 9)))
            for _ in range(500)]
    types = [abi.BIGINT, abi.VARCHAR, abi.decimal(30, 2), abi.BIGINT]
    functions = [(COUNT, [1], ROWS), (COUNT, [2], RANGE), (COUNT, [1], WHOLE), (COUNT, [2], ROWS), COUNT_STAR]
    run_framed(types, rows, [0], [3], [ASC_NULLS_LAST], functions, sizes=[200], output_channels=[0, 1, 4])
    run_framed(types, rows, [0], [3], [DESC_NULLS_LAST], functions, device_input=True, output_mem=abi.MEM_DEVICE)


def test_dictionary_and_rle_argument_blocks(gpu):
    part = Block.dictionary_block(Block.flat(abi.BIGINT, [5, 4, 0], [0, 0, 1]), [0, 1, 2, 2, 0, 1, 0, 0])
    x = Block.dictionary_block(Block.flat(abi.BIGINT, [7, -3, 0], [0, 0, 1]), [1, 1, 2, 0, 2, 0, 0, 1])
    rle = Block.rle(Block.double([2.5]), 8)
    rle_null = Block.rle(Block.flat(abi.INTEGER, [0], [1]), 8)
    types = [abi.BIGINT, abi.BIGINT, abi.DOUBLE, abi.INTEGER]
    rows = list(zip(part.to_pylist(), x.to_pylist(), rle.to_pylist(), rle_null.to_pylist()))
    functions = [(SUM, [1], ROWS), (MIN, [1]), (MAX, [2], WHOLE), (COUNT, [3]), (SUM, [3], WHOLE), (MIN, [2], ROWS), (COUNT, [1], ROWS)]
    for device in (False, True):
        op = FramedWindowOperator(types + [abi.BIGINT], [0, 4], functions, [0], [1], [ASC_NULLS_FIRST])
        all_rows = []
        for rep in range(3):
            page = Page([part, x, rle, rle_null, Block.bigint(list(range(8 * rep, 8 * rep + 8)))], 8)
            op.addInput(upload_page(page) if device else page)
            all_rows += rows
        got = [r for p in drain(op) for r in p.to_rows()]
        want = frame_model(types, all_rows, [0], [1], [ASC_NULLS_FIRST], functions)
        assert [g[1] for g in got] == [i for i, _ in want]
        for g, (i, values) in zip(got, want):
            assert all(same_out(result_type(types, f, a), v, w) for (f, a, _), v, w in zip(framed(functions), g[2:], values)), (g, values)


def test_an_argument_channel_that_is_also_a_sort_partition_or_output_channel(gpu):
    rng = np.random.default_rng(81)
    rows = [(None if rng.random() < 0.1 else int(rng.integers(0, 5)), None if rng.random() < 0.2 else int(rng.integers(-20, 20))) for _ in range(400)]
    functions = [(SUM, [0], ROWS), (MAX, [0]), (COUNT, [0], WHOLE), (SUM, [1], ROWS), (MIN, [1], RANGE), (COUNT, [1], ROWS)]
    run_framed([abi.BIGINT, abi.BIGINT], rows, [0], [1], [DESC_NULLS_FIRST], functions, sizes=[150, 150])      # channel 0 partitions, 1 sorts; both go out
    run_framed([abi.BIGINT, abi.BIGINT], rows, [1], [0], [ASC_NULLS_LAST], functions, output_channels=[2])


# ---- 7. sum overflow ----------------------------------------------------------------------------------------------------------------------------------
def sum_status(partitions, values, frame=RANGE, extra=()):
    """status of pa_op_get_output after finish for sum(values) partitioned by `partitions` in arrival order; the operator is closed and destroyed"""
    n = len(values)
    op = FramedWindowOperator([abi.BIGINT, abi.BIGINT, abi.BIGINT], [2], [(SUM, [1], frame)] + list(extra), [0], [2], [ASC_NULLS_LAST])
    nulls = [v is None for v in values]
    op.addInput(Page([Block.bigint(np.asarray(partitions, np.int64)), Block.bigint(np.asarray([0 if v is None else v for v in values], np.int64), nulls),
                      Block.bigint(np.arange(n, dtype=np.int64))], n))
    op.finish()
    out = abi.pa_page()
    status = lib().pa_op_get_output(op._h, C.byref(out))
    message = lib().pa_last_error() if status < 0 else b""
    if status < 0:
        assert op.getOutput() is None and op.isFinished()     # nothing is emitted
    op.close()
    return status, message


def test_sum_overflow(gpu):
    ok = 0                                                    # (a page, or none: not an error)
    for frame in (ROWS, RANGE, WHOLE):                        # the rule does not depend on the frame
        assert sum_status([1, 1, 1], [INT64_MAX - 5, 2, 3], frame)[0] >= ok                     # exactly INT64_MAX
        status, message = sum_status([1, 1, 1], [INT64_MAX - 5, 2, 4], frame)                   # one more
        assert status == abi.ERR_NUMERIC_VALUE_OUT_OF_RANGE and b"overflow" in message
        assert sum_status([1, 1, 1], [INT64_MIN + 5, -2, -3], frame)[0] >= ok                   # exactly INT64_MIN
        assert sum_status([1, 1, 1], [INT64_MIN + 5, -2, -4], frame)[0] == abi.ERR_NUMERIC_VALUE_OUT_OF_RANGE
        assert sum_status([1, 1, 1], [INT64_MAX, 1, -5], frame)[0] == abi.ERR_NUMERIC_VALUE_OUT_OF_RANGE      # a prefix overflows, a later row brings it back
        assert sum_status([1, 1, 1, 1], [INT64_MAX, None, 1, -5], frame)[0] == abi.ERR_NUMERIC_VALUE_OUT_OF_RANGE
        assert sum_status([1, 1, 2, 2], [INT64_MAX - 1, 1, INT64_MAX - 1, 1], frame)[0] >= ok   # neighbouring partitions never affect each other
        assert sum_status([1, 2, 3], [INT64_MAX, INT64_MAX, INT64_MIN], frame)[0] >= ok
    n = 3 * T
    assert sum_status([7] * n, [1 << 62] * n)[0] == abi.ERR_NUMERIC_VALUE_OUT_OF_RANGE         # shows only across tiles
    assert sum_status([7] * n, [(1 << 62) if k % 2 == 0 else -(1 << 62) for k in range(n)])[0] >= ok
    assert sum_status([7] * n + [8], [1] * n + [INT64_MAX], extra=[(MIN, [1])])[0] >= ok
    with pytest.raises(SumOverflow):
        frame_model([abi.BIGINT] * 2, [(1, INT64_MAX), (1, 1), (1, -5)], [0], [], [], [(SUM, [1], WHOLE)])


# ---- 8. page cuts, memory spaces, the state machine ---------------------------------------------------------------------------------------------------
def test_page_cuts_and_memory_spaces_do_not_change_the_output(gpu):
    rng = np.random.default_rng(91)
    rows = [(int(rng.integers(0, 6)), "s%d" % int(rng.integers(0, 4)), None if rng.random() < 0.2 else float(rng.integers(0, 5)) / 2,
             None if rng.random() < 0.2 else int(rng.integers(-9, 9))) for _ in range(60)]
    types = [abi.BIGINT, abi.VARCHAR, abi.DOUBLE, abi.BIGINT]
    functions = [(SUM, [3], ROWS), (MIN, [2]), RANK, (MAX, [2], WHOLE), (COUNT, [1], ROWS), (COUNT_STAR, [], GROUPS), (SUM, [3])]
    outputs = []
    for sizes in ([60], [7, 0, 40], [1] * 60):
        for device, output_mem in MODES:
            outputs.append(run_framed(types, rows, [0], [1], [DESC_NULLS_LAST], functions, sizes=sizes, device_input=device, output_mem=output_mem))
    assert all(repr(o) == repr(outputs[0]) for o in outputs)


def test_state_machine_and_memory_bytes(gpu):
    functions = [(SUM, [0], ROWS), (MIN, [0])]
    op = FramedWindowOperator([abi.BIGINT, abi.VARCHAR], [0, 1], functions, [0], [1], [ASC_NULLS_LAST])
    assert op.needsInput() and not op.isFinished() and op.getOutput() is None
    empty = Page([Block.bigint([]), Block.varchar([])], 0)
    op.addInput(empty)
    op.addInput(Page([Block.bigint([3, 1, 3]), Block.varchar(["b", "a", "a"])], 3))
    held = op.memoryBytes()
    assert held > 0 and op.needsInput() and op.getOutput() is None and not op.isFinished()
    op.finish()
    assert not op.needsInput() and not op.isFinished()
    cpage, _keep = Page([Block.bigint([1]), Block.varchar(["x"])], 1).to_c()
    assert lib().pa_op_add_input(op._h, C.byref(cpage)) == abi.ERR_ILLEGAL_STATE
    assert op.getOutput().to_rows() == [(1, b"a", 1, 1), (3, b"a", 3, 3), (3, b"b", 6, 3)]
    assert op.isFinished() and op.getOutput() is None and not op.needsInput()
    op.finish()
    op.close()
    # the scans' scratch is counted: the same rows cost more with an aggregate than with rank() alone
    n = 4 * T
    page = Page([Block.bigint(np.arange(n) % 7), Block.bigint(np.arange(n))], n)
    sizes = []
    for fs in ([RANK], [RANK, (SUM, [1], ROWS)], [RANK, (SUM, [1], ROWS), (MAX, [1], ROWS)]):
        op = FramedWindowOperator([abi.BIGINT, abi.BIGINT], [0], fs, [0], [1], [ASC_NULLS_LAST])
        op.addInput(page)
        before = op.memoryBytes()
        assert len(drain(op)) >= 1
        sizes.append(op.memoryBytes() - before)
        op.close()
    assert sizes[0] + 2 * 8 * n <= sizes[1] and sizes[0] + 3 * 8 * n <= sizes[2]   # the sorted argument and one scanned state; one more state
    for fs in ([COUNT_STAR], [(SUM, [0])]):                                         # no rows at all: no page
        op = FramedWindowOperator([abi.BIGINT], [0], fs, [], [], [])
        op.addInput(Page([Block.bigint([])], 0))
        assert drain(op) == []
        op.close()


def test_the_same_function_and_frame_twice(gpu):
    rows = [(k % 3, None if k % 5 == 0 else k) for k in range(50)]
    functions = [(SUM, [1], ROWS), (SUM, [1], ROWS), (MAX, [1]), (SUM, [1], WHOLE), (MAX, [1]), COUNT_STAR, COUNT_STAR] + [(COUNT, [1], ROWS)] * 9
    got = run_framed([abi.BIGINT, abi.BIGINT], rows, [0], [1], [ASC_NULLS_LAST], functions)
    assert all(g[3] == g[4] and g[5] == g[7] and g[8] == g[9] and len(set(g[10:])) == 1 for g in got)


# ---- 9. seeded fuzz ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_fuzz(gpu, seed):
    rng = np.random.default_rng(8000 + seed)
    total = int(rng.integers(1, 5001))
    types = [abi.BIGINT, abi.INTEGER, abi.DOUBLE] + [MIN_MAX_TYPES[int(k)] for k in rng.integers(0, len(MIN_MAX_TYPES), 3)] + [abi.VARCHAR]
    null_rate = float(rng.choice([0.0, 0.1, 0.9]))
    columns = [[int(k) for k in rng.integers(0, int(rng.choice([1, 3, 200])), total)], [int(k) for k in rng.integers(0, 3, total)],
               [float(k) / 4 for k in rng.integers(0, int(rng.choice([1, 3, 40])), total)]]
    columns += [values_of(t, rng, total) for t in types[3:6]] + [["s%d" % k for k in rng.integers(0, 5, total)]]
    columns = [c if at < 3 and null_rate > 0.5 else [None if rng.random() < null_rate else v for v in c] for at, c in enumerate(columns)]
    rows = list(zip(*columns))
    partition = [[0], [0, 1], []][int(rng.integers(0, 3))]
    sort = [[2], [2, 1], [], [3]][int(rng.integers(0, 4))]
    orders = [int(rng.integers(0, 4)) for _ in sort]
    functions = []
    for _ in range(int(rng.integers(1, 17))):
        f = int(rng.integers(0, 11))
        frame = FRAMES[int(rng.integers(0, len(FRAMES)))]
        if f < NTILE:
            functions.append((f, [], frame))
        elif f == NTILE:
            functions.append((ROW_NUMBER, [], frame))
        elif f == COUNT_STAR:
            functions.append((f, [], frame))
        elif f == COUNT:
            functions.append((f, [int(rng.integers(0, 7))], frame))
        elif f == SUM:
            functions.append((f, [int(rng.integers(0, 2))], frame))
        else:
            functions.append((f, [int(rng.integers(0, 6))], frame))
    sizes = [int(s) for s in rng.integers(1, max(2, total // 2), int(rng.integers(1, 6)))]
    run_framed(types, rows, partition, sort, orders, functions, sizes=sizes, device_input=bool(rng.integers(0, 2)), output_mem=int(rng.integers(0, 2)))


# ---- 10. the C++ mirror --------------------------------------------------------------------------------------------------------------------------------
def test_cpp_mirror(gpu):
    """tests/cpp/test_window_frames.cpp: the operator through the C++ host mirror's runDriver."""
    exe = os.path.join(ROOT, "tests", "cpp", "test_window_frames")
    src = exe + ".cpp"
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-L" + os.path.join(ROOT, "presto_amd"),
                               "-lpresto_amd", "-Wl,-rpath,$ORIGIN/../../presto_amd", "-Wl,--allow-shlib-undefined", "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode == 0, r.stdout.decode()[-2000:]
    assert "window frames ok" in r.stdout.decode()
