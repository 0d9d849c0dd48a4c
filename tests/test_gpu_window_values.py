"""GPU checks of the value window functions of WindowOperator (pa_framed_window_create ids 11 .. 15: lag / lead / first_value / last_value /
nth_value).  Order, partitions, peers, the ranking functions and the frame end e are the restatements of tests/test_gpu_window.py and
tests/test_gpu_window_frames.py, imported; this file adds only the five rules of include/presto_amd.h (`value_of`): which row of the
partition a value is copied from, or the default, or NULL.  The model names the SOURCE of every result -- (channel, input row) -- and
the operator's column is compared with the input column's bytes at that row: every comparison is exact, bit for bit, whatever the type.
Known answers by hand, workgroup boundaries and the 64-bit offsets, per-row offsets, every value type, identities that need no model,
mixed functions, segment hygiene, offset errors, page cuts and memory spaces, fuzz."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from presto_amd import abi
from presto_amd._lib import lib
from presto_amd.operators import FramedWindowOperator, FramedWindowOperatorFactory, upload_page
from presto_amd.page import Block, Page
from tests.test_gpu_window import ASC_NULLS_FIRST, ASC_NULLS_LAST, DESC_NULLS_FIRST, DESC_NULLS_LAST, MODES, NTILE, RANK, ROW_NUMBER, drain, split
from tests.test_gpu_window_frames import (COUNT, COUNT_STAR, FRAMES, GROUPS, INT64_MAX, INT64_MIN, MIN, RANGE, ROWS, SUM, WHOLE, frame_model, framed,
                                          raw_columns, result_type, same_out)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# rows of one workgroup of the function pass, as the kernel header states it
BLOCK = int(re.search(r"kWindowRowsPerBlock\s*=\s*(\d+)", open(os.path.join(ROOT, "presto_amd", "csrc", "window_kernels.hpp")).read()).group(1))
LAG, LEAD, FIRST_VALUE, LAST_VALUE, NTH_VALUE = abi.WINDOW_LAG, abi.WINDOW_LEAD, abi.WINDOW_FIRST_VALUE, abi.WINDOW_LAST_VALUE, abi.WINDOW_NTH_VALUE
VALUE_FUNCTIONS = (LAG, LEAD, FIRST_VALUE, LAST_VALUE, NTH_VALUE)
VALUE_TYPES = [abi.BIGINT, abi.INTEGER, abi.DATE, abi.DOUBLE, abi.REAL, abi.BOOLEAN, abi.decimal(12, 2), abi.decimal(30, 2)]
DTYPES = {abi.BIGINT: np.int64, abi.INTEGER: np.int32, abi.DATE: np.int32, abi.DOUBLE: np.float64, abi.REAL: np.float32, abi.BOOLEAN: np.uint8,
          abi.DECIMAL: np.int64}
NAN_BITS_64 = [0x7FF8000000000000, 0xFFF8000000ABCDEF]          # two NaNs: the canonical one, and a negative one with a payload
NAN_BITS_32 = [0x7FC00000, 0xFFC12345]


# ---- the contract of the value functions, restated -----------------------------------------------------------------------------------------
class BadOffset(Exception):
    pass


def source(rows, row, channel):
    """the value of `channel` at input row `row`: where it stands, or NULL"""
    return None if rows[row][channel] is None else (channel, row)


def value_of(f, args, rows, i, place, size, e, row_at):
    """Input row i stands at `place` of a partition of `size` rows whose place t holds input row row_at(t); its frame is the places 0 .. e."""
    if f in (LAG, LEAD):
        offset = 1 if len(args) < 2 else rows[i][args[1]]
        if offset is None:
            return None
        if offset < 0:
            raise BadOffset("Offset must be at least 0")
        if offset > (place if f == LAG else size - 1 - place):
            return source(rows, i, args[2]) if len(args) > 2 else None
        return source(rows, row_at(place - offset if f == LAG else place + offset), args[0])
    if f == FIRST_VALUE:
        return source(rows, row_at(0), args[0])
    if f == LAST_VALUE:
        return source(rows, row_at(e), args[0])
    offset = rows[i][args[1]]
    if offset is None:
        return None
    if offset < 1:
        raise BadOffset("Offset must be at least 1")
    return source(rows, row_at(offset - 1), args[0]) if offset - 1 <= e else None


def value_model(types, rows, partition, sort, orders, functions):
    """-> [(input position, [per function: a value function's source (channel, input row) or None = NULL; any other function's value])] in
    output order.  Place, partition size and frame end are read off frame_model's row_number and count(*) columns."""
    fs = framed(functions)
    probes = [ROW_NUMBER, (COUNT_STAR, [], WHOLE)]
    for f, a, frame in fs:
        probes.append((COUNT_STAR, [], WHOLE if f in (LAG, LEAD) else frame) if f in VALUE_FUNCTIONS else (f, a, frame))
    base = frame_model(types, rows, partition, sort, orders, probes)
    out = []
    for at, (i, values) in enumerate(base):
        place, size = values[0] - 1, values[1]
        first = at - place
        result = []
        for (f, a, _), v in zip(fs, values[2:]):
            result.append(value_of(f, a, rows, i, place, size, v - 1, lambda t: base[first + t][0]) if f in VALUE_FUNCTIONS else v)
        out.append((i, result))
    return out


# ---- driving the operator ---------------------------------------------------------------------------------------------------------------------
def column_block(t, values, nulls):
    if int(t) == abi.LONG_DECIMAL:
        nl = None if nulls is None or not nulls.any() else np.ascontiguousarray(nulls.astype(np.uint8))
        return Block(abi.LONG_DECIMAL, abi.FLAT, len(values), values=np.ascontiguousarray(values), nulls=nl)
    return Block.flat(int(t), values, nulls)


def rows_of(types, columns, nulls):
    """the columns as rows of Python values for the model: None = NULL; a long decimal only says whether it is NULL"""
    def py(t, v):
        if int(t) == abi.LONG_DECIMAL:
            return 0
        return float(v) if int(t) in (abi.DOUBLE, abi.REAL) else int(v)
    return [tuple(None if nl is not None and nl[r] else py(t, c[r]) for t, c, nl in zip(types, columns, nulls)) for r in range(len(columns[0]))]


def make_operator(types, functions, partition, sort, orders, output_mem=abi.MEM_HOST):
    return FramedWindowOperator(list(types) + [abi.BIGINT], [len(types)], functions, partition, sort, orders, output_mem=output_mem)


def feed_columns(op, types, columns, nulls, sizes=None, device_input=False):
    total = len(columns[0])
    at = 0
    for chunk in split(list(range(total)), sizes or [total]):
        m = len(chunk)
        blocks = [column_block(t, c[at:at + m], None if nl is None else nl[at:at + m]) for t, c, nl in zip(types, columns, nulls)]
        page = Page(blocks + [Block.bigint(np.arange(at, at + m, dtype=np.int64))], m)
        op.addInput(upload_page(page) if device_input else page)
        at += m


def output_columns(pages, count):
    """-> [(type, values, nulls as bool or None)] of the first `count` columns over all pages"""
    out = []
    for c in range(count):
        values = np.concatenate([p.blocks[c].values[:p.position_count] for p in pages])
        has = any(p.blocks[c].nulls is not None for p in pages)
        nulls = np.concatenate([np.zeros(p.position_count, np.uint8) if p.blocks[c].nulls is None else p.blocks[c].nulls[:p.position_count]
                                for p in pages]).astype(bool) if has else None
        out.append((int(pages[0].blocks[c].type), values, nulls))
    return out


def run_values(types, columns, nulls, partition, sort, orders, functions, sizes=None, device_input=False, output_mem=abi.MEM_HOST, op=None):
    """numpy columns (nulls[c]: a bool array or None) + a BIGINT input-position column behind them -> (input positions in output order,
    [(type, values, nulls or None) per function])"""
    op = op or make_operator(types, functions, partition, sort, orders, output_mem)
    feed_columns(op, types, columns, nulls, sizes, device_input)
    pages = drain(op)
    op.close()
    cols = output_columns(pages, 1 + len(functions))
    assert cols[0][2] is None
    return cols[0][1], cols[1:]


def check(types, columns, nulls, partition, sort, orders, functions, want=None, **kw):
    """the operator against value_model: which row stands where; a value column's NULLs and, bit for bit, the bytes of its sources; any other
    column by value"""
    total = len(columns[0])
    want = value_model(types, rows_of(types, columns, nulls), partition, sort, orders, functions) if want is None else want
    pos, cols = run_values(types, columns, nulls, partition, sort, orders, functions, **kw)
    assert pos.tolist() == [i for i, _ in want]
    for k, ((f, a, _), (t, values, null)) in enumerate(zip(framed(functions), cols)):
        w = [r[k] for _, r in want]
        got_null = np.zeros(total, bool) if null is None else null
        if f not in VALUE_FUNCTIONS:
            for at in range(total):
                g = None if got_null[at] else values[at].item()
                assert same_out(result_type(types, f, a), g, w[at]), (f, at, g, w[at])
            continue
        assert t == int(types[a[0]]), (f, t)                       # the result column has the value channel's type
        assert np.array_equal(got_null, np.array([x is None for x in w], bool)), (k, f, a)
        for ch in {x[0] for x in w if x is not None}:              # the value channel, and the default channel where it was taken
            sel = np.array([x is not None and x[0] == ch for x in w], bool)
            src = np.array([x[1] for x in w if x is not None and x[0] == ch], np.int64)
            assert values[sel].tobytes() == columns[ch][src].tobytes(), (k, f, a, ch)
    return pos, cols


def image(cols):
    """columns as bytes: equal images = the same types, values and NULLs"""
    return [(t, values.tobytes(), None if null is None else null.tobytes()) for t, values, null in cols]


def nullable(rng, total, rate):
    return rng.random(total) < rate


# ---- 1. known answers by hand ------------------------------------------------------------------------------------------------------------------
# channels: partition key, sort key, x, offset of lag / lead, default, offset of nth_value.  By sorted place:
#   partition 1: (10, 5, 1, 100, 1) (10, NULL, 2, NULL, 1) | (20, -3, NULL, 102, 3) | (30, 7, 0, 103, 5) (30, 2, 3, 104, 5)
#   partition 2: (5, NULL, 1, 200, 3) (5, NULL, 1, NULL, NULL) | (6, 4, 2, 202, 3)                   (| = a new peer group)
N_ = None
KAT_TYPES = [abi.BIGINT] * 6
KAT_SORTED = [(1, 10, 5, 1, 100, 1), (1, 10, N_, 2, N_, 1), (1, 20, -3, N_, 102, 3), (1, 30, 7, 0, 103, 5), (1, 30, 2, 3, 104, 5),
              (2, 5, N_, 1, 200, 3), (2, 5, N_, 1, N_, N_), (2, 6, 4, 2, 202, 3)]
KAT_ORDER = [2, 5, 7, 0, 3, 1, 6, 4]                     # the input row that stands at each sorted place; peers keep their arrival order
KAT = [((LAG, [2]), [N_, 5, N_, -3, 7, N_, N_, N_]),
       ((LEAD, [2]), [N_, -3, 7, 2, N_, N_, 4, N_]),
       ((LAG, [2, 3]), [N_, N_, N_, 7, N_, N_, N_, N_]),
       ((LAG, [2, 3, 4]), [100, N_, N_, 7, N_, 200, N_, N_]),
       ((LEAD, [2, 3, 4]), [N_, 7, N_, 7, 104, N_, 4, 202]),
       ((FIRST_VALUE, [2], ROWS), [5, 5, 5, 5, 5, N_, N_, N_]),
       ((FIRST_VALUE, [2], WHOLE), [5, 5, 5, 5, 5, N_, N_, N_]),
       ((LAST_VALUE, [2], ROWS), [5, N_, -3, 7, 2, N_, N_, 4]),
       ((LAST_VALUE, [2], RANGE), [N_, N_, -3, 2, 2, N_, N_, 4]),
       ((LAST_VALUE, [2], WHOLE), [2, 2, 2, 2, 2, 4, 4, 4]),
       ((NTH_VALUE, [2, 5], ROWS), [5, 5, -3, N_, 2, N_, N_, 4]),
       ((NTH_VALUE, [2, 5], RANGE), [5, 5, -3, 2, 2, N_, N_, 4]),
       ((NTH_VALUE, [2, 5], WHOLE), [5, 5, -3, 2, 2, 4, N_, 4])]
KAT_FUNCTIONS = [f for f, _ in KAT]


def kat_columns():
    rows = [None] * 8
    for place, i in enumerate(KAT_ORDER):
        rows[i] = KAT_SORTED[place]
    columns = [np.array([0 if r[c] is None else r[c] for r in rows], np.int64) for c in range(6)]
    nulls = [np.array([r[c] is None for r in rows], bool) for c in range(6)]
    return rows, columns, nulls


def test_the_model_reproduces_the_known_answers():
    """(the restatement itself against the answers worked out by hand: no GPU work)"""
    rows, _, _ = kat_columns()
    got = value_model(KAT_TYPES, rows, [0], [1], [ASC_NULLS_LAST], KAT_FUNCTIONS)
    assert [i for i, _ in got] == KAT_ORDER
    for k, (f, answer) in enumerate(KAT):
        assert [None if r[k] is None else rows[r[k][1]][r[k][0]] for _, r in got] == answer, f
    assert KAT[7][1] != KAT[8][1] and KAT[10][1] != KAT[11][1]                 # ROWS and RANGE differ where peers are tied
    for f, bad in ((LAG, -1), (LEAD, -1), (NTH_VALUE, 0)):
        with pytest.raises(BadOffset):
            value_model([abi.BIGINT] * 2, [(1, bad)], [], [], [], [(f, [0, 1])])
    assert value_model([abi.BIGINT] * 2, [(1, None)], [], [], [], [(NTH_VALUE, [0, 1])]) == [(0, [None])]


@pytest.mark.parametrize("device,output_mem", MODES)
def test_known_answers(gpu, device, output_mem):
    rows, columns, nulls = kat_columns()
    pos, cols = check(KAT_TYPES, columns, nulls, [0], [1], [ASC_NULLS_LAST], KAT_FUNCTIONS, sizes=[3, 0, 4], device_input=device, output_mem=output_mem)
    assert pos.tolist() == KAT_ORDER
    for (f, answer), (t, values, null) in zip(KAT, cols):
        assert t == abi.BIGINT and [None if null is not None and null[at] else int(values[at]) for at in range(8)] == answer, f
    # GROUPS .. CURRENT ROW is RANGE .. CURRENT ROW, the default frame is RANGE, and lag / lead do not read their frame
    odd = (abi.FRAME_ROWS, abi.BOUND_PRECEDING, abi.BOUND_FOLLOWING, 3, 3, 0)
    again = [(f[0], f[1], odd) if f[0] in (LAG, LEAD) else (f[0], f[1], GROUPS) if f[2] == RANGE else f for f in KAT_FUNCTIONS]
    _, other = run_values(KAT_TYPES, columns, nulls, [0], [1], [ASC_NULLS_LAST], again, device_input=device, output_mem=output_mem)
    default = [(f[0], f[1]) if len(f) > 2 and f[2] == RANGE else f for f in KAT_FUNCTIONS]
    _, third = run_values(KAT_TYPES, columns, nulls, [0], [1], [ASC_NULLS_LAST], default, device_input=device, output_mem=output_mem)
    assert image(other) == image(cols) and image(third) == image(cols)


# ---- 2. workgroup boundaries and the 64-bit offsets ------------------------------------------------------------------------------------------------
CONSTANT_OFFSETS = [0, 1, 255, 256, 257, BLOCK, 1 << 62, INT64_MAX]


def boundary_input(n, cut):
    """By sorted place: one partition (cut None), or a partition that ends at `cut` and another behind it.  Channels: partition key, sort
    key, x, the constant offsets, N - 1, N, then the offsets of nth_value under ROWS: 1, e + 1, e + 2."""
    at = np.arange(n, dtype=np.int64)
    part = np.zeros(n, np.int64) if cut is None else (at >= cut).astype(np.int64)
    first = np.where(part == 0, 0, cut if cut is not None else 0)
    size = np.bincount(part)[part]
    place = at - first
    rng = np.random.default_rng(n * 7 + (cut or 0))
    columns = [part, at.copy(), rng.integers(-1000, 1000, n).astype(np.int64)] + [np.full(n, v, np.int64) for v in CONSTANT_OFFSETS]
    columns += [size - 1, size.astype(np.int64), np.ones(n, np.int64), place + 1, place + 2]
    nulls = [None, None, nullable(rng, n, 0.1)] + [None] * (len(columns) - 3)
    shuffle = rng.permutation(n)                 # the sort has work to do
    return [c[shuffle] for c in columns], [None if nl is None else nl[shuffle] for nl in nulls]


# (a partition can end at `cut` only where rows stand behind it)
BOUNDARY_CASES = [(n, cut) for n in (1, 2, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 3) for cut in (None, BLOCK - 1, BLOCK, BLOCK + 1) if cut is None or cut < n]


@pytest.mark.parametrize("n,cut", BOUNDARY_CASES)
def test_workgroup_boundaries(gpu, n, cut):
    """offsets that cross lanes, waves and workgroups, reach exactly the first / last row of the partition and one past it, and the two
    that would overflow i +- offset"""
    columns, nulls = boundary_input(n, cut)
    types = [abi.BIGINT] * len(columns)
    offsets = list(range(3, 3 + len(CONSTANT_OFFSETS) + 2))
    nth = [(NTH_VALUE, [2, c], ROWS) for c in (offsets[-2] + 2, offsets[-2] + 3, offsets[-2] + 4, 3 + CONSTANT_OFFSETS.index(INT64_MAX))]
    check(types, columns, nulls, [0], [1], [ASC_NULLS_LAST], [(LAG, [2, c]) for c in offsets] + nth + [(LAST_VALUE, [2], WHOLE), (FIRST_VALUE, [2])])
    check(types, columns, nulls, [0], [1], [ASC_NULLS_LAST], [(LEAD, [2, c]) for c in offsets] + [(LEAD, [2, 4, 1]), (LAG, [2, 5, 1])],
          device_input=True, output_mem=abi.MEM_DEVICE)


# ---- 3. per-row offsets ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset_type", [abi.BIGINT, abi.INTEGER])
def test_per_row_offsets_with_nulls_and_a_default_with_nulls(gpu, offset_type):
    rng = np.random.default_rng(101 + int(offset_type))
    total = BLOCK + 200
    pool = np.array([0, 0, 1, 1, 2, 3, 7, 63, 64, 65, 300, total, 1 << 30], np.int64)
    columns = [rng.integers(0, 6, total).astype(np.int64), rng.integers(0, 50, total).astype(np.int64), rng.integers(-99, 99, total).astype(np.int64),
               pool[rng.integers(0, len(pool), total)].astype(DTYPES[offset_type]), rng.integers(1000, 2000, total).astype(np.int64),
               (1 + pool[rng.integers(0, len(pool), total)]).astype(DTYPES[offset_type])]
    nulls = [None, None, nullable(rng, total, 0.2), nullable(rng, total, 0.15), nullable(rng, total, 0.3), nullable(rng, total, 0.15)]
    types = [abi.BIGINT, abi.BIGINT, abi.BIGINT, offset_type, abi.BIGINT, offset_type]
    functions = [(LAG, [2, 3, 4]), (LEAD, [2, 3, 4]), (LAG, [2, 3]), (LEAD, [2, 3]), (NTH_VALUE, [2, 5], ROWS), (NTH_VALUE, [2, 5], RANGE), (NTH_VALUE, [2, 5], WHOLE)]
    _, cols = check(types, columns, nulls, [0], [1], [ASC_NULLS_LAST], functions, sizes=[500, 500])
    assert all(null is not None and null.any() and not null.all() for _, _, null in cols)


# ---- 4. every value type, bit for bit ---------------------------------------------------------------------------------------------------------------------
def typed_values(t, rng, total):
    """values of type t as the column holds them, the edge values among them"""
    if int(t) == abi.LONG_DECIMAL:
        v = rng.integers(0, 1 << 62, (total, 2)).astype(np.uint64)
        v[::3, 1] |= np.uint64(1 << 63)                           # negative: the sign is the top bit of the high word
        v[-1] = (0xFFFFFFFFFFFFFFFF, 0x7FFFFFFFFFFFFFFF)          # every magnitude bit set
        return v
    if int(t) == abi.DOUBLE:
        v = rng.integers(-8, 8, total).astype(np.float64) / 4
        v[::5] = -0.0
        bits = v.view(np.uint64)
        bits[1::7], bits[2::7] = NAN_BITS_64
        return v
    if int(t) == abi.REAL:
        v = rng.integers(-8, 8, total).astype(np.float32) / 4
        v[::5] = -0.0
        bits = v.view(np.uint32)
        bits[1::7], bits[2::7] = NAN_BITS_32
        return v
    if int(t) == abi.BOOLEAN:
        return rng.integers(0, 3, total).astype(np.uint8)         # a BOOLEAN byte of 2 stays 2
    if int(t) in (abi.BIGINT, abi.DECIMAL):
        v = rng.integers(-(1 << 40), 1 << 40, total).astype(np.int64)
        v[::4], v[1::9] = INT64_MIN, INT64_MAX
        return v
    v = rng.integers(-100000, 100000, total).astype(np.int32)
    v[::4] = -(1 << 31)
    return v


@pytest.mark.parametrize("t", VALUE_TYPES, ids=lambda t: repr(t) if isinstance(t, abi.DecimalType) else abi.TYPE_NAMES[int(t)])
def test_every_value_type_bit_for_bit(gpu, t):
    """all five functions and the default path over a channel of type t: the bytes of the source row"""
    rng = np.random.default_rng(201 + int(t) + abi.type_param(t))
    total = BLOCK + 77
    x, d = typed_values(t, rng, total), typed_values(t, rng, total)[::-1].copy()
    columns = [rng.integers(0, 9, total).astype(np.int64), rng.integers(0, 40, total).astype(np.int64), x, rng.integers(0, 5, total).astype(np.int64), d,
               rng.integers(1, 6, total).astype(np.int64)]
    types = [abi.BIGINT, abi.BIGINT, t, abi.BIGINT, t, abi.BIGINT]
    functions = [(LAG, [2]), (LEAD, [2, 3]), (LAG, [2, 3, 4]), (LEAD, [2, 3, 4]), (FIRST_VALUE, [2]), (LAST_VALUE, [2], ROWS), (LAST_VALUE, [2]),
                 (NTH_VALUE, [2, 5], WHOLE), (LAST_VALUE, [4], WHOLE)]
    for rate in (0.0, 0.2):
        nulls = [None, None, nullable(rng, total, rate), None, nullable(rng, total, rate), None]
        pos, cols = check(types, columns, nulls, [0], [1], [DESC_NULLS_LAST], functions, sizes=[400], device_input=rate > 0, output_mem=int(rate > 0))
        if rate == 0:                            # last_value over ROWS is the channel itself: every edge value comes through
            assert cols[5][1].tobytes() == x[pos].tobytes() and (cols[5][2] is None or not cols[5][2].any())
    if int(t) == abi.DOUBLE:
        assert {int(b) for b in x.view(np.uint64)} >= set(NAN_BITS_64) | {1 << 63}
    if int(t) == abi.BOOLEAN:
        assert 2 in x


# ---- 5. identities that need no model ------------------------------------------------------------------------------------------------------------------------
def test_identities(gpu):
    rng = np.random.default_rng(301)
    total = 2 * BLOCK + 301
    part, key = rng.integers(0, 25, total).astype(np.int64), rng.integers(0, 12, total).astype(np.int64)
    x = typed_values(abi.DOUBLE, rng, total)
    x_null = nullable(rng, total, 0.2)
    zero, one = np.zeros(total, np.int64), np.ones(total, np.int64)
    types = [abi.BIGINT, abi.BIGINT, abi.DOUBLE, abi.BIGINT, abi.BIGINT]
    functions = [(LAG, [2, 3]), (LEAD, [2, 3]), (LAST_VALUE, [2], ROWS), (FIRST_VALUE, [2], WHOLE), (NTH_VALUE, [2, 4], WHOLE), (LAG, [2, 4]), (LEAD, [2, 4]),
                 ROW_NUMBER, (COUNT_STAR, [], WHOLE), (LAG, [2]), (LEAD, [2]), (FIRST_VALUE, [2], ROWS), (FIRST_VALUE, [2], RANGE)]
    pos, cols = run_values(types, [part, key, x, zero, one], [None, None, x_null, None, None], [0], [1], [ASC_NULLS_LAST], functions, sizes=[1000, 1000],
                           device_input=True, output_mem=abi.MEM_DEVICE)

    def image(k):                                # a column as (bits where not NULL, NULLs)
        _, values, null = cols[k]
        null = np.zeros(total, bool) if null is None else null
        return np.where(null, 0, values.view(np.uint64)), null

    def same(a, b):
        return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])

    itself = (np.where(x_null[pos], 0, x[pos].view(np.uint64)), x_null[pos])
    assert same(image(0), itself) and same(image(1), itself) and same(image(2), itself)            # lag(x, 0) = lead(x, 0) = last_value ROWS = x
    assert same(image(3), image(4)) and same(image(3), image(11)) and same(image(3), image(12))    # first_value = nth_value(x, 1); any frame
    assert same(image(5), image(9)) and same(image(6), image(10))                                  # the offset is 1 without a channel
    # lag(x, 1) at place i + 1 = x at place i = lead(x, 1) at place i - 1, inside a partition
    place, size = cols[7][1] - 1, cols[8][1]
    lag, lead = image(5), image(6)
    inner = place > 0
    assert np.array_equal(lag[0][inner], itself[0][np.flatnonzero(inner) - 1]) and np.array_equal(lag[1][inner], itself[1][np.flatnonzero(inner) - 1])
    assert lag[1][~inner].all()
    inner = place < size - 1
    assert np.array_equal(lead[0][inner], itself[0][np.flatnonzero(inner) + 1]) and np.array_equal(lead[1][inner], itself[1][np.flatnonzero(inner) + 1])
    assert lead[1][~inner].all()
    two_apart = place < size - 2
    at = np.flatnonzero(two_apart)
    assert np.array_equal(lead[0][at], lag[0][at + 2]) and np.array_equal(lead[1][at], lag[1][at + 2])


# ---- 6. mixed functions ---------------------------------------------------------------------------------------------------------------------------------------
def test_rank_and_sum_are_bit_for_bit_what_they_are_without_the_lag(gpu):
    rng = np.random.default_rng(401)
    total = 2 * BLOCK + 17
    columns = [rng.integers(0, 40, total).astype(np.int64), rng.integers(0, 9, total).astype(np.int64), rng.integers(-1000, 1000, total).astype(np.int64)]
    nulls = [None, None, nullable(rng, total, 0.2)]
    types = [abi.BIGINT] * 3

    def raw(functions):
        op = make_operator(types, functions, [0], [1], [DESC_NULLS_FIRST])
        feed_columns(op, types, columns, nulls, [1500])
        out = raw_columns(drain(op))
        op.close()
        return out

    plain = raw([RANK, (SUM, [2], ROWS)])
    mixed = raw([(LAG, [2]), RANK, (LAST_VALUE, [2]), (SUM, [2], ROWS), (LEAD, [2, 1, 2])])
    assert mixed[0] == plain[0] and mixed[2] == plain[1] and mixed[4] == plain[2]
    check(types, columns, nulls, [0], [1], [DESC_NULLS_FIRST], [(LAG, [2]), RANK, (LAST_VALUE, [2]), (SUM, [2], ROWS), (LEAD, [2, 1, 2])])


def test_sixteen_functions_at_once(gpu):
    rng = np.random.default_rng(402)
    total = BLOCK + 9
    columns = [rng.integers(0, 7, total).astype(np.int64), rng.integers(0, 30, total).astype(np.int64), rng.integers(-50, 50, total).astype(np.int64),
               rng.integers(0, 4, total).astype(np.int32), typed_values(abi.REAL, rng, total), rng.integers(1, 5, total).astype(np.int64)]
    nulls = [None, None, nullable(rng, total, 0.2), nullable(rng, total, 0.1), nullable(rng, total, 0.2), None]
    types = [abi.BIGINT, abi.BIGINT, abi.BIGINT, abi.INTEGER, abi.REAL, abi.BIGINT]
    functions = [(LAG, [2]), (LEAD, [4]), (LAG, [2, 3]), (LEAD, [4, 3, 4]), (FIRST_VALUE, [2]), (FIRST_VALUE, [4], ROWS), (LAST_VALUE, [2], ROWS), (LAST_VALUE, [4]),
                 (LAST_VALUE, [2], WHOLE), (NTH_VALUE, [4, 5], WHOLE), (NTH_VALUE, [2, 5], ROWS), RANK, (SUM, [2], ROWS), (MIN, [4]), (NTILE, [5]), (LAG, [2])]
    assert len(functions) == 16
    _, cols = check(types, columns, nulls, [0], [1], [ASC_NULLS_FIRST], functions, sizes=[300, 0, 300])
    assert image(cols[:1]) == image(cols[15:])


# ---- 7. segment hygiene ------------------------------------------------------------------------------------------------------------------------------------------
def test_nothing_is_picked_up_from_the_neighbouring_partition(gpu):
    """two adjacent partitions whose rows differ only in x: a lag / lead / nth_value that ignored the partition bound would show the other's"""
    types = [abi.BIGINT, abi.BIGINT, abi.BIGINT, abi.BIGINT]
    columns = [np.array([1, 1, 1, 2, 2, 2], np.int64), np.array([1, 2, 3, 1, 2, 3], np.int64), np.array([11, 12, 13, 21, 22, 23], np.int64), np.array([4, 4, 4, 4, 4, 4], np.int64)]
    nulls = [None] * 4
    functions = [(LAG, [2]), (LEAD, [2]), (FIRST_VALUE, [2]), (LAST_VALUE, [2], WHOLE), (NTH_VALUE, [2, 3], WHOLE), (NTH_VALUE, [2, 1], WHOLE)]
    _, cols = check(types, columns, nulls, [0], [1], [ASC_NULLS_LAST], functions)
    got = [[None if null is not None and null[at] else int(values[at]) for at in range(6)] for _, values, null in cols]
    assert got == [[None, 11, 12, None, 21, 22], [12, 13, None, 22, 23, None], [11] * 3 + [21] * 3, [13] * 3 + [23] * 3, [None] * 6, [11, 12, 13, 21, 22, 23]]
    # the same around a workgroup boundary, with a descending sort
    n = BLOCK + 40
    at = np.arange(n, dtype=np.int64)
    columns = [(at >= BLOCK - 1).astype(np.int64), at % 17 + 1, at * 10, np.full(n, 4, np.int64)]
    check(types, columns, nulls, [0], [1], [DESC_NULLS_LAST], functions + [(LAG, [2, 3]), (LEAD, [2, 3])])


@pytest.mark.parametrize("order", [ASC_NULLS_FIRST, ASC_NULLS_LAST, DESC_NULLS_FIRST, DESC_NULLS_LAST])
def test_null_partition_keys_and_every_sort_order(gpu, order):
    rng = np.random.default_rng(501)
    total = 300
    columns = [rng.integers(0, 4, total).astype(np.int64), rng.integers(-5, 6, total).astype(np.int64), rng.integers(0, 1000, total).astype(np.int64),
               rng.integers(0, 4, total).astype(np.int64)]
    nulls = [nullable(rng, total, 0.2), nullable(rng, total, 0.3), nullable(rng, total, 0.2), None]
    functions = [(LAG, [2, 3]), (LEAD, [2, 3, 2]), (FIRST_VALUE, [2], RANGE), (LAST_VALUE, [2], RANGE), (LAST_VALUE, [1], ROWS)]
    check([abi.BIGINT] * 4, columns, nulls, [0], [1], [order], functions, sizes=[100, 100])
    check([abi.BIGINT] * 4, columns, nulls, [], [], [], functions)                       # no partition, no order: arrival order


# ---- 8. offset errors ------------------------------------------------------------------------------------------------------------------------------------------------
def offset_status(function, offsets, offset_nulls=None, offset_type=abi.BIGINT):
    """status and message of pa_op_get_output after finish; nothing is emitted, and the operator is closed and destroyed.  The rows
    arrive sorted, so the last rows of the input stand in the last workgroup."""
    n = len(offsets)
    op = FramedWindowOperator([abi.BIGINT, offset_type], [0], [ROW_NUMBER, (function, [0, 1], WHOLE)], [0], [0], [ASC_NULLS_LAST])
    op.addInput(Page([Block.bigint(np.arange(n, dtype=np.int64) // 300), Block.flat(offset_type, offsets, offset_nulls)], n))
    op.finish()
    out = abi.pa_page()
    status = lib().pa_op_get_output(op._h, C.byref(out))
    message = lib().pa_last_error() if status < 0 else b""
    if status < 0:
        assert op.getOutput() is None and op.isFinished()
    op.close()
    return status, message


@pytest.mark.parametrize("offset_type", [abi.BIGINT, abi.INTEGER])
def test_bad_offsets(gpu, offset_type):
    """one bad offset somewhere in the last workgroup: PA_ERR_INVALID_ARGUMENT with the reference's message (a data error reported through
    the error word: nothing faults)"""
    n = 2 * BLOCK + 5
    for function, bad, message in ((LAG, -1, b"Offset must be at least 0"), (LEAD, -7, b"Offset must be at least 0"), (NTH_VALUE, 0, b"Offset must be at least 1"),
                                   (NTH_VALUE, -3, b"Offset must be at least 1")):
        offsets = np.full(n, 2, DTYPES[offset_type])
        assert offset_status(function, offsets, offset_type=offset_type)[0] >= 0
        offsets[n - 2] = bad
        status, text = offset_status(function, offsets, offset_type=offset_type)
        assert status == abi.ERR_INVALID_ARGUMENT and message in text, (function, bad)
        with pytest.raises(BadOffset):
            value_model([abi.BIGINT] * 2, [(1, bad)], [0], [0], [ASC_NULLS_LAST], [(function, [0, 1], WHOLE)])
        # a NULL offset that holds the bad value is not one, also next to good ones
        nulls = np.zeros(n, np.uint8)
        nulls[n - 2] = 1
        assert offset_status(function, offsets, nulls, offset_type)[0] >= 0
    assert offset_status(LAG, np.array([0], DTYPES[offset_type]), offset_type=offset_type)[0] >= 0      # 0 is an offset of lag, not of nth_value
    assert offset_status(NTH_VALUE, np.array([1], DTYPES[offset_type]), offset_type=offset_type)[0] >= 0


# ---- 9. page cuts, memory spaces, reuse through the factory -----------------------------------------------------------------------------------------------------------
def test_page_cuts_and_memory_spaces_do_not_change_the_output(gpu):
    rng = np.random.default_rng(601)
    total = 60
    types = [abi.BIGINT, abi.DOUBLE, abi.decimal(30, 2), abi.BIGINT, abi.decimal(30, 2)]
    columns = [rng.integers(0, 6, total).astype(np.int64), rng.integers(0, 5, total).astype(np.float64) / 2, typed_values(types[2], rng, total),
               rng.integers(0, 4, total).astype(np.int64), typed_values(types[2], rng, total)]
    nulls = [None, nullable(rng, total, 0.2), nullable(rng, total, 0.2), nullable(rng, total, 0.1), nullable(rng, total, 0.2)]
    functions = [(LAG, [2, 3, 4]), (LEAD, [1]), RANK, (LAST_VALUE, [2]), (NTH_VALUE, [1, 3], WHOLE)]
    columns[3] += 1                                                   # (also nth_value's offset: at least 1)
    outputs = []
    for sizes in ([60], [7, 0, 40], [1] * 60):
        for device, output_mem in MODES:
            outputs.append(check(types, columns, nulls, [0], [1], [DESC_NULLS_LAST], functions, sizes=sizes, device_input=device, output_mem=output_mem))
    assert all(np.array_equal(pos, outputs[0][0]) and image(cols) == image(outputs[0][1]) for pos, cols in outputs)


def test_operators_of_one_factory(gpu):
    """the factory is reused: every operator it creates gives the same columns, and a finished one does not disturb the next"""
    rng = np.random.default_rng(602)
    total = BLOCK + 1
    types = [abi.BIGINT, abi.BIGINT, abi.REAL]
    columns = [rng.integers(0, 5, total).astype(np.int64), rng.integers(0, 100, total).astype(np.int64), typed_values(abi.REAL, rng, total)]
    nulls = [None, None, nullable(rng, total, 0.2)]
    functions = [(LEAD, [2, 0]), (FIRST_VALUE, [2]), (LAST_VALUE, [2], WHOLE)]
    factory = FramedWindowOperatorFactory(types + [abi.BIGINT], [3], functions, [0], [1], [ASC_NULLS_LAST], output_mem=abi.MEM_DEVICE)
    first = check(types, columns, nulls, [0], [1], [ASC_NULLS_LAST], functions, op=factory.createOperator())
    a, b = factory.createOperator(), factory.createOperator()           # two at once, fed in turn
    feed_columns(a, types, columns, nulls, [100])
    feed_columns(b, types, columns, nulls, [900], device_input=True)
    for op in (b, a):
        got = output_columns(drain(op), 4)
        op.close()
        assert np.array_equal(got[0][1], first[0]) and image(got[1:]) == image(first[1])


# ---- 10. seeded fuzz -----------------------------------------------------------------------------------------------------------------------------------------------------
TAKEN_FRAMES = FRAMES                                                  # ROWS, RANGE, GROUPS .. CURRENT ROW and the three whole-partition frames
ANY_FRAMES = FRAMES + [(abi.FRAME_ROWS, abi.BOUND_PRECEDING, abi.BOUND_FOLLOWING, 0, 0, 0), (abi.FRAME_RANGE, abi.BOUND_CURRENT_ROW, abi.BOUND_CURRENT_ROW)]


@pytest.mark.parametrize("seed", range(30))
def test_fuzz(gpu, seed):
    """channels 0 .. 2: keys (BIGINT, INTEGER, DOUBLE); 3, 4: BIGINT / INTEGER offsets >= 1 (so they serve nth_value too); 5 .. 8: two pairs of
    value channels of random types, each pair one type (a value and its default).  Every generated shape is one the device path takes."""
    rng = np.random.default_rng(9000 + seed)
    total = int(rng.integers(1, 700))
    pair = [VALUE_TYPES[int(k)] for k in rng.integers(0, len(VALUE_TYPES), 2)]
    types = [abi.BIGINT, abi.INTEGER, abi.DOUBLE, abi.BIGINT, abi.INTEGER, pair[0], pair[0], pair[1], pair[1]]
    high = int(rng.choice([2, 5, 400]))
    columns = [rng.integers(0, int(rng.choice([1, 3, 200])), total).astype(np.int64), rng.integers(0, 3, total).astype(np.int32),
               rng.integers(0, int(rng.choice([1, 3, 40])), total).astype(np.float64) / 4, rng.integers(1, high, total).astype(np.int64),
               rng.integers(1, high, total).astype(np.int32)] + [typed_values(t, rng, total) for t in types[5:]]
    rate = float(rng.choice([0.0, 0.1, 0.9]))
    nulls = [None if rate == 0.0 or (c < 3 and rate > 0.5) else nullable(rng, total, rate) for c in range(len(types))]
    partition = [[0], [0, 1], []][int(rng.integers(0, 3))]
    sort = [[2], [2, 1], [], [3]][int(rng.integers(0, 4))]
    orders = [int(rng.integers(0, 4)) for _ in sort]
    functions = []
    for _ in range(int(rng.integers(1, 17))):
        f = int(rng.choice([LAG, LEAD, FIRST_VALUE, LAST_VALUE, NTH_VALUE, LAG, LEAD, RANK, SUM, COUNT]))
        value = 5 + 2 * int(rng.integers(0, 2))
        offset = 3 + int(rng.integers(0, 2))
        frame = TAKEN_FRAMES[int(rng.integers(0, len(TAKEN_FRAMES)))]
        if f in (LAG, LEAD):
            args = [[value], [value, offset], [value, offset, value + 1], [value + 1, offset, value]][int(rng.integers(0, 4))]
            functions.append((f, args, ANY_FRAMES[int(rng.integers(0, len(ANY_FRAMES)))]))
        elif f == NTH_VALUE:
            functions.append((f, [value + int(rng.integers(0, 2)), offset], frame))
        elif f in (FIRST_VALUE, LAST_VALUE):
            functions.append((f, [int(rng.choice([value, value + 1, 0, 2, 3]))], frame))
        elif f == RANK:
            functions.append((RANK, [], frame))
        else:
            functions.append((f, [3], frame))                          # (sums of at most 700 x 400: far from int64's ends)
    sizes = [int(s) for s in rng.integers(1, max(2, total // 2), int(rng.integers(1, 6)))]
    check(types, columns, nulls, partition, sort, orders, functions, sizes=sizes, device_input=bool(rng.integers(0, 2)), output_mem=int(rng.integers(0, 2)))
