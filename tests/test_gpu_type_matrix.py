"""Every (operator, role, type) pair of the operators that take their input types unchecked by an expression compiler: the pair is
either computed EXACTly -- compared here, by value and by bit pattern, with a plain Python reference over Page.to_rows() -- or REFUSED
with NOT_SUPPORTED when the operator is created (pa_hash_page and pa_page_serialize, which have no creation step: at the call), before
a row is produced.  There is no third state: a declared type never yields rows that were not computed for it.

MATRIX below is the whole classification ("Operator x type support", mirrors it).  It is looked up by the names in
abi.TYPE_NAMES, so a type added to the ABI fails every row here until it has been classified.

Reference rules (all restated in this file, none taken from the C oracle except the row hash of the types it restates from the
reference):
  sort     stable sort under SortOrder (oracle.topn's docstring): NULLS FIRST / LAST independent of ASC / DESC; integers, DATE and
           decimals (by unscaled value) numeric, DOUBLE / REAL in Double.compare order (-0.0 < 0.0, NaN above everything), VARCHAR by
           unsigned bytes with a proper prefix first, BOOLEAN false < true; rows that compare equal stay in arrival order, which the
           trailing arrival-index channel pins
  join     key -> build positions, matches of a probe row in descending build position, probe rows in order; NULL keys and NaN match
           nothing, -0.0 matches 0.0; PROBE_OUTER emits an unmatched probe row once with NULL build channels
  dynamic  the distinct non-NULL, non-NaN values ascending (one zero for -0.0 / 0.0) while they are at most max_distinct_values, their
  filter   [min, max] beyond that for the types that are not floating point, TupleDomain.all for those that are
  hash     InterpretedHashGenerator: 31 * h + hash(value), NULL = 0 -- oracle.hash_page; LONG_DECIMAL pinned by hand-computed values
"""
import ctypes as C
import functools
import math
import struct

import numpy as np
import pytest

from presto_amd import abi
from presto_amd._lib import DeviceAllocation, PrestoAmdError, check, lib
from presto_amd.expr import field
from presto_amd.operators import (Driver, DynamicFilterSourceOperator, FusedJoinOperator, HashBuilderOperator, LookupJoinOperator,
                                  LookupSourceFactory, Operator, OrderByOperator, TopNOperator, download, download_page, to_pages, upload_page)
from presto_amd.page import Block, DeviceBuffer, Page, deserialize_page, serialize_page

on_gpu = pytest.mark.gpu
per_type = pytest.mark.parametrize("name", list(abi.TYPE_NAMES))

EXACT, REFUSED = "EXACT", "REFUSED"
E, R = EXACT, REFUSED
COLUMNS = ["BIGINT", "INTEGER", "DATE", "DOUBLE", "BOOLEAN", "VARCHAR", "ROW", "REAL", "DECIMAL", "LONG_DECIMAL"]


def _row(*states):
    assert len(states) == len(COLUMNS)
    return dict(zip(COLUMNS, states))


# (operator, role) ->        BIGINT INTEGER DATE DOUBLE BOOLEAN VARCHAR ROW REAL DECIMAL LONG_DECIMAL
MATRIX = {
    ("order_by", "sort_key"):        _row(E, E, E, E, E, E, R, E, E, R),
    ("order_by", "payload"):         _row(E, E, E, E, E, E, R, E, E, E),
    ("topn", "sort_key_first"):      _row(E, E, E, E, E, E, R, E, E, R),
    ("topn", "sort_key_second"):     _row(E, E, E, E, E, E, R, E, E, R),
    ("topn", "payload"):             _row(E, E, E, E, E, E, R, E, E, E),
    ("join", "join_key"):            _row(E, E, E, E, E, E, R, E, E, R),
    ("join", "build_payload"):       _row(E, E, E, E, E, E, R, E, E, E),
    ("join", "probe_payload"):       _row(E, E, E, E, E, E, R, E, E, E),
    ("dynamic_filter", "filter"):    _row(E, E, E, E, E, E, R, E, E, R),
    ("dynamic_filter", "pass"):      _row(E, E, E, E, E, E, R, E, E, E),
    ("hash_page", "hashed"):         _row(E, E, E, E, E, E, R, E, E, E),
    ("exchange", "partition"):       _row(E, E, E, E, E, E, R, R, R, R),
    ("exchange", "carried"):         _row(E, E, E, E, E, E, R, R, R, R),
    ("serde", "channel"):            _row(E, E, E, E, E, E, R, E, R, R),
}

# the type as a descriptor names it: decimals carry their parameters (DECIMAL(18, 2) is the widest short decimal)
TYPE_OF = {"BIGINT": abi.BIGINT, "INTEGER": abi.INTEGER, "DATE": abi.DATE, "DOUBLE": abi.DOUBLE, "BOOLEAN": abi.BOOLEAN, "VARCHAR": abi.VARCHAR,
           "ROW": abi.ROW, "REAL": abi.REAL, "DECIMAL": abi.decimal(18, 2), "LONG_DECIMAL": abi.decimal(38, 2)}

CELLS = [(op, role, name) for (op, role) in MATRIX for name in abi.TYPE_NAMES]


def state(op, role, name):
    return MATRIX[(op, role)][name]   # KeyError: a type of the ABI that this table does not classify yet


def test_every_cell_is_classified():
    assert sorted(COLUMNS) == sorted(abi.TYPE_NAMES) and sorted(TYPE_OF) == sorted(abi.TYPE_NAMES)
    for op, role, name in CELLS:
        assert state(op, role, name) in (EXACT, REFUSED), (op, role, name)
    for key in MATRIX:
        assert MATRIX[key]["ROW"] == REFUSED, key
    # what the project requires to be exact: a short decimal wherever BIGINT is, except through exchange and serde; LONG_DECIMAL and
    # REAL as payload of sorts and joins
    for key in MATRIX:
        if key[0] not in ("exchange", "serde"):
            assert MATRIX[key]["DECIMAL"] == MATRIX[key]["BIGINT"] == EXACT, key
    for key in [("order_by", "payload"), ("topn", "payload"), ("join", "build_payload"), ("join", "probe_payload")]:
        assert MATRIX[key]["LONG_DECIMAL"] == MATRIX[key]["REAL"] == EXACT, key


def refused(create):
    """NOT_SUPPORTED, by status: from the factory call (or, without one, the call itself)."""
    with pytest.raises(PrestoAmdError) as e:
        create()
    assert e.value.status == abi.ERR_NOT_SUPPORTED, e.value


# ---- values -------------------------------------------------------------------------------------------------------------------------------
M64 = (1 << 64) - 1
LD_STEP = 0x0123456789ABCDEF0123   # every byte of a 16-byte element matters: +-(i * LD_STEP + 7)
f32 = lambda v: float(np.float32(v))
EDGES = {
    "BIGINT": [0, 1, -1, 2 ** 63 - 1, -2 ** 63, 0x0123456789ABCDEF, -0x0123456789ABCDEF, 1 << 32, -(1 << 32)],
    "INTEGER": [0, 1, -1, 2 ** 31 - 1, -2 ** 31, 0x01234567, -0x01234567, 1 << 16],
    "DATE": [0, 1, -1, 2 ** 31 - 1, -2 ** 31, 9000, 19000, -719162],
    "DOUBLE": [0.0, -0.0, float("nan"), float("inf"), float("-inf"), 1.5, -1.5, 5e-324, -5e-324, 1.7976931348623157e308,
               struct.unpack("<d", struct.pack("<Q", 0x0123456789ABCDEF))[0]],
    "REAL": [f32(v) for v in (0.0, -0.0, float("nan"), float("inf"), float("-inf"), 1.5, -1.5, 1e-45, -1e-45, 3.4028235e38, 16777217.0)],
    "BOOLEAN": [True, False],
    # equal first 8 bytes with different lengths and tails (the 64-bit image of a string is its first 8 bytes), the empty string, high bytes
    "VARCHAR": [b"", b"a", b"ab", b"abcdefgh", b"abcdefghi", b"abcdefgh\x00", b"abcdefghj", b"abcdefg", b"\xff\xfe", b"zz" * 10, b"\x00"],
    # as doubles the bits of -1, -2, -3 are NaNs and those of 0 a zero; DECIMAL(18, s) ends at +-(10^18 - 1), so -2^63 (the bits of -0.0)
    # is out of its range: -(10^18 - 1) is the nearest it holds
    "DECIMAL": [0, 1, -1, -2, -3, 10 ** 18 - 1, -(10 ** 18 - 1), 12345, -12345, 0x0123456789ABCDE, -0x0123456789ABCDE],
    "LONG_DECIMAL": [0, 7, -7, 10 ** 38 - 1, -(10 ** 38 - 1), 1 << 64, -(1 << 64), (1 << 64) + 1, (1 << 64) - 1, LD_STEP + 7, -(LD_STEP + 7)],
}


def random_value(name, rng, i):
    if name == "BIGINT":
        return int(rng.integers(-2 ** 62, 2 ** 62))
    if name == "INTEGER":
        return int(rng.integers(-2 ** 31, 2 ** 31 - 1))
    if name == "DATE":
        return int(rng.integers(-100000, 100000))
    if name == "DOUBLE":
        return float(rng.standard_normal() * 10.0 ** int(rng.integers(-20, 20)))
    if name == "REAL":
        return f32(rng.standard_normal() * 10.0 ** int(rng.integers(-10, 10)))
    if name == "BOOLEAN":
        return bool(rng.integers(0, 2))
    if name == "VARCHAR":
        return bytes(rng.integers(0, 256, int(rng.integers(0, 21)), dtype=np.uint8).tolist()) if i % 3 else b"abcdefgh" + str(i).encode()
    if name == "DECIMAL":
        return int(rng.integers(-(10 ** 18 - 1), 10 ** 18 - 1)) if i % 2 else int(rng.integers(-1000, 1000))
    if name == "LONG_DECIMAL":
        return (-1 if i % 2 else 1) * ((i + 1) * LD_STEP + 7)
    raise KeyError(name)


def equality_key(v):
    """identity under the type's EQUAL: None for what equals nothing (NULL, NaN); 0.0 and -0.0 are one key (== in Python too)"""
    if v is None or (isinstance(v, float) and math.isnan(v)):
        return None
    return v


def distinct_pool(name, count, seed):
    """up to `count` values of the type, pairwise different under EQUAL, the edge values first (BOOLEAN has two)"""
    rng = np.random.default_rng(seed)
    pool, seen = [], set()
    i = 0
    limit = 2 if name == "BOOLEAN" else count
    candidates = iter(EDGES[name])
    while len(pool) < limit:
        v = next(candidates, None)
        if v is None:
            v = random_value(name, rng, i)
            i += 1
        k = equality_key(v)
        if k is None or k in seen:
            continue
        seen.add(k)
        pool.append(v)
    return pool


def draw(name, n, seed, null_rate=0.05, pool=None, nan=True):
    """n values (None = NULL): from `pool`, or the edge values and random ones"""
    rng = np.random.default_rng(seed)
    if pool is None:
        pool = EDGES[name] + [random_value(name, rng, i) for i in range(min(n, 997))]
    picks = rng.integers(0, len(pool), n).tolist()
    nulls = (rng.random(n) < null_rate).tolist()
    out = [None if z else pool[p] for p, z in zip(picks, nulls)]
    if nan and name in ("DOUBLE", "REAL") and n > 3:   # whatever the pool holds: a NaN and both zeros
        out[n // 2], out[n // 2 + 1], out[n // 2 - 1] = float("nan"), -0.0, 0.0
    return out


def block_of(name, values):
    nulls = [v is None for v in values]
    if name == "VARCHAR":
        return Block.varchar(values)
    if name == "LONG_DECIMAL":
        return Block.long_decimal(values)
    if name == "BOOLEAN":
        return Block.boolean([bool(v) for v in values], nulls)
    zero = 0.0 if name in ("DOUBLE", "REAL") else 0
    return Block.flat(TYPE_OF[name], [zero if v is None else v for v in values], nulls)


def pages_of(names, columns, cuts):
    """columns of values -> host pages of cuts[i] rows"""
    pages, at = [], 0
    for m in cuts:
        if m:
            pages.append(Page([block_of(nm, col[at:at + m]) for nm, col in zip(names, columns)], m))
        at += m
    assert at == len(columns[0])
    return pages


def row_page():
    return Page([Block.bigint([1, 2, 3]), Block.row([Block.bigint([4, 5, 6]), Block.varchar([b"x", None, b"z"])], None)], 3)


def bits(rows):
    """rows compared by bit pattern: a float as the 8 bytes of the double to_rows gave (NaN equals NaN, -0.0 differs from 0.0)"""
    return [tuple(struct.pack("<d", v) if isinstance(v, float) else v for v in r) for r in rows]


def rows_of(pages):
    return [r for p in pages for r in (p if p.mem == abi.MEM_HOST else download_page(p)).to_rows()]


def types_of(names):
    return [TYPE_OF[n] for n in names]


# ---- sort ---------------------------------------------------------------------------------------------------------------------------------
ORDERS = [abi.ASC_NULLS_FIRST, abi.ASC_NULLS_LAST, abi.DESC_NULLS_FIRST, abi.DESC_NULLS_LAST]


def image(name, v):
    if name in ("DOUBLE", "REAL"):   # Double.compare (RealType: Float.compare, the same order on the widened value)
        b = 0x7ff8000000000000 if math.isnan(v) else struct.unpack("<Q", struct.pack("<d", v))[0]
        return (~b) & M64 if b >> 63 else b | (1 << 63)
    return v


def sorted_rows(rows, names, sort_channels, sort_orders):
    """stable, least significant channel first; reverse=True keeps equal rows in their order as well"""
    rows = list(rows)
    for ch, order in reversed(list(zip(sort_channels, sort_orders))):
        descending, nulls_first = order >= 2, (order & 1) == 0
        values = [r for r in rows if r[ch] is not None]
        nulls = [r for r in rows if r[ch] is None]
        values.sort(key=lambda r: image(names[ch], r[ch]), reverse=descending)
        rows = nulls + values if nulls_first else values + nulls
    return rows


def sort_case(role, name, n, seed, few_first=False):
    """(names, columns, sort channels): the trailing BIGINT channel is the arrival index"""
    arrival = list(range(n))
    tied = lambda nm, distinct, nulls, k: draw(nm, n, seed + k, nulls, pool=distinct_pool(nm, distinct, seed))
    if role in ("sort_key", "sort_key_first"):
        # ties on the key: a third as many distinct values as rows, or -- few_first -- three, so that the second channel decides
        return [name, "BIGINT", "BIGINT"], [tied(name, 3 if few_first else max(n // 3, 2), 0.05, 1), tied("BIGINT", 50, 0.0, 2), arrival], [0, 1]
    if role == "sort_key_second":
        return ["BIGINT", name, "BIGINT"], [tied("BIGINT", 3, 0.0, 1), tied(name, max(n // 3, 2), 0.05, 2), arrival], [0, 1]
    return ["BIGINT", name, "BIGINT"], [tied("BIGINT", max(n // 3, 2), 0.0, 1), draw(name, n, seed + 2, 0.1), arrival], [0]


def refused_sort(make, role, name):
    t = TYPE_OF[name]
    if role in ("sort_key", "sort_key_first"):
        refused(lambda: make([t, abi.BIGINT], [0], [abi.ASC_NULLS_LAST]))
    elif role == "sort_key_second":
        refused(lambda: make([abi.BIGINT, t, abi.BIGINT], [0, 1], [abi.ASC_NULLS_LAST, abi.DESC_NULLS_FIRST]))
    else:
        refused(lambda: make([abi.BIGINT, t], [0], [abi.ASC_NULLS_LAST]))


@on_gpu
@pytest.mark.parametrize("role", ["sort_key", "payload"])
@per_type
def test_order_by(gpu, role, name):
    """n = 1, 2049 (one past a single LDS bucket of the sort), 5000, in two pages; all four SortOrders; with and without NULL rows in
    the payload (a channel without NULLs can ride with the sort's pairs, one with NULLs is gathered)."""
    if state("order_by", role, name) == REFUSED:
        return refused_sort(lambda types, sc, so: OrderByOperator(types, list(range(len(types))), sc, so), role, name)
    for n in (1, 2049, 5000):
        names, columns, sort_channels = sort_case(role, name, n, 100 + n)
        if role == "sort_key":
            sort_channels = [0]
        variants = [columns]
        if role == "payload":
            variants.append([columns[0], draw(name, n, n + 3, 0.0), columns[2]])
        for cols in variants:
            pages = pages_of(names, cols, [(n + 1) // 2, n // 2])
            rows = rows_of(pages)
            for order in ORDERS:
                orders = [order] * len(sort_channels)
                op = OrderByOperator(types_of(names), [0, 1, 2], sort_channels, orders)
                got = rows_of(to_pages(op, pages))
                op.close()
                assert bits(got) == bits(sorted_rows(rows, names, sort_channels, orders)), (n, order)


@functools.lru_cache(maxsize=2)
def topn_input(role, name, shape):
    if shape == "pages":       # the first page (> 2^14 rows) goes the exact way, the later ones under the bound carried over
        n, cuts, few = 60000, [20000, 20000, 20000], False
    elif shape == "sampled":   # >= 4 * 2^14 rows: the bound comes from a sample
        n, cuts, few = 70001, [70001], False
    else:                      # few distinct first keys: the second sort channel decides, on the host comparator
        n, cuts, few = 60000, [20000, 20000, 20000], True
    names, columns, sort_channels = sort_case(role, name, n, 7 + len(shape), few_first=few)
    pages = pages_of(names, columns, cuts)
    return names, pages, rows_of(pages), sort_channels


@on_gpu
@pytest.mark.parametrize("role", ["sort_key_first", "sort_key_second", "payload"])
@per_type
def test_topn(gpu, role, name):
    if state("topn", role, name) == REFUSED:
        return refused_sort(lambda types, sc, so: TopNOperator(types, 10, sc, so), role, name)
    runs = [("pages", n, o) for n in (1, 10, 2500) for o in range(4)] + [("sampled", 10, o) for o in range(4)]
    if role == "sort_key_first":
        runs += [("ties", 10, o) for o in range(4)]
    expected = {}
    for shape, n, o in runs:
        names, pages, rows, sort_channels = topn_input(role, name, shape)
        orders = [ORDERS[o], ORDERS[(o + 1) % 4]][:len(sort_channels)]
        if (shape, o) not in expected:
            expected[(shape, o)] = bits(sorted_rows(rows, names, sort_channels, orders))
        op = TopNOperator(types_of(names), n, sort_channels, orders)
        got = rows_of(to_pages(op, pages))
        op.close()
        assert bits(got) == expected[(shape, o)][:n], (shape, n, o)


# ---- join ---------------------------------------------------------------------------------------------------------------------------------
def join_case(role, name):
    """build 3000 rows, probe 5000: about 5 build rows per key for half the build rows, the rest unique; 5 % NULL keys on both sides; one
    probe key in ten absent from the build side.  BOOLEAN has two key values -- every probe row would match half the build side --: 60
    build rows and 100 probe rows for it."""
    key_name = name if role == "join_key" else "BIGINT"
    nb, npr = (60, 100) if key_name == "BOOLEAN" else (3000, 5000)
    pool = distinct_pool(key_name, nb // 10 + nb // 2 + nb // 10, 11)
    shared, unique, absent = pool[:nb // 10], pool[nb // 10:nb // 10 + nb // 2], pool[nb // 10 + nb // 2:]
    rng = np.random.default_rng(12)
    build_keys = (shared * 5 + unique)[:nb] if key_name != "BOOLEAN" else [pool[i % 2] for i in range(nb)]
    build_keys = [build_keys[i] for i in rng.permutation(len(build_keys)).tolist()]
    build_keys = [None if z else k for k, z in zip(build_keys, (rng.random(len(build_keys)) < 0.05).tolist())]
    if key_name in ("DOUBLE", "REAL"):
        build_keys[3] = float("nan")
    probe_keys = draw(key_name, npr, 13, 0.05, pool=pool)   # (one pool value in seven is on no build row)
    b_names = [key_name, name if role == "build_payload" else "BIGINT", "BIGINT"]
    p_names = [key_name, name if role == "probe_payload" else "BIGINT", "BIGINT"]
    nb, npr = len(build_keys), len(probe_keys)
    build = [build_keys, draw(b_names[1], nb, 14, 0.1), list(range(nb))]
    probe = [probe_keys, draw(p_names[1], npr, 15, 0.1), list(range(npr))]
    return b_names, pages_of(b_names, build, [nb // 2, nb - nb // 2]), p_names, pages_of(p_names, probe, [npr // 3, npr - npr // 3])


def unique_join_case(role, name):
    """build 600 rows with pairwise different keys (and 5 % NULL keys), probe 1000 rows, one key in six absent from the build side: over
    a BIGINT / INTEGER / DATE key the lookup source then has one integer key without duplicates, which is what sends the fused join
    through its one-pass form (filter, probe and output in the FilterAndProject kernels) and not through the operator chain."""
    key_name = name if role == "join_key" else "BIGINT"
    nb, npr = (2, 100) if key_name == "BOOLEAN" else (600, 1000)
    pool = distinct_pool(key_name, nb + nb // 5, 17)
    rng = np.random.default_rng(18)
    build_keys = [pool[i] for i in rng.permutation(min(nb, len(pool))).tolist()]
    nb = len(build_keys)
    if nb > 2:
        build_keys = [None if z else k for k, z in zip(build_keys, (rng.random(nb) < 0.05).tolist())]
    b_names = [key_name, name if role == "build_payload" else "BIGINT", "BIGINT"]
    p_names = [key_name, name if role == "probe_payload" else "BIGINT", "BIGINT"]
    build = [build_keys, draw(b_names[1], nb, 19, 0.1), list(range(nb))]
    probe = [draw(key_name, npr, 20, 0.05, pool=pool), draw(p_names[1], npr, 24, 0.1), list(range(npr))]
    return b_names, pages_of(b_names, build, [nb // 2, nb - nb // 2]), p_names, pages_of(p_names, probe, [npr // 3, npr - npr // 3])


def joined_rows(build_rows, probe_rows, outer):
    positions = {}
    for i, r in enumerate(build_rows):
        k = equality_key(r[0])
        if k is not None:
            positions.setdefault(k, []).append(i)
    out = []
    for r in probe_rows:
        k = equality_key(r[0])
        matches = positions.get(k, []) if k is not None else []
        for i in reversed(matches):
            out.append(r + build_rows[i][1:])
        if outer and not matches:
            out.append(r + (None, None))
    return out


@on_gpu
@pytest.mark.parametrize("role", ["join_key", "build_payload", "probe_payload"])
@per_type
def test_join(gpu, role, name):
    """HashBuilder + LookupJoin, INNER and PROBE_OUTER, and the INNER join through the fused FilterAndProject -> LookupJoin handle: over
    the build side with duplicate keys (the operator chain) and over one with unique keys (the one-pass form where the key is an integer;
    a build column that form does not carry -- VARCHAR, DECIMAL, LONG_DECIMAL -- sends it back to the chain).
    Output: the probe channels, then the build payload and build arrival index."""
    t = TYPE_OF[name]
    if state("join", role, name) == REFUSED:
        if role == "join_key":      # refused by the build side: no lookup source, nothing for a probe to be created over
            return refused(lambda: HashBuilderOperator(LookupSourceFactory(), [t, abi.BIGINT], [0], [1]))
        if role == "build_payload":
            return refused(lambda: HashBuilderOperator(LookupSourceFactory(), [abi.BIGINT, t], [0], [1]))
        bridge = LookupSourceFactory()
        builder = HashBuilderOperator(bridge, [abi.BIGINT, abi.BIGINT], [0], [1])
        for join_type in (abi.JOIN_INNER, abi.JOIN_PROBE_OUTER):
            refused(lambda: LookupJoinOperator(bridge, [abi.BIGINT, t], [0], [0, 1], join_type=join_type))
        refused(lambda: FusedJoinOperator(bridge, [abi.BIGINT, t], None, [field(0, abi.BIGINT), field(1, t)], [0], [0, 1]))
        builder.close()
        return
    b_names, build, p_names, probe = join_case(role, name)
    build_rows, probe_rows = rows_of(build), rows_of(probe)
    bridge = LookupSourceFactory()
    Driver(build, [HashBuilderOperator(bridge, types_of(b_names), [0], [1, 2])]).run()
    inner = bits(joined_rows(build_rows, probe_rows, False))
    assert len(inner) > len(probe_rows) // 2 and any(r[3] is None for r in inner) and any(r[1] is None for r in inner)
    for join_type, expected in ((abi.JOIN_INNER, inner), (abi.JOIN_PROBE_OUTER, bits(joined_rows(build_rows, probe_rows, True)))):
        op = LookupJoinOperator(bridge, types_of(p_names), [0], [0, 1, 2], join_type=join_type)
        got = rows_of(to_pages(op, probe))
        op.close()
        assert bits(got) == expected, join_type
    op = FusedJoinOperator(bridge, types_of(p_names), None, [field(c, TYPE_OF[nm]) for c, nm in enumerate(p_names)], [0], [0, 1, 2])
    got = rows_of(to_pages(op, probe))
    op.close()
    assert bits(got) == inner
    # the fused join's other execution: no duplicate build keys (positionLinks stays empty)
    b_names, build, p_names, probe = unique_join_case(role, name)
    build_rows, probe_rows = rows_of(build), rows_of(probe)
    bridge = LookupSourceFactory()
    Driver(build, [HashBuilderOperator(bridge, types_of(b_names), [0], [1, 2])]).run()
    assert (bridge.tables()[1] == -1).all()
    inner = bits(joined_rows(build_rows, probe_rows, False))
    assert len(inner) > len(probe_rows) // 2 and any(r[1] is None for r in inner)
    assert len(build_rows) == 2 or any(r[3] is None for r in inner)   # (BOOLEAN key: two build rows)
    op = FusedJoinOperator(bridge, types_of(p_names), None, [field(c, TYPE_OF[nm]) for c, nm in enumerate(p_names)], [0], [0, 1, 2])
    got = rows_of(to_pages(op, probe))
    op.close()
    assert bits(got) == inner


# ---- dynamic filter -----------------------------------------------------------------------------------------------------------------------
def domain_values(name, column):
    vals = {}
    for v in column:
        k = equality_key(v)
        if k is not None:
            vals.setdefault(k, 0.0 if isinstance(v, float) and v == 0.0 else v)   # the zero that is kept is +0.0
    return sorted(vals.values(), key=lambda v: image(name, v))


@on_gpu
@pytest.mark.parametrize("role", ["filter", "pass"])
@per_type
def test_dynamic_filter(gpu, role, name):
    """2000 rows in two pages, 40 distinct values (negatives and the edge values among them) and NULLs; max_distinct_values above 40:
    the values, typed as the channel; below 40 with min_max_collection_limit on: [min, max] (floating-point channels: no filter)."""
    t = TYPE_OF[name]
    if state("dynamic_filter", role, name) == REFUSED:
        if role == "filter":
            return refused(lambda: DynamicFilterSourceOperator([t, abi.BIGINT], [0], 100, 1 << 20, 1 << 20))
        return refused(lambda: DynamicFilterSourceOperator([abi.BIGINT, t], [0], 100, 1 << 20, 1 << 20))
    n = 2000
    key_name = name if role == "filter" else "BIGINT"
    names = [key_name, name if role == "pass" else "BIGINT"]
    columns = [draw(key_name, n, 21, 0.05, pool=distinct_pool(key_name, 40, 22)), draw(names[1], n, 23, 0.1)]
    pages = pages_of(names, columns, [n // 2, n - n // 2])
    rows = rows_of(pages)
    values = domain_values(key_name, [r[0] for r in rows])
    assert len(values) == (2 if key_name == "BOOLEAN" else 40) and any(r[0] is None for r in rows)
    for limit in (100, 10):
        op = DynamicFilterSourceOperator(types_of(names), [0], limit, 1 << 20, 1 << 20)
        passed = []
        for p in pages:
            assert op.needsInput()
            op.addInput(p)
            passed.append(Operator.getOutput(op))   # the pa_page the operator hands on (decoded: not the Python page given to addInput)
        op.finish()
        assert op.isFinished()
        assert bits(rows_of(passed)) == bits(rows)
        assert [b.type for b in passed[0].blocks] == [int(x) for x in types_of(names)]
        pred = op.predicate()
        domain_types = op.domain_types
        op.close()
        if limit >= len(values) + 1:
            assert pred[0][0] == "values" and bits([tuple(pred[0][1])]) == bits([tuple(values)]), (limit, pred)
        elif key_name in ("DOUBLE", "REAL"):
            assert pred == "all", (limit, pred)
            continue
        else:
            assert pred == [("range", values[0], values[-1])], (limit, pred)
        assert domain_types == [int(TYPE_OF[key_name])], (limit, domain_types)   # (a DECIMAL domain is not a BIGINT one)


# ---- row hash -----------------------------------------------------------------------------------------------------------------------------
def device_hash(page, channels):
    dev = upload_page(page)
    cpage, keep = dev.to_c()
    n = page.position_count
    buf = DeviceAllocation(8 * max(n, 1))
    check(lib().pa_hash_page(C.byref(cpage), len(channels), abi.int32_array(channels), buf.ptr, None))
    check(lib().pa_stream_synchronize(None))
    return download(DeviceBuffer(buf.ptr, 8 * n), np.int64, n).tolist()


@on_gpu
@per_type
def test_hash_page(gpu, oracle, name):
    """1000 rows with NULLs against oracle.hash_page (which restates the reference's hash operator of every type), alone and combined
    with a BIGINT channel.  LONG_DECIMAL heads its column with 0, 1, -1, 2^64, whose hashes are worked out by hand in
    tests/test_oracle_hash.py (XxHash64.hash(low) ^ XxHash64.hash(high)); DECIMAL hashes to its unscaled value itself."""
    if state("hash_page", "hashed", name) == REFUSED:
        return refused(lambda: device_hash(row_page(), [1]))
    n = 1000
    head = {"LONG_DECIMAL": [0, 1, -1, 1 << 64], "DECIMAL": [0, -1, 10 ** 18 - 1, -(10 ** 18 - 1)]}.get(name, [])
    column = head + draw(name, n - len(head), 31, 0.1)
    page = Page([block_of(name, column), block_of("BIGINT", draw("BIGINT", n, 32, 0.1))], n)
    got = device_hash(page, [0])
    assert got == oracle.hash_page(page, [0]).tolist()
    if name == "LONG_DECIMAL":
        assert [h & M64 for h in got[:4]] == [0, 0xABE0A1DA687F822E, 0xA06B95BB52B1DD75, 0xABE0A1DA687F822E]
    if name == "DECIMAL":
        assert got[:4] == head
    assert any(h == 0 for h, v in zip(got, column) if v is None)
    assert device_hash(page, [0, 1]) == oracle.hash_page(page, [0, 1]).tolist()
    assert device_hash(page, [1, 0]) == oracle.hash_page(page, [1, 0]).tolist()


# ---- exchange (one rank) and the wire format ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def comm(gpu):
    from presto_amd.exchange import Comm
    c = Comm.single()
    yield c
    c.destroy()


@on_gpu
@pytest.mark.parametrize("role", ["partition", "carried"])
@per_type
def test_exchange(gpu, comm, role, name):
    """World of one rank: every row comes back, in page order.  1000 rows with NULLs in two pages."""
    from presto_amd.exchange import Exchange, ExchangeOperator
    t = TYPE_OF[name]
    types, channels = ([t, abi.BIGINT], [0]) if role == "partition" else ([abi.BIGINT, t], [0])
    if state("exchange", role, name) == REFUSED:
        return refused(lambda: Exchange(comm, types, channels))
    n = 1000
    names = [name, "BIGINT"] if role == "partition" else ["BIGINT", name]
    pages = pages_of(names, [draw(names[0], n, 41, 0.1), draw(names[1], n, 42, 0.1)], [n // 2, n - n // 2])
    ex = ExchangeOperator(comm, types, channels, output_mem=abi.MEM_HOST)
    for p in pages:
        ex.addInput(p)
    ex.finish()
    out = ex.getOutput()
    assert ex.isFinished()
    got = rows_of([out])
    ex.close()
    assert bits(got) == bits(rows_of(pages))


@on_gpu
@per_type
def test_serde(gpu, name):
    """pa_page_serialize -> pa_page_deserialize_typed of a host and of a device page: 1000 rows with NULLs."""
    if state("serde", "channel", name) == REFUSED:
        page = row_page() if name == "ROW" else Page([block_of("BIGINT", [1, 2, 3]), block_of(name, EDGES[name][:3])], 3)
        refused(lambda: serialize_page(page))
        return refused(lambda: serialize_page(upload_page(page)))
    n = 1000
    page = Page([block_of(name, draw(name, n, 51, 0.1)), block_of("BIGINT", draw("BIGINT", n, 52, 0.1))], n)
    types = [TYPE_OF[name], abi.BIGINT]
    for source in (page, upload_page(page)):
        back = deserialize_page(serialize_page(source), types=[int(t) for t in types])
        assert [b.type for b in back.blocks] == [int(t) for t in types]
        assert bits(rows_of([back])) == bits(page.to_rows())
