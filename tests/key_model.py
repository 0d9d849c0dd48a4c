"""Group identity and the emitted group key, stated from the reference -- not from the kernels (tests/test_key_model_cpu.py pins it,
tests/test_gpu_group_key_edges.py runs the fused aggregation against it).

Identity is the IS NOT DISTINCT FROM of GroupByHash (MultiChannelGroupByHash / BigintGroupByHash compare positions with the type's
`DISTINCT FROM` operator):
  NULL          one group, whatever the block holds under the flag
  BIGINT, INTEGER, DATE, short DECIMAL   the (unscaled) value
  DOUBLE, REAL  every NaN is one group -- whatever its sign and payload, quiet or signalling -- and -0.0 / +0.0 are one group
                (DoubleType.java:181-192, RealType.java:127-140: distinctFrom goes through isNaN and ==)
  BOOLEAN       the truth value (ByteArrayBlock: getByte(position) != 0)
  VARCHAR       the bytes, whatever the declared bound: no padding, a trailing 0x00 is a byte like any other

Emitted value: the reference emits the pattern of the group's first row.  The device keeps canonical key bits and emits those: +0.0 for
both zeros, 0x7ff8000000000000 (REAL: 0x7fc00000) for every NaN, 1 for every true byte.  `emitted` returns that canonical form and
DIVERGENCES tags the edge values for which it is not the pattern that went in (divergence (2)).

Values: int for the integer types and DECIMAL (unscaled), bool or a raw byte (int) for BOOLEAN, bytes for VARCHAR, F64(bits) / F32(bits)
for the floating-point types -- bit patterns, so that a NaN's payload survives every step on the host --, None for NULL.

$hashvalue is expected from oracle.hash_page over the page of emitted keys (hash_of below), which tests/test_gpu_type_matrix.py's
test_hash_page pins for every type.
"""
import collections
import struct

import numpy as np

from presto_amd.page import Page
from tests.test_gpu_type_matrix import EDGES, TYPE_OF, bits, block_of, distinct_pool  # noqa: F401  (bits: rows by bit pattern)

F64 = collections.namedtuple("F64", "bits")
F32 = collections.namedtuple("F32", "bits")

M64 = (1 << 64) - 1
KEY_CLEAR = 0xA5A5A5A5A5A5A5A5            # the pattern new key arrays of the HBM table are filled with (PA_GT_KEY_CLEAR)
CLEAR32 = 0xA5A5A5A5
NAN64, NAN32 = 0x7ff8000000000000, 0x7fc00000


def s64(u):
    return u - (1 << 64) if u >> 63 else u


def s32(u):
    return u - (1 << 32) if u >> 31 else u


def f64(v):
    return F64(struct.unpack("<Q", struct.pack("<d", v))[0])


def f32(v):
    return F32(int(np.asarray([v], dtype=np.float32).view(np.uint32)[0]))


# ---- labels: a type as a key part declares it ------------------------------------------------------------------------------------------------
# VARCHAR<n>: VARCHAR(n); VARCHAR0: no declared bound (the type parameter 0)
def base(label):
    return "VARCHAR" if label.startswith("VARCHAR") else label


def bound(label):
    return int(label[len("VARCHAR"):]) if label.startswith("VARCHAR") else 0


def type_of(label):
    return TYPE_OF[base(label)]


def type_param(label):
    from presto_amd import abi
    return bound(label) if base(label) == "VARCHAR" else abi.type_param(type_of(label))


def is_nan(v):
    if isinstance(v, F64):
        return (v.bits >> 52) & 0x7ff == 0x7ff and v.bits & ((1 << 52) - 1) != 0
    return (v.bits >> 23) & 0xff == 0xff and v.bits & ((1 << 23) - 1) != 0


def is_zero(v):
    return v.bits & ((1 << (63 if isinstance(v, F64) else 31)) - 1) == 0


def identity(label, v):
    """hashable; equal for two values exactly when GroupByHash puts them into one group"""
    if v is None:
        return ("null",)
    name = base(label)
    if name in ("DOUBLE", "REAL"):
        assert isinstance(v, F64 if name == "DOUBLE" else F32), (label, v)
        return ("nan",) if is_nan(v) else (("zero",) if is_zero(v) else ("bits", v.bits))
    if name == "BOOLEAN":
        return ("bool", v not in (False, 0))
    if name == "VARCHAR":
        assert isinstance(v, bytes)
        return ("bytes", v)
    assert isinstance(v, int) and not isinstance(v, bool), (label, v)
    return ("int", v)


def emitted(label, v):
    """what the output block holds for the group of v: None, an int, a bool, bytes, or the bit pattern (int) of a DOUBLE / REAL"""
    if v is None:
        return None
    name = base(label)
    if name in ("DOUBLE", "REAL"):
        return (NAN64 if name == "DOUBLE" else NAN32) if is_nan(v) else (0 if is_zero(v) else v.bits)
    if name == "BOOLEAN":
        return v not in (False, 0)
    return v


def diverges(label, v):
    """-> the DIVERGENCES tag of a value whose emitted form is not its own pattern (the reference would emit the pattern when the value
    is the group's first row), or None"""
    if v is None or base(label) not in ("DOUBLE", "REAL"):
        return None
    if is_nan(v) and v.bits != (NAN64 if base(label) == "DOUBLE" else NAN32):
        return "key-nan-payload"
    if is_zero(v) and v.bits != 0:
        return "key-negative-zero"
    return None


# ---- edge values ---------------------------------------------------------------------------------------------------------------------------------
def _fp(name, values):
    return [(f64 if name == "DOUBLE" else f32)(v) for v in values]


P15, P39 = b"0123456789abcde", b"the quick brown fox jumps over the lazy"
assert len(P15) == 15 and len(P39) == 39
_STRINGS = EDGES["VARCHAR"] + [
    b"", b"\x00", b"a", b"a\x00", b"\x00a", b"\x00\x00", b" ", b"a ",
    b"x", b"xyz", b"xy\x00", b"abcdefg", b"abcdef\x00", b"12345678", b"1234567\x00", P15, P15[:14] + b"\x00",   # at the bounds 1, 3, 7, 8, 15
    b"abcdefgh1", b"abcdefgh2", b"abcdefgh\x00\x00",                                                             # equal in the first 8 bytes
    P15[:14], P15[:14] + b"f", P15[:13], P15[:13] + b"\x00",                                                      # equal in the first 13 / 14 of 15
]
_LONG = [P15 + b"1", P15 + b"2", P15 + b"\x00", P39 + b"1", P39 + b"2", P39 + b"\x00", P39]     # 16 and 40 bytes: the last byte, a trailing 0x00


def _varchar_edges(n):
    out = []
    for s in _STRINGS + ([b"\xff" * k for k in (1, 2, 3, 7, 8, 15) if k <= n] if n else [b"\xff" * 15, b"\xff" * 16]) + ([] if n else _LONG):
        if (n == 0 or len(s) <= n) and s not in out:
            out.append(s)
    return out


KEY_EDGES = {
    "BIGINT": EDGES["BIGINT"] + [s64(KEY_CLEAR), CLEAR32, s64(CLEAR32 << 32), -2 ** 31, 2 ** 31 - 1, 2 ** 31, (1 << 32) - 1, s64(0x7FFFFFFF00000000),
                                 s64(0x8000000000000001), s64(0xFFFFFFFF7FFFFFFF), s64(0x00000001FFFFFFFF), s64(0xA5A5A5A5A5A5A5A4), s64(0xA5A5A5A5A5A5A5A6)],
    # DECIMAL(18, 2) ends at +-(10^18 - 1): the clear pattern (-6510615555426900571) is out of its range
    "DECIMAL": EDGES["DECIMAL"] + [(1 << 32) - 1, 1 << 32, -(1 << 32), -2 ** 31, 2 ** 31 - 1, CLEAR32, -(CLEAR32 << 28)],
    "INTEGER": EDGES["INTEGER"] + [s32(CLEAR32), s32(CLEAR32) + 1, 0xFFFF, -(1 << 16), s32(0x80000001)],
    "DATE": EDGES["DATE"] + [s32(CLEAR32), 0xFFFF, -(1 << 16)],
    "DOUBLE": _fp("DOUBLE", EDGES["DOUBLE"]) + [F64(b) for b in (
        KEY_CLEAR, 0xFFF8000000000001, 0x7FF8000000000000, 0x7FF0000000000001, 0xFFF4000000000000, 0x7FFFFFFFFFFFFFFF, M64, 0xFFFFFFFF00000000,
        0x7FF00000FFFFFFFF, 0x00000000FFFFFFFF, 0x80000000FFFFFFFF, 0x3FF00000FFFFFFFF, 0xFFEFFFFF00000000, 0x0000000100000000, 0x8000000000000001)],
    "REAL": _fp("REAL", EDGES["REAL"]) + [F32(b) for b in (CLEAR32, 0xFFC00001, 0x7FC00000, 0x7F800001, 0xFFA00000, 0x7FFFFFFF, 0xFFFFFFFF, 0x0000FFFF, 0xFFFF0000 & 0xFF7FFFFF,
                                                           0x80000001)],
    "BOOLEAN": [True, False, 2, 0x80, 0xA5, 0xFF],      # (a true byte is any byte but 0)
}
for _n in (0, 1, 2, 3, 7, 15):
    KEY_EDGES["VARCHAR%d" % _n] = _varchar_edges(_n)

# the -1 / 0 / MIN / MAX of a type, for the rows of a multi-key shape that differ only in where they sit
SPECIAL = {
    "BIGINT": dict(zero=0, ones=-1, min=-2 ** 63, max=2 ** 63 - 1), "DECIMAL": dict(zero=0, ones=-1, min=-(10 ** 18 - 1), max=10 ** 18 - 1),
    "INTEGER": dict(zero=0, ones=-1, min=-2 ** 31, max=2 ** 31 - 1), "DATE": dict(zero=0, ones=-1, min=-2 ** 31, max=2 ** 31 - 1),
    "DOUBLE": dict(zero=F64(0), ones=F64(0xBFF0000000000000), min=F64(0xFFF0000000000000), max=F64(0x7FF0000000000000)),
    "REAL": dict(zero=F32(0), ones=F32(0xBF800000), min=F32(0xFF800000), max=F32(0x7F800000)),
    "BOOLEAN": dict(zero=False, ones=True, min=False, max=True),
}


def special(label):
    if base(label) == "VARCHAR":
        n = bound(label) or 16
        return dict(zero=b"", ones=b"\xff" * n, min=b"\x00", max=b"\xff")
    return SPECIAL[label]


def edge_name(label, v):
    return "%s:%s" % (label, "%x" % v.bits if isinstance(v, (F64, F32)) else repr(v))


DIVERGENCES = {tag: [edge_name(label, v) for label in sorted(KEY_EDGES) for v in KEY_EDGES[label] if diverges(label, v) == tag]
               for tag in ("key-negative-zero", "key-nan-payload")}


# ---- shapes ----------------------------------------------------------------------------------------------------------------------------------------
Part = collections.namedtuple("Part", "label nullable")        # nullable: the channel comes with a valueIsNull array (and NULL keys)
Shape = collections.namedtuple("Shape", "name parts")


def _shape(name, *parts):
    return Shape(name, [Part(*p) for p in parts])


SINGLE = [
    _shape("bigint", ("BIGINT", True)), _shape("bigint_nn", ("BIGINT", False)),
    _shape("integer_nn", ("INTEGER", False)),          # 32 bits: one bit too many for the packed form
    _shape("integer", ("INTEGER", True)),              # 33 bits
    _shape("date", ("DATE", True)), _shape("double", ("DOUBLE", True)), _shape("real", ("REAL", True)), _shape("boolean", ("BOOLEAN", True)),
    _shape("decimal", ("DECIMAL", True)),
    _shape("varchar1", ("VARCHAR1", True)), _shape("varchar7", ("VARCHAR7", True)), _shape("varchar15", ("VARCHAR15", True)),
    _shape("varchar0", ("VARCHAR0", True)),            # no declared bound: grouped by interned id
]
MULTI = [
    _shape("integer_integer_nn", ("INTEGER", False), ("INTEGER", False)),                    # one full word: holds the clear pattern
    _shape("integer_date_boolean", ("INTEGER", True), ("DATE", True), ("BOOLEAN", True)),      # the second part in word 1, flags first-fit into the gaps
    _shape("boolean_varchar3", ("BOOLEAN", True), ("VARCHAR3", True)),                        # 1 + 1 + 28 + 1 = 31 bits: the packed form
    _shape("varchar15_bigint_varchar2", ("VARCHAR15", False), ("BIGINT", True), ("VARCHAR2", False)),
    Shape("bigint_x8_nn", [Part("BIGINT", False)] * 8),                                      # the 8-word limit
]
SHAPES = collections.OrderedDict((s.name, s) for s in SINGLE + MULTI)


def part_values(part):
    return list(KEY_EDGES[part.label]) + ([None] if part.nullable else [])


def edge_keys(shape):
    """the key tuples of a shape's edges: every edge value (and NULL) of every part next to zeros and next to NULLs / all-ones, the same
    edge value in every part of the first part's type, and for every two parts the pairs that differ only in where the NULL, the zero,
    the -1, MIN and MAX sit"""
    parts = shape.parts
    if len(parts) == 1:
        return [(v,) for v in part_values(parts[0])]
    out = []

    def add(t):
        if t not in out:
            out.append(t)

    zero = [special(p.label)["zero"] for p in parts]
    other = [None if p.nullable else special(p.label)["ones"] for p in parts]
    for i, p in enumerate(parts):
        for v in part_values(p):
            for rest in (zero, other):
                t = list(rest)
                t[i] = v
                add(tuple(t))
    for v in part_values(parts[0]):         # the same value in every part of the first part's type: every key word the clear pattern among them
        add(tuple(v if p == parts[0] else z for p, z in zip(parts, zero)))
    for i, p in enumerate(parts):
        for j, q in enumerate(parts):
            if i == j:
                continue
            sp, sq = special(p.label), special(q.label)
            pairs = [(sp["ones"], sq["zero"]), (sp["zero"], sq["ones"]), (sp["min"], sq["max"]), (sp["max"], sq["min"])]
            if p.nullable:
                pairs += [(None, sq["zero"]), (None, sq["ones"])]
            if q.nullable:
                pairs += [(sp["zero"], None), (sp["ones"], None)]
            for a, b in pairs:
                t = list(zero)
                t[i], t[j] = a, b
                add(tuple(t))
    return out


def key_identity(shape, key):
    return tuple(identity(p.label, v) for p, v in zip(shape.parts, key))


def key_emitted(shape, key):
    return tuple(emitted(p.label, v) for p, v in zip(shape.parts, key))


def distinct_edge_keys(shape):
    """edge_keys without the tuples that are the group of an earlier one"""
    seen, out = set(), []
    for k in edge_keys(shape):
        i = key_identity(shape, k)
        if i not in seen:
            seen.add(i)
            out.append(k)
    return out


def from_python(label, v):
    """a value as tests/test_gpu_type_matrix.py draws it -> as this model holds it"""
    name = base(label)
    return f64(v) if name == "DOUBLE" else (f32(v) if name == "REAL" else v)


def fillers(label, count, seed):
    """up to `count` further values of the type, pairwise different under identity and different from every edge value"""
    name = base(label)
    taken = {identity(label, v) for v in KEY_EDGES[label]}
    out = []
    if name == "VARCHAR" and 0 < bound(label) < 15:
        n = bound(label)
        rng = np.random.default_rng(seed)
        cands = [bytes([b]) for b in range(256)] if n == 1 else []
        cands += [bytes(rng.integers(0, 256, int(rng.integers(1, n + 1)), dtype=np.uint8).tolist()) for _ in range(2 * count if n > 1 else 0)]
    elif name == "BOOLEAN":
        cands = []
    else:
        cands = [from_python(label, v) for v in distinct_pool(name, (2 if name == "VARCHAR" else 1) * count + len(EDGES[name]) + 64, seed)]
        if name == "VARCHAR":
            cands = [s for s in cands if not bound(label) or len(s) <= bound(label)]
    for v in cands:
        i = identity(label, v)
        if i not in taken and len(out) < count:
            taken.add(i)
            out.append(v)
    return out


# ---- blocks ----------------------------------------------------------------------------------------------------------------------------------------
def key_block(label, values, nullable):
    """a host block of the part's type holding exactly the given patterns (None = NULL: a zero under the flag)"""
    name = base(label)
    assert nullable or None not in values
    if name in ("DOUBLE", "REAL"):
        b = block_of(name, [None if v is None else 0.0 for v in values])
        raw = np.asarray([0 if v is None else v.bits for v in values], dtype=np.uint64 if name == "DOUBLE" else np.uint32)
        b.values = raw.view(np.float64 if name == "DOUBLE" else np.float32)
    elif name == "BOOLEAN":
        b = block_of(name, values)
        b.values = np.asarray([0 if v is None else int(v) for v in values], dtype=np.uint8)
    else:
        b = block_of(name, values)
    if nullable and b.nulls is None:
        b.nulls = np.zeros(b.position_count, dtype=np.uint8)
    return b


def column_patterns(block, label):
    """a host output block -> what `emitted` returns per position"""
    name, n = base(label), block.position_count
    if name in ("DOUBLE", "REAL"):
        out = np.ascontiguousarray(block.values[:n]).view(np.uint64 if name == "DOUBLE" else np.uint32).tolist()
        return [None if block.nulls is not None and block.nulls[i] else out[i] for i in range(n)]
    if name == "BOOLEAN":
        raw = block.values[:n].tolist()
        assert all(v in (0, 1) for v in raw), "a BOOLEAN key is emitted as 0 or 1"
    return block.to_pylist()


def emitted_page(shape, keys):
    """the page of the emitted forms of `keys` (tuples of values), every channel as the output has it"""
    cols = []
    for i, p in enumerate(shape.parts):
        name = base(p.label)
        vals = [emitted(p.label, k[i]) for k in keys]
        if name in ("DOUBLE", "REAL"):
            vals = [None if v is None else (F64 if name == "DOUBLE" else F32)(v) for v in vals]
        cols.append(key_block(p.label, vals, True))
    return Page(cols, len(keys))


def hash_of(oracle, shape, keys):
    """$hashvalue of the groups of `keys`: InterpretedHashGenerator over the emitted key columns"""
    return oracle.hash_page(emitted_page(shape, keys), list(range(len(shape.parts)))).tolist()
