"""tests/key_model.py pinned by the facts of the reference it restates (no GPU): which values are one group, what the group's key
is emitted as, and that every shape of tests/test_gpu_group_key_edges.py has edge keys that tell groups apart."""
import os
import re
import struct

import numpy as np

from presto_amd import abi
from tests import key_model as K
from tests.key_model import F32, F64, emitted, identity


def test_null_is_one_group_of_its_own():
    for label in K.KEY_EDGES:
        assert identity(label, None) == identity(label, None)
        for v in K.KEY_EDGES[label]:
            assert identity(label, v) != identity(label, None), (label, v)
        assert emitted(label, None) is None


def test_every_nan_is_one_group_and_the_zeros_are_one_group():
    """DoubleType.java:181-192 / RealType.java:127-140: distinctFrom is false for two NaNs (isNaN on both sides) and goes by == otherwise"""
    nans64 = [F64(b) for b in (0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFFFFFFFFFFFFFFF, 0x7FF8000000000001)]
    assert len({identity("DOUBLE", v) for v in nans64}) == 1
    assert {emitted("DOUBLE", v) for v in nans64} == {0x7FF8000000000000}
    nans32 = [F32(b) for b in (0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF, 0x7FC00001)]
    assert len({identity("REAL", v) for v in nans32}) == 1
    assert {emitted("REAL", v) for v in nans32} == {0x7FC00000}
    assert identity("DOUBLE", F64(1 << 63)) == identity("DOUBLE", F64(0)) and emitted("DOUBLE", F64(1 << 63)) == 0
    assert identity("REAL", F32(1 << 31)) == identity("REAL", F32(0)) and emitted("REAL", F32(1 << 31)) == 0
    # the infinities are values, not NaNs; the smallest denormals are not zeros
    for label, T, inf, tiny in (("DOUBLE", F64, 0x7FF0000000000000, 1), ("REAL", F32, 0x7F800000, 1)):
        assert identity(label, T(inf)) not in (identity(label, T(K.NAN64 if T is F64 else K.NAN32)), identity(label, T(0)))
        assert identity(label, T(tiny)) != identity(label, T(0)) and emitted(label, T(tiny)) == tiny
    # the model agrees with Python's own floats on every DOUBLE edge: equal exactly when == or both NaN
    vals = K.KEY_EDGES["DOUBLE"]
    fl = [struct.unpack("<d", struct.pack("<Q", v.bits))[0] for v in vals]
    for a, x in zip(vals, fl):
        for b, y in zip(vals, fl):
            assert (identity("DOUBLE", a) == identity("DOUBLE", b)) == (x == y or (x != x and y != y)), (a, b)
    vals = K.KEY_EDGES["REAL"]
    fl = np.asarray([v.bits for v in vals], dtype=np.uint32).view(np.float32)
    for a, x in zip(vals, fl):
        for b, y in zip(vals, fl):
            assert (identity("REAL", a) == identity("REAL", b)) == bool(x == y or (np.isnan(x) and np.isnan(y))), (a, b)


def test_other_values_are_emitted_as_they_are():
    for label, vals in K.KEY_EDGES.items():
        for v in vals:
            if K.diverges(label, v) or K.base(label) == "BOOLEAN":
                continue
            assert emitted(label, v) == (v.bits if isinstance(v, (F64, F32)) else v), (label, v)


def test_varchar_compares_by_bytes_whatever_the_bound():
    for label in ("VARCHAR0", "VARCHAR1", "VARCHAR3", "VARCHAR7", "VARCHAR15"):
        assert identity(label, b"") != identity(label, b"\x00") != identity(label, b"\x00\x00")
        assert identity(label, b"a") != identity(label, b"a\x00") and identity(label, b"a") != identity(label, b"a ")
        assert identity(label, b"a") == identity(label, bytes(bytearray(b"a")))
    assert identity("VARCHAR3", b"ab") == identity("VARCHAR15", b"ab") == identity("VARCHAR0", b"ab")


def test_boolean_compares_by_truth_value():
    assert len({identity("BOOLEAN", v) for v in (True, 1, 2, 0x80, 0xFF)}) == 1
    assert identity("BOOLEAN", False) == identity("BOOLEAN", 0) != identity("BOOLEAN", True)
    assert emitted("BOOLEAN", 0xA5) is True and emitted("BOOLEAN", 0) is False


def test_integers_and_decimals_compare_by_value():
    for label in ("BIGINT", "INTEGER", "DATE", "DECIMAL"):
        vals = K.KEY_EDGES[label]
        assert len({identity(label, v) for v in vals}) == len(set(vals)) == len(vals), label
    assert identity("DECIMAL", 100) != identity("DECIMAL", 1)         # 1.00 and 0.01: the unscaled value, one scale per channel


def test_the_edges_the_key_path_is_written_around():
    assert K.s64(K.KEY_CLEAR) == -6510615555426900571 and K.s64(K.KEY_CLEAR) in K.KEY_EDGES["BIGINT"]
    assert F64(K.KEY_CLEAR) in K.KEY_EDGES["DOUBLE"]
    assert not -(10 ** 18) < K.s64(K.KEY_CLEAR) < 10 ** 18            # out of DECIMAL(18, 2)'s range: not among its edges
    assert all(abs(v) < 10 ** 18 for v in K.KEY_EDGES["DECIMAL"])
    assert K.s32(K.CLEAR32) == -1515870811
    for label in ("INTEGER", "DATE"):
        assert K.s32(K.CLEAR32) in K.KEY_EDGES[label] and {-1, 0, -2 ** 31, 2 ** 31 - 1} <= set(K.KEY_EDGES[label])
    assert F32(K.CLEAR32) in K.KEY_EDGES["REAL"]
    assert {-1, 0, -2 ** 63, 2 ** 63 - 1, -2 ** 31} <= set(K.KEY_EDGES["BIGINT"])
    # (INTEGER, INTEGER) without null arrays packs the clear pattern into its one word
    both = (K.s32(K.CLEAR32), K.s32(K.CLEAR32))
    assert both in K.edge_keys(K.SHAPES["integer_integer_nn"])
    assert ((both[0] & 0xFFFFFFFF) | ((both[1] & 0xFFFFFFFF) << 32)) == K.KEY_CLEAR
    for label, T, quiet_bit in (("DOUBLE", F64, 1 << 51), ("REAL", F32, 1 << 22)):
        nans = [v for v in K.KEY_EDGES[label] if K.is_nan(v)]
        top = 63 if T is F64 else 31
        assert any(v.bits >> top for v in nans) and any(not v.bits & quiet_bit for v in nans)          # a sign bit; a signalling NaN
        assert any(v.bits & (quiet_bit - 1) for v in nans)                                               # payload bits
    b = [v & K.M64 for v in K.KEY_EDGES["BIGINT"]] + [v.bits for v in K.KEY_EDGES["DOUBLE"]]
    for part in (lambda v: v & 0xFFFFFFFF, lambda v: v >> 32):
        assert any(part(v) == 0xFFFFFFFF and v != K.M64 for v in b) and any(part(v) == 0 and v != 0 for v in b)
    for n in (1, 3, 7, 15):
        edges = K.KEY_EDGES["VARCHAR%d" % n]
        assert all(len(s) <= n for s in edges) and any(len(s) == n for s in edges) and b"\xff" * n in edges
        assert {b"", b"\x00", b"a"} <= set(edges) and (n == 1 or b"a\x00" in edges)
    v15 = K.KEY_EDGES["VARCHAR15"]
    assert any(len(s) == 8 for s in v15) and any(len(s) == 7 for s in v15)
    assert sum(1 for s in v15 if s[:8] == b"abcdefgh") >= 4 and sum(1 for s in v15 if s[:13] == K.P15[:13]) >= 4
    v0 = K.KEY_EDGES["VARCHAR0"]
    for stem in (K.P15, K.P39):
        assert {stem, stem + b"1", stem + b"2", stem + b"\x00"} <= set(v0)
    assert {len(K.P15 + b"1"), len(K.P39 + b"1")} == {16, 40}


def test_every_shape_has_edge_keys_that_differ():
    assert [s.name for s in K.SINGLE] == ["bigint", "bigint_nn", "integer_nn", "integer", "date", "double", "real", "boolean", "decimal", "varchar1",
                                          "varchar7", "varchar15", "varchar0"]
    for name, shape in K.SHAPES.items():
        groups = {K.key_identity(shape, k) for k in K.edge_keys(shape)}
        if name == "boolean":
            assert len(groups) == 3        # true, false, NULL
        else:
            assert len(groups) >= 2, name
        assert len(K.distinct_edge_keys(shape)) == len(groups)
    # the pairs that differ only in where a value sits are different groups
    s = K.SHAPES["integer_date_boolean"]
    assert K.key_identity(s, (None, 0, False)) != K.key_identity(s, (0, None, False)) != K.key_identity(s, (0, 0, None))
    assert K.key_identity(s, (-1, 0, False)) != K.key_identity(s, (0, -1, False))
    for t in ((None, 0, False), (0, None, False), (-1, 0, False), (0, -1, False), (-2 ** 31, 2 ** 31 - 1, False), (2 ** 31 - 1, -2 ** 31, False)):
        assert t in K.edge_keys(s), t
    # the packed forms as the planner's sizes give them: a nullable INTEGER is 33 bits, (BOOLEAN, VARCHAR(3)) with flags 31
    assert 1 + 1 + (8 * 3 + 4) + 1 == 31


def test_blocks_hold_the_patterns():
    vals = K.KEY_EDGES["REAL"] + [None]
    b = K.key_block("REAL", vals, True)
    assert b.type == abi.REAL and b.values.view(np.uint32).tolist() == [0 if v is None else v.bits for v in vals]
    assert K.column_patterns(b, "REAL") == [None if v is None else v.bits for v in vals]
    vals = K.KEY_EDGES["DOUBLE"]
    b = K.key_block("DOUBLE", vals, False)
    assert b.nulls is None and K.column_patterns(b, "DOUBLE") == [v.bits for v in vals]
    b = K.key_block("BOOLEAN", [True, 0xA5, False, None], True)
    assert b.values.tolist() == [1, 0xA5, 0, 0] and b.nulls.tolist() == [0, 0, 0, 1]
    b = K.key_block("VARCHAR7", [b"a\x00", b"", None], True)
    assert K.column_patterns(b, "VARCHAR7") == [b"a\x00", b"", None]
    assert K.key_block("BIGINT", [1, 2], True).nulls.tolist() == [0, 0] and K.key_block("BIGINT", [1, 2], False).nulls is None
    for label in K.KEY_EDGES:
        f = K.fillers(label, 60, 3)
        ids = {K.identity(label, v) for v in f}
        assert len(ids) == len(f) and not ids & {K.identity(label, v) for v in K.KEY_EDGES[label]}, label
        assert len(f) == (0 if label == "BOOLEAN" else 60), (label, len(f))


def test_hash_of_is_the_hash_of_the_canonical_key(oracle):
    """$hashvalue follows the emitted key: one hash for both zeros and for every NaN, 0 for NULL"""
    for label, T in (("DOUBLE", F64), ("REAL", F32)):
        shape = K.Shape("one", [K.Part(label, True)])
        keys = [(v,) for v in K.KEY_EDGES[label]] + [(None,)]
        hashes = K.hash_of(oracle, shape, keys)
        by_group = {}
        for k, h in zip(keys, hashes):
            by_group.setdefault(K.key_identity(shape, k), set()).add(h)
        assert all(len(h) == 1 for h in by_group.values())
        assert by_group[("null",),] == {0}


def test_design_names_the_key_divergences():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "DESIGN.md")).read()
    section = text[text.index("## 5. Parity"):text.index("## 6. Measurement")]
    assert set(re.findall(r"`(key-[a-z-]+)`", section)) == set(K.DIVERGENCES)
    for tag, names in K.DIVERGENCES.items():
        assert names, tag
    assert all(n.startswith(("DOUBLE:", "REAL:")) for names in K.DIVERGENCES.values() for n in names)
