"""VARCHAR(1) group keys without their offsets ("VARCHAR(1) keys without offsets"), off the GPU: the Q1 shape is generated
and compiled for gfx950 (hiprtc in process) in every tier whose vector loop reads the key channels, with no channel and with every
channel nullable; the vector loops must hold the wave-uniform guard (the page's n strings hold n bytes) and the per-quad ASCII test, and
load the offsets only behind them.  Shapes whose VARCHAR key has a bound of 2..7 bytes or none must generate what they generated
before the change: their sources are compared with hashes taken from the parent commit (scripts/dump_codegen.py writes the sources)."""
import ctypes as C
import hashlib
import re

import pytest

from presto_amd import abi
from presto_amd._lib import lib
from presto_amd.expr import constant, field
from presto_amd.operators import fused_aggregation_desc
from tests import test_codegen_tiers as T

Q1 = "two_varchar1_keys_q1"
TIERS = [T.V_LDS, T.V_GT, T.V_LDSH, T.V_LDS_R, T.V_GLOBAL_R]
ALL_NULLABLE = (1 << 7) - 1

# sha256 of the generated source on the parent commit: (bound of the VARCHAR key, tier) -> digest
PARENT_SOURCES = {
    (2, "lds"): "499c1f51b169d3a46f85d4231a9da0a2bb06ed0b64817172283003abb6deb639",
    (2, "gt"): "1cd7fa6a0d2161c04fe2e6bd64b47a3f7da771824aafa8283336488904271fa7",
    (2, "lds_ranges"): "6e30d3eb4c5ce019479bd4cb97a8310aeedfc5d6615adf51a9d558c59c988337",
    (7, "lds"): "5bf192c39fd0bd221b6ac2e35fe9f26b5dbe3d9259be10c998bae4f5e94f6a5c",
    (7, "ldsh"): "3a2c1f4095a8908becc154a551df0b745cce93dc409beada96d8f2498284cf62",
    (0, "lds"): "b31fea4ed7b76e689abb3422c075853cc3ea954f0f003fa07473dffb72aa0f5f",
    (0, "gt"): "23787594b1bffacdd7efdd6afc4132c615a52e5251f4c4d1797a599720220a16",
    (12, "ldsh"): "12d82e617a155d23c2761f5007fa9ef8b11a5a0204e3d6fe6bc340f2136875bd",
    (1, "global"): "b9d5d0f51a6c3614e2b29ef8d396ab93197591d03e8d56f047f6f8099aa8be55",
    (1, "global_ranges"): "35411a29eae3511a5d25d562680f02f10a9fcf50e43e2940b8cd3549cd2bd6a2",
}


def keyed_source(bound, variant, mask=0):
    """a VARCHAR key declared VARCHAR(bound) (0: no bound) next to a BIGINT key, a sum and a count; the `global` tiers (no group key):
    a sum over the rows whose VARCHAR(bound) channel equals a constant"""
    types = [abi.VARCHAR, abi.BIGINT, abi.DOUBLE]
    if variant in (T.V_GLOBAL, T.V_GLOBAL_R):
        d, keep = fused_aggregation_desc(types, field(0, abi.VARCHAR).eq(constant("y", abi.VARCHAR)), [field(1, abi.BIGINT)], [],
                                         [(abi.AGG_SUM, 0, abi.BIGINT)], type_params=[bound, 0, 0])
    else:
        d, keep = fused_aggregation_desc(types, None, [field(0, abi.VARCHAR), field(1, abi.BIGINT), field(2, abi.DOUBLE)], [0, 1],
                                         [(abi.AGG_SUM, 2, abi.DOUBLE), (abi.AGG_COUNT_STAR, -1, None)], type_params=[bound, 0, 0])
    L = lib()
    L.pa_codegen_fused_layout.restype = C.c_int64
    L.pa_codegen_fused_layout.argtypes = [C.c_void_p, C.c_int32, C.c_uint64, C.c_int32, C.c_char_p, C.c_int64]
    need = L.pa_codegen_fused_layout(C.byref(d), variant, mask, 0, None, 0)
    assert need > 0, (bound, T.TIER_NAMES[variant], L.pa_last_error())
    buf = C.create_string_buffer(need)
    L.pa_codegen_fused_layout(C.byref(d), variant, mask, 0, buf, need)
    return buf.value.decode()


def vector_loops(src):
    """the bodies of the loops over row quads (`for (i64 q = ...`) of the generated kernels"""
    out = []
    for m in re.finditer(r"^ *for \(i64 q = [^\n]*\{\n", src, re.M):
        depth, i = 1, m.end()
        while depth:
            depth += {"{": 1, "}": -1}.get(src[i], 0)
            i += 1
        out.append(src[m.end():i])
    return out


@pytest.mark.parametrize("mask", [0, ALL_NULLABLE])
@pytest.mark.parametrize("variant", TIERS, ids=[T.TIER_NAMES[v] for v in TIERS])
def test_q1_shape_compiles_and_guards_its_offset_loads(variant, mask):
    rc, msg = T.generate(Q1, variant, mask, True)
    if variant == T.V_GLOBAL_R:
        # the ungrouped tier has no kernel for a descriptor with group keys, and only a group key is ever a short channel: what a
        # VARCHAR(1) channel without a key generates there is pinned by test_other_bounds_generate_what_they_did
        assert rc == abi.ERR_INVALID_ARGUMENT and "variant does not match the descriptor" in msg, (rc, msg)
        return
    assert rc > 1000, (T.TIER_NAMES[variant], mask, rc, msg[-800:])
    src = T.source(Q1, variant, mask)
    n = "RN" if variant in (T.V_LDS_R, T.V_GLOBAL_R) else "a.n"
    for c in (0, 1):
        assert "const bool U%d = PB%d == (i64)%s;" % (c, c, n) in src
    loops = [b for b in vector_loops(src) if "pa_i32x4 O0" in b]
    assert loops, "no vector loop reads the key channels"
    for body in loops:
        for c in (0, 1):
            guard = "if (U%d && (K%d & 0x80808080u) == 0u) {" % (c, c)
            assert body.count(guard) == 1
            load = re.compile(r"O%d = \(\(const pa_i32x4\*\)[^;]*\)\[q\]; E%d = [^;]*\[4 \* q \+ 4\];" % (c, c))
            hits = [m.start() for m in load.finditer(body)]
            assert len(hits) == 1, "the offsets of a quad are loaded in one place"
            at = body.index(guard)
            # ... the else branch of the guard, behind every independent load of the quad (the key bytes K<c> among them)
            assert at < body.index("} else {", at) < hits[0] < body.index("pa_row(")
            assert max(m.start() for m in re.finditer(r"\(\(const pa_(?:f64x2|i32x4)\*\)(?:a\.v\[|RV)", body)) < at
    # the row-by-row paths keep reading the offsets and keep the check of the declared bound
    assert src.count("pa_short_bytes(") >= 8


@pytest.mark.parametrize("bound,tier", sorted(PARENT_SOURCES))
def test_other_bounds_generate_what_they_did(bound, tier):
    src = keyed_source(bound, T.TIER_NAMES.index(tier))
    assert "0x80808080u" not in src and "const bool U0" not in src
    assert hashlib.sha256(src.encode()).hexdigest() == PARENT_SOURCES[(bound, tier)]
