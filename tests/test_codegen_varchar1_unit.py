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

# sha256 of the generated source on the parent commit: (bound of the VARCHAR key, tier) -> digest (of the whole translation unit, so
# re-taken when the device header in front of the generated text changed -- kernels/pa_args.h -- with the generated text byte-identical)
PARENT_SOURCES = {
    (2, "lds"): "500cb6159a496929ca0cf3292b12a88ed930559332dd171340b9b4533d27f3a1",
    (2, "gt"): "3ecb2d0f4904d2d9efde49fd8ac9b8cfd383dc898b7b0a816ca8a3c0576d394b",
    (2, "lds_ranges"): "50aabf62b3adb2533951e58dc07fa122bcd9202736009607a712884d8a0be3ef",
    (7, "lds"): "66fbe7e7cd74e109757a7c60636ec57c89cbaa3d99ec6f02b75fa4d8283cef54",
    (7, "ldsh"): "9d82aa329a675c5a6829c079fd295430c82b4e6a86f8e5dd2192ebed9d8cf0e3",
    (0, "lds"): "ba84a9dec53c3a4f57d64557e03de2eb0273819ba52f58112e26c37d7d03569c",
    (0, "gt"): "bfa27f004b617f2a8b04a59928d60a329975907cadf0e0de40a3f45d581a2513",
    (12, "ldsh"): "50f2f094a1292101ef571beb99545b58747c0ff6ad70282eeca84a13f7990433",
    (1, "global"): "966f8de711c418a82946be8c13b133fa7580ac82386f5fa89d16837ea0f8619e",
    (1, "global_ranges"): "7995876c6ee291533cd4c591a93f3f640e9f18f60d3e292eec639421a2b3a496",
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
