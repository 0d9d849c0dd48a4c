"""The cache policy of the staged ungrouped kernel's column loads ("Cache policy of the column streams"), off the
GPU, on the Q6 shape (V_GLOBAL_S) and the Q1 shape (V_LDS).

PRESTO_AMD_NT=0 generates the source of before the switch; the sha256 digests were taken from the parent commit.  From level 1 on every
16-byte load of a stage-0 column in the staged page loop goes through __builtin_nontemporal_load, both halves of a quad alike (the
compiler drops the policy from two adjacent loads of which only one asks for it); level 2 wraps the later stages' masked loads too.
Offsets, NULL flags and every other loop keep plain loads: the head loop of the few-groups tier was measured with the policy and keeps
the default one, so the Q1 source does not depend on the switch at all.  Every level compiles for gfx950 (hiprtc in process) under a
kernel name of its own."""
import hashlib
import re

import pytest

from presto_amd import abi, tpch
from presto_amd.operators import fused_aggregation_desc
from tests.test_codegen_packed_keys import kernel_name, translation_unit

V_GLOBAL, V_LDS, V_GT, V_GLOBAL_S = 0, 1, 2, 9
NT = "__builtin_nontemporal_load(pa_p)"   # behind `const T* const pa_p = &<the element>;`
WIDE = re.compile(r"\(\(const pa_(?:f64x2|i64x2|i32x4|f32x4)\*\)a\.v\[(\d+)\]\)")   # a 16-byte load of channel <n>'s values
# sha256 of the generated source on the parent commit (of the whole translation unit, so re-taken when the device header in front of
# the generated text changed -- the argument blocks moved into kernels/pa_args.h -- with the generated text byte-identical)
PARENT = {
    ("q1", V_LDS): "fb5aeddc85e6ba29c4f4dca14228574b00c67c2210313e16a7cd8e55ccaf638b",
    ("q6", V_GLOBAL_S): "feb141fef084aabb29e7120e4277d358008ceb55ee1b181bca32887a023faf45",
    ("q6", V_GLOBAL): "43c3b1f7656c006115b920ccb9d986a0a4052665b0ceb78f3730fd969d899172",
}


def desc(which):
    if which == "q1":
        return fused_aggregation_desc(tpch.Q1_TYPES, tpch.q1_filter(), tpch.q1_projections(), tpch.Q1_GROUP_BY, tpch.Q1_AGGREGATES,
                                      type_params=tpch.Q1_TYPE_PARAMS)
    return fused_aggregation_desc(tpch.Q6_TYPES, tpch.q6_filter(), tpch.q6_projections(), [],
                                  tpch.Q6_AGGREGATES + [(abi.AGG_COUNT_STAR, -1, None)])


def source(monkeypatch, which, variant, nt=None, compile_it=False):
    """the translation unit under PRESTO_AMD_NT = nt (None: not set)"""
    if nt is None:
        monkeypatch.delenv("PRESTO_AMD_NT", raising=False)
    else:
        monkeypatch.setenv("PRESTO_AMD_NT", str(nt))
    monkeypatch.delenv("PRESTO_AMD_LDS_PIPE", raising=False)
    d, keep = desc(which)
    return translation_unit(d, variant, 0, compile_it)


def staged_loop(src):
    """the staged page loop of the ungrouped kernel: from its stage counters to the rows behind the last whole quad"""
    at = src.index("void PA_K(pa_fused_global_staged)(")
    return src[src.index("u32 pa_cnt1 = 0u;", at):src.index("for (i64 r = (nq << 2) + t;", at)]


def wide_loads(text):
    """(line, wrapped) of every line of `text` that loads 16 bytes of a column's values"""
    out = []
    for line in text.split("\n"):
        m = WIDE.search(line)
        if m:
            assert line.count(NT) in (0, 1) and len(WIDE.findall(line)) == 1, line
            assert (NT in line) == ("pa_p = &" + m.group(0) in line), line
            out.append((line, NT in line))
    return out


@pytest.mark.parametrize("which,variant", sorted(PARENT))
def test_level_0_generates_the_parent_source(which, variant, monkeypatch):
    src = source(monkeypatch, which, variant, nt=0)
    assert "__builtin_nontemporal_load" not in src
    assert hashlib.sha256(src.encode()).hexdigest() == PARENT[(which, variant)]


@pytest.mark.parametrize("level", [1, 2])
def test_staged_loop_wraps_the_stages_the_level_covers(level, monkeypatch):
    src = source(monkeypatch, "q6", V_GLOBAL_S, nt=level)
    loop = staged_loop(src)
    loads = wide_loads(loop)
    # nothing outside the loop asks for the policy
    assert loads and src.count("__builtin_nontemporal_load") == loop.count("__builtin_nontemporal_load")
    # holder 0 keeps the columns of stage 0 -- those every row reads; the later holders' loads are the masked later-stage loads
    stage0 = [wrapped for line, wrapped in loads if re.search(r"\bh0_[AB]\d+ = ", line)]
    later = [wrapped for line, wrapped in loads if not re.search(r"\bh0_[AB]\d+ = ", line)]
    assert len(stage0) == 2 and len(later) >= 6   # Q6: the DATE column in front of and inside the loop; three DOUBLE columns behind it
    assert all(stage0)
    assert all(wrapped == (level == 2) for wrapped in later)
    # both halves of a quad alike
    for line, wrapped in loads:
        m = re.search(r"\b(h\d+_)A(\d+) = ", line)
        if m and "pa_f64x2" in line:
            other = [w for l, w in loads if re.search(r"\b%sB%s = " % (m.group(1), m.group(2)), l)]
            assert other and all(w == wrapped for w in other)
    # NULL flags and offsets keep plain loads
    assert not any("__builtin_nontemporal_load" in line for line in loop.split("\n") if "a.nl[" in line or "a.o[" in line)


def test_the_default_level_is_1(monkeypatch):
    assert source(monkeypatch, "q6", V_GLOBAL_S) == source(monkeypatch, "q6", V_GLOBAL_S, nt=1)


def test_levels_compile_under_names_of_their_own(monkeypatch):
    names = set()
    for level in (0, 1, 2):
        source(monkeypatch, "q6", V_GLOBAL_S, nt=level, compile_it=True)
        names.add(kernel_name(source(monkeypatch, "q6", V_GLOBAL_S, nt=level)))
    assert len(names) == 3


def test_other_kernels_do_not_depend_on_the_switch(monkeypatch):
    """the plain ungrouped kernel of Q6, the few-groups and the table tier of Q1 generate one source under every level"""
    for which, variant in (("q6", V_GLOBAL), ("q1", V_LDS), ("q1", V_GT)):
        srcs = {source(monkeypatch, which, variant, nt=level) for level in (0, 1, 2)}
        assert len(srcs) == 1 and "__builtin_nontemporal_load" not in srcs.pop()
