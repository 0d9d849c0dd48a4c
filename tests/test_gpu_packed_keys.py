"""Packed group keys on the GPU ("Packed keys: a 32-bit key table and the next quad's loads"): FusedAggregationOperator
over device pages with two VARCHAR(1) keys, and with a nullable (BOOLEAN, VARCHAR(3)) pair, whose few-groups kernels keep a 32-bit key
table and load a lane's next quad ahead.  Every case is checked against the oracle with the tolerance of tests/test_gpu_fused.py
(DOUBLE sums to 1e-9, keys and counts exact), and the loop that loads ahead against the plain loop (PRESTO_AMD_LDS_PIPE=0) bit for
bit: both walk a lane's quads and a quad's rows in the same order."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from presto_amd import abi
from presto_amd._lib import PrestoAmdError, lib
from presto_amd.expr import constant, field
from presto_amd.operators import FusedAggregationOperator, fused_aggregation_desc, to_pages, upload_page
from presto_amd.page import Block, Page
from tests.util import rows_equal_ignore_order

pytestmark = pytest.mark.gpu
REL = 1e-9
DAY = 100    # rows with a date <= DAY pass the filter of the VARCHAR(1) shape

VV_TYPES = [abi.VARCHAR, abi.VARCHAR, abi.DOUBLE, abi.DATE]
VV = dict(types=VV_TYPES, params=[1, 1, 0, 0], filter=field(3, abi.DATE) <= constant(DAY, abi.DATE),
          proj=[field(0, abi.VARCHAR), field(1, abi.VARCHAR), field(2, abi.DOUBLE)], group_by=[0, 1],
          aggs=[(abi.AGG_SUM, 2, abi.DOUBLE), (abi.AGG_AVG, 2, abi.DOUBLE), (abi.AGG_COUNT_STAR, -1, None)])
BV_TYPES = [abi.BOOLEAN, abi.VARCHAR, abi.DOUBLE]
BV = dict(types=BV_TYPES, params=[0, 3, 0], filter=None, proj=[field(i, t) for i, t in enumerate(BV_TYPES)], group_by=[0, 1],
          aggs=[(abi.AGG_SUM, 2, abi.DOUBLE), (abi.AGG_COUNT_STAR, -1, None)])


def operator(shape):
    return FusedAggregationOperator(shape["types"], shape["filter"], shape["proj"], shape["group_by"], shape["aggs"], type_params=shape["params"])


def run(shape, pages):
    op = operator(shape)
    try:
        rows = [r for p in to_pages(op, pages) for r in p.to_rows()]
        return rows, op.kernelName()
    finally:
        op.close()


def expected_rows(oracle, shape, pages):
    ref = oracle.HashAggregation([p.type for p in shape["proj"]], shape["group_by"], shape["aggs"])
    for page in pages:
        projected = oracle.filter_project(page, shape["filter"], shape["proj"]) if shape["filter"] is not None else page
        if projected is not None:    # (None: no row of the page passes the filter)
            ref.add_page(projected)
    return ref.build_result().to_rows()


def bits(rows):
    """the rows in a fixed order with every DOUBLE as its bit pattern"""
    return sorted((tuple(v.hex() if isinstance(v, float) else v for v in r) for r in rows), key=repr)


def check(oracle, monkeypatch, shape, pages, few_groups=True):
    """oracle == loop that loads ahead == plain loop (the latter two bit for bit); returns the oracle's rows.  few_groups=False: more
    groups than the wave's table holds, the rows come from the next tier, whose DOUBLE sums are atomic adds in the order of arrival --
    two runs of one kernel differ in the last bits there, so the two loops are compared as each is with the oracle: keys and counts
    exact, sums to REL."""
    expected = expected_rows(oracle, shape, pages)
    dev = [upload_page(p) for p in pages]
    monkeypatch.delenv("PRESTO_AMD_LDS_PIPE", raising=False)
    got, name = run(shape, dev)
    rows_equal_ignore_order(got, expected, rel=REL)
    monkeypatch.setenv("PRESTO_AMD_LDS_PIPE", "0")
    plain, plain_name = run(shape, dev)
    if few_groups:
        assert bits(plain) == bits(got)
    else:
        rows_equal_ignore_order(plain, got, rel=REL)
        rows_equal_ignore_order(plain, expected, rel=REL)
    if few_groups and any(p.position_count >= 256 for p in pages):   # (the vector kernel ran: it is the operator's dominant kernel)
        assert name.startswith("pa_fused_lds_") and plain_name.startswith("pa_fused_lds_") and name != plain_name, (name, plain_name)
    return expected


def unit(n):
    return np.arange(n + 1, dtype=np.int32)


def vv_page(n, seed, k0=b"ANR", k1=b"FO", dates=None):
    rng = np.random.default_rng(seed)
    a = rng.choice(np.frombuffer(k0, dtype=np.uint8), n)
    b = rng.choice(np.frombuffer(k1, dtype=np.uint8), n)
    d = rng.integers(DAY - 50, DAY + 10, n).astype(np.int32) if dates is None else np.full(n, dates, dtype=np.int32)
    return Page([Block.varwidth(a, unit(n)), Block.varwidth(b, unit(n)), Block.double(rng.random(n) * 1e4 - 3e3), Block.date(d)], n)


def head_launch_grid(shape):
    """workgroups (waves) of the few-groups tier's launch over a page that fills the device: launch_lds (op_fused_launch.cpp) takes
    min(quads / 64, CUs x per_cu) with per_cu = clamp(160 KiB / (NW x 8 slots x 64 lanes x 8 B + 512), 1, 16)"""
    d, keep = fused_aggregation_desc(shape["types"], shape["filter"], shape["proj"], shape["group_by"], shape["aggs"], type_params=shape["params"])
    L = lib()
    L.pa_codegen_fused_layout.restype = C.c_int64
    L.pa_codegen_fused_layout.argtypes = [C.c_void_p, C.c_int32, C.c_uint64, C.c_int32, C.c_char_p, C.c_int64]
    need = L.pa_codegen_fused_layout(C.byref(d), 1, 0, 0, None, 0)
    assert need > 0, L.pa_last_error()
    buf = C.create_string_buffer(need)
    L.pa_codegen_fused_layout(C.byref(d), 1, 0, 0, buf, need)
    src = buf.value.decode()
    nw, c = (int(re.search(r"#define %s (\d+)" % m, src).group(1)) for m in ("PA_NW", "PA_C"))
    assert c == 8
    per_cu = max(1, min(16, 160 * 1024 // (nw * c * 64 * 8 + 512)))
    return torch.cuda.get_device_properties(0).multi_processor_count * per_cu


# 256 rows = the 64 quads of one wave.  R = 256 x grid rows give every lane of a full launch exactly one quad (its loads are issued in
# front of the loop and the guarded loads in the loop never run); R + 256 give the first wave's lanes a second one, R - 256 leave the
# launch one wave short of the device.
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1021, "R-256", "R", "R+256"])
def test_row_counts_around_the_prologue_the_last_guarded_loads_and_the_tail(gpu, oracle, monkeypatch, n):
    if isinstance(n, str):
        R = 256 * head_launch_grid(VV)
        assert 1 << 16 <= R <= 1 << 21
        n = R + int(n[1:] or 0)
    expected = check(oracle, monkeypatch, VV, [vv_page(n, n)])
    if n >= 255:
        assert len(expected) == 6


def test_second_page_without_a_row_that_passes_the_filter(gpu, oracle, monkeypatch):
    """two launches; the second one's rows all fail the filter and must leave the first one's groups as they are"""
    pages = [vv_page(5 * 256 + 3, 1), vv_page(3 * 256 + 1, 2, k0=b"XYZ", dates=DAY + 1)]
    expected = check(oracle, monkeypatch, VV, pages)
    assert len(expected) == 6 and all(r[0] in (b"A", b"N", b"R") for r in expected)


@pytest.mark.parametrize("groups", [1, 8, 9])
def test_one_group_a_full_table_and_one_group_too_many(gpu, oracle, monkeypatch, groups):
    """8 groups fill the wave's table; with 9 the wave overflows and the exact result comes from the next tier"""
    k0 = {1: b"A", 8: b"ABCD", 9: b"ABC"}[groups]
    k1 = {1: b"F", 8: b"FO", 9: b"FOP"}[groups]
    expected = check(oracle, monkeypatch, VV, [vv_page(40 * 256 + 77, groups, k0=k0, k1=k1)], few_groups=groups <= 8)
    assert len(expected) == groups


def test_a_group_first_seen_in_the_last_quad(gpu, oracle, monkeypatch):
    n = 64 * 256
    page = vv_page(n, 3, dates=DAY)
    page.blocks[0].values[n - 4:] = ord("Q")      # the last quad of the last wave's last lane
    expected = check(oracle, monkeypatch, VV, [page])
    late = [r for r in expected if r[0] == b"Q"]
    assert 1 <= len(late) <= 2 and len(expected) == 6 + len(late) and sum(r[-1] for r in late) == 4


def test_the_key_whose_packed_value_is_zero(gpu, oracle, monkeypatch):
    """two empty VARCHAR(1) strings pack to 0, and so does (false, '') of the other shape: a group of its own next to the others,
    never mistaken for an empty slot of the table.  (The page with empty strings also holds fewer bytes than rows: PB < n, every
    quad loads its offsets behind the guard while the next quad's loads are in flight.)"""
    n = 9 * 256 + 5
    rng = np.random.default_rng(4)
    la, lb = (rng.random(n) < 0.7).astype(np.int32), (rng.random(n) < 0.6).astype(np.int32)
    la[:8], lb[:8] = 0, 0                          # the first quads' rows are the zero key
    oa, ob = np.concatenate([[0], np.cumsum(la)]).astype(np.int32), np.concatenate([[0], np.cumsum(lb)]).astype(np.int32)
    page = Page([Block.varwidth(np.full(max(int(oa[-1]), 1), ord("A"), dtype=np.uint8), oa), Block.varwidth(np.full(max(int(ob[-1]), 1), ord("F"), dtype=np.uint8), ob),
                 Block.double(rng.random(n)), Block.date(np.full(n, DAY, dtype=np.int32))], n)
    expected = check(oracle, monkeypatch, VV, [page])
    assert sorted(r[:2] for r in expected) == [(b"", b""), (b"", b"F"), (b"A", b""), (b"A", b"F")]
    flags = rng.random(n) < 0.5
    words = [b"", b"ab", b"abc"]
    strings = [words[i] for i in rng.integers(0, 3, n)]
    flags[:4], strings[:4] = False, [b""] * 4
    page = Page([Block.boolean(flags), Block.varchar(strings), Block.double(rng.random(n))], n)
    expected = check(oracle, monkeypatch, BV, [page])
    assert len(expected) == 6 and (False, b"") in [r[:2] for r in expected]


def test_null_keys_next_to_the_values_with_the_same_payload(gpu, oracle, monkeypatch):
    """a NULL key packs as payload 0 plus its flag bit: NULL next to false, NULL next to '' -- and all of it in 31 bits, the widest
    packed key (1 + 1 + 28 + 1)"""
    n = 11 * 256 + 9
    rng = np.random.default_rng(5)
    flags, flag_nulls = rng.random(n) < 0.5, rng.random(n) < 0.3
    flags[flag_nulls] = False
    strings = [None if u < 0.3 else (b"" if u < 0.6 else b"abc") for u in rng.random(n)]
    page = Page([Block.boolean(flags, flag_nulls.astype(np.uint8)), Block.varchar(strings), Block.double(rng.random(n))], n)
    expected = check(oracle, monkeypatch, BV, [page], few_groups=False)
    assert len(expected) == 9    # {true, false, NULL} x {NULL, '', 'abc'}: one more than the table holds
    few = Page([Block.boolean(flags, flag_nulls.astype(np.uint8)), Block.varchar([s if s != b"abc" else None for s in strings]),
                Block.double(rng.random(n))], n)
    expected = check(oracle, monkeypatch, BV, [few])
    assert sorted((r[:2] for r in expected), key=repr) == sorted([(f, s) for f in (True, False, None) for s in (None, b"")], key=repr)


def test_quads_that_need_their_offsets(gpu, oracle, monkeypatch):
    """single bytes >= 0x80 (one byte per string: the page qualifies, the quads that hold one do not) send a quad to the offsets it
    loads behind the guard, while the next quad's loads are in flight; a real two-byte code point exceeds the bound the device key
    packing supports for VARCHAR(1) and is refused, as before, by either loop"""
    n = 20 * 256 + 130
    page = vv_page(n, 6, k0=b"A", k1=b"FO")
    rng = np.random.default_rng(7)
    page.blocks[0].values[rng.random(n) < 1 / 50] = 0xE9
    page.blocks[1].values[rng.random(n) < 1 / 50] = 0x80
    expected = check(oracle, monkeypatch, VV, [page])
    assert len(expected) == 6
    lengths = np.ones(n, dtype=np.int32)
    lengths[1000], lengths[1006] = 2, 0     # 'é' and, in the quad behind its own, an empty string: n bytes over n strings
    values = np.full(n, ord("A"), dtype=np.uint8)
    values[1000:1002] = np.frombuffer("é".encode(), dtype=np.uint8)
    two = Page([Block.varwidth(values, np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32))] + page.blocks[1:], n)
    dev = upload_page(two)
    for value in (None, "0"):
        if value is not None:
            monkeypatch.setenv("PRESTO_AMD_LDS_PIPE", value)
        else:
            monkeypatch.delenv("PRESTO_AMD_LDS_PIPE", raising=False)
        with pytest.raises(PrestoAmdError) as err:
            run(VV, [dev])
        assert err.value.status == abi.ERR_NOT_SUPPORTED and "VARCHAR group key longer than its declared bound" in err.value.message
