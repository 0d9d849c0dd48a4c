"""The group keys of the fused aggregation at edge values, against the key model (tests/key_model.py) -- not the C oracle: every edge key
of key_model.KEY_EDGES goes through every tier (each leg asserts the tier by the kernel's name) of every shape of key_model.SHAPES.

Every operator computes count(*), sum(arrival index) and min(arrival index) grouped by the shape's keys: exact integers, so a row that
lands in a wrong group changes an answer.  Keys are compared by bit pattern (key_model.emitted), block types are checked, and the
number of output rows is the number of groups: a group that comes out twice, or two groups that come out as one, fail.

One JIT compilation costs more than all launches of a leg, so the legs of a (shape, tier) share one operator description -- the plan
cache serves every page of every leg.

CELLS classifies every (shape, tier): EXACT in the tier's own kernel, OTHER (computed exactly by another tier's kernel, named there) or
REFUSED (NOT_SUPPORTED), the last two with what decides it in the code.
"""
import collections
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from presto_amd import abi
from presto_amd._lib import PrestoAmdError
from presto_amd.exchange import partial_layout
from presto_amd.expr import field
from presto_amd.operators import (Driver, FusedAggregationOperator, FusedJoinAggregationOperator, HashBuilderOperator, LookupSourceFactory, download_page,
                                  to_pages, upload_page)
from presto_amd.page import Block, Page
from tests import key_model as K

on_gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOT_SUPPORTED = abi.ERR_NOT_SUPPORTED

TIERS = ["lds", "ldsh", "ldsp", "gt"]
PREFIX = {"lds": "pa_fused_lds_", "ldsh": "pa_fused_ldsh_", "ldsp": "pa_fused_ldsp_", "gt": "pa_fused_gt_", "probe": "pa_fused_probe_"}
MANY = (1 << 20) + 1            # expected_groups beyond 2^20: the HBM table at once (op_fused.cpp: mode_ = ... V_GT), the partition-owned tables in front of it
BATCH = {"lds": 6, "ldsh": 48}  # groups per operator: within the 8 slots of the few-groups tier; past them, within the workgroup's table
FILLERS, EMITTER_FILLERS = 3000, 5200       # below / above the 4096 groups from which the device emits the result (op_fused_output.cpp: kMinGroups)

EXACT, OTHER, REFUSED = "EXACT", "OTHER", "REFUSED"
# the tiers a multi-key shape runs in: one LDS tier and the HBM table
MULTI_TIERS = {"integer_integer_nn": ["lds", "gt"], "integer_date_boolean": ["ldsh", "gt"], "boolean_varchar3": ["lds", "gt"],
               "varchar15_bigint_varchar2": ["ldsh", "gt"], "bigint_x8_nn": ["lds", "gt"]}
# (shape, tier) -> (state, the tier whose kernel computes it or None, what decides it)
NOT_EXACT = {
    ("boolean", "ldsh"): (OTHER, "lds", "three groups (true, false, NULL) never fill the 8 slots of the few-groups tier, and only its overflow moves an operator on "
                                        "(op_fused_launch.cpp run_tiers: `mode_ = V_LDSH` after a launch that reported overflow)"),
}
# a variable-width input column keeps the position list of the hash-partitioned pass, which the workgroup-table kernel walks; only 1-, 4-
# and 8-byte columns are regrouped for the partition-owned tables.  (VARCHAR without a bound is grouped by its interned id, a 4-byte column.)
for _name in ("varchar1", "varchar7", "varchar15"):
    NOT_EXACT[(_name, "ldsp")] = (OTHER, "ldsh", "op_fused_table.cpp run_page_partitioned: `ldsp = !dp.cols[c].varwidth && type_width(dp.cols[c].type) <= 8`, "
                                                 "then `kernel_for(sig, layout, ldsp ? V_LDSP : V_LDSH)`")
CELLS = collections.OrderedDict()
for _s in K.SHAPES.values():
    for _t in (TIERS if len(_s.parts) == 1 else MULTI_TIERS[_s.name]):
        CELLS[(_s.name, _t)] = NOT_EXACT.get((_s.name, _t), (EXACT, None, ""))


def cells(kind):
    return [c for c in CELLS if (len(K.SHAPES[c[0]].parts) == 1) == (kind == "single")]


# ---- the keys a cell is fed --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def filler_keys(shape_name, count):
    """further keys of the shape, each different from every edge key: the fillers of the first part next to zeros"""
    shape = K.SHAPES[shape_name]
    zero = [K.special(p.label)["zero"] for p in shape.parts]
    at = next((i for i, p in enumerate(shape.parts) if K.base(p.label) != "BOOLEAN"), None)
    if at is None:
        return []
    edges = {K.key_identity(shape, k) for k in K.edge_keys(shape)}
    out = []
    for v in K.fillers(shape.parts[at].label, count + 64, 7):
        k = tuple(zero[:at] + [v] + zero[at + 1:])
        if K.key_identity(shape, k) not in edges and len(out) < count:
            out.append(k)
    return out


@functools.lru_cache(maxsize=None)
def batches(shape_name, tier, fill=FILLERS):
    """the operators' key lists for a cell.  lds / ldsh: the edge keys cut into lists of BATCH[tier] groups, all of one size (a last list
    of a few groups would stay in the tier below), an ldsh list topped up with filler keys; ldsp / gt: all edge keys and `fill` filler keys"""
    shape = K.SHAPES[shape_name]
    keys = K.edge_keys(shape)
    if tier in ("ldsp", "gt"):
        return [keys + filler_keys(shape_name, fill)]
    groups = collections.OrderedDict()
    for k in keys:
        groups.setdefault(K.key_identity(shape, k), []).append(k)
    groups = list(groups.values())
    count = max(1, -(-len(groups) // BATCH[tier]))
    size = -(-len(groups) // count)
    out = []
    for i in range(0, len(groups), size):
        batch = [k for g in groups[i:i + size] for k in g]
        if tier == "ldsh":
            batch = batch + filler_keys(shape_name, BATCH[tier])[:max(0, BATCH[tier] - len(groups[i:i + size]))]
        out.append(batch)
    return out


def fed(shape_name, tier):
    return [k for b in batches(shape_name, tier) for k in b]


def test_every_cell_is_classified():
    for name, shape in K.SHAPES.items():
        for tier in (TIERS if len(shape.parts) == 1 else MULTI_TIERS[name]):
            state, other, why = CELLS[(name, tier)]
            assert state in (EXACT, OTHER, REFUSED), (name, tier)
            if state != EXACT:
                assert why and (state == REFUSED or other in PREFIX), (name, tier)
        if len(shape.parts) == 1:
            assert CELLS[(name, "gt")][0] == EXACT, name
            assert any(CELLS[(name, t)][0] == EXACT for t in ("lds", "ldsh", "ldsp")), name
        else:
            assert "gt" in MULTI_TIERS[name] and any(t in MULTI_TIERS[name] for t in ("lds", "ldsh", "ldsp")), name
    assert set(CELLS) >= set(NOT_EXACT)


def test_every_edge_key_is_fed_to_every_cell():
    """on the CPU: no leg drops an edge key silently -- every entry of KEY_EDGES (and NULL where the part is nullable) reaches every EXACT
    and OTHER cell of every shape that has a part of its type, in every position, and so do the pairs that differ only in where a value sits"""
    for (name, tier), (state, _, _) in CELLS.items():
        if state == REFUSED:
            continue
        shape = K.SHAPES[name]
        keys = fed(name, tier)
        assert set(K.edge_keys(shape)) <= set(keys), (name, tier)
        for i, p in enumerate(shape.parts):
            have = {k[i] for k in keys}
            assert set(K.part_values(p)) <= have, (name, tier, i)
        for i in range(len(shape.parts)):
            for j in range(len(shape.parts)):
                if i == j:
                    continue
                si, sj = K.special(shape.parts[i].label), K.special(shape.parts[j].label)
                pairs = {(k[i], k[j]) for k in keys}
                assert {(si["ones"], sj["zero"]), (si["zero"], sj["ones"]), (si["min"], sj["max"]), (si["max"], sj["min"])} <= pairs, (name, i, j)
                if shape.parts[i].nullable:
                    assert (None, sj["zero"]) in pairs, (name, i, j)
                if shape.parts[j].nullable:
                    assert (si["zero"], None) in pairs, (name, i, j)
        # an lds list stays within the few-groups tier, an ldsh list goes past it
        for b in batches(name, tier):
            n = len({K.key_identity(shape, k) for k in b})
            if tier == "lds":
                assert n <= 8, (name, n)
            if tier == "ldsh" and state == EXACT:
                assert n > 8, (name, n)
    for name in ("bigint", "bigint_nn", "integer_nn", "integer", "date", "double", "real"):
        for tier in ("ldsp", "gt"):
            assert len({K.key_identity(K.SHAPES[name], k) for k in batches(name, tier, EMITTER_FILLERS)[0]}) >= 5000


# ---- operators and pages ---------------------------------------------------------------------------------------------------------------------------
class Plan:
    """the key channels, the arrival index[, a $hashvalue channel] -> identity projections, count(*), sum and min of the arrival index"""

    def __init__(self, shape, hashed=False):
        self.shape, self.hashed = shape, hashed
        self.nkeys = len(shape.parts)
        self.input_types = [K.type_of(p.label) for p in shape.parts] + [abi.BIGINT] + ([abi.BIGINT] if hashed else [])
        self.type_params = [K.type_param(p.label) for p in shape.parts] + [0] + ([0] if hashed else [])
        self.projections = [field(i, t) for i, t in enumerate(self.input_types)]
        self.group_by = list(range(self.nkeys))
        self.aggregates = [(abi.AGG_COUNT_STAR, -1, None), (abi.AGG_SUM, self.nkeys, abi.BIGINT), (abi.AGG_MIN, self.nkeys, abi.BIGINT)]

    def operator(self, tier, output_mem=abi.MEM_HOST, step=abi.STEP_SINGLE, expected_groups=None):
        kw = dict(type_params=self.type_params, output_mem=output_mem, step=step)
        if expected_groups is not None:
            kw["expected_groups"] = expected_groups
        elif tier in ("ldsp", "gt"):
            kw["expected_groups"] = MANY
        if self.hashed:
            kw["hash_channel"] = self.nkeys + 1
        return FusedAggregationOperator(self.input_types, None, self.projections, self.group_by, self.aggregates, **kw)

    def page(self, keys, first, oracle=None):
        blocks = [K.key_block(p.label, [k[i] for k in keys], p.nullable) for i, p in enumerate(self.shape.parts)]
        blocks.append(Block.bigint(np.arange(first, first + len(keys), dtype=np.int64)))
        if self.hashed:     # as the planner's HashGenerationOptimizer would have computed it
            blocks.append(Block.bigint(oracle.hash_page(Page(blocks[:self.nkeys], len(keys)), self.group_by)))
        return Page(blocks, len(keys))


def tier_env(monkeypatch, tier):
    if tier == "gt":
        monkeypatch.setenv("PRESTO_AMD_NO_PARTITIONED", "1")     # the HBM table's own kernel
    else:
        monkeypatch.delenv("PRESTO_AMD_NO_PARTITIONED", raising=False)


# name -> (order, rows per page; None: one page).  A key's rows lie len(keys) rows apart in "strided": in different lanes, waves,
# workgroups (4 rows per lane, 256 lanes) and pages.  "adjacent": runs of one key -- 68 rows in the few-groups tier (a wave's lanes and
# the next wave's first), 4 rows elsewhere (one lane's quad; longer runs would leave a wave with 8 keys at most, and the operator in
# the few-groups tier) --, the runs repeated
LAYOUTS = collections.OrderedDict([
    ("adjacent", ("group", None)),
    ("strided", ("round", 1027)),           # ragged pages, the last one below 256 rows (the row-by-row tail)
    ("workgroups", ("round", None)),        # one page of more than 4096 rows
])
MIN_ROWS = 4200                             # (not a multiple of 256: the head kernel and the tail)


def lay_out(keys, layout, tier):
    """-> pages (lists of keys): every key on at least two rows, MIN_ROWS rows at least"""
    order, page_rows = LAYOUTS[layout]
    if order == "group":
        run = 68 if tier == "lds" else 4
        seq = [k for k in keys for _ in range(run)]
        seq = seq * max(1, -(-MIN_ROWS // len(seq)))
    else:
        seq = list(keys) * max(2, -(-MIN_ROWS // len(keys)))
    if page_rows is None:
        return [seq]
    return [seq[i:i + page_rows] for i in range(0, len(seq), page_rows)]


def expected_of(shape, pages, times=1):
    """{emitted key: (count, sum, min)} of the model; times: every row counted that often (FINAL over repeated states)"""
    groups, at = collections.OrderedDict(), 0
    for page in pages:
        for k in page:
            g = groups.setdefault(K.key_identity(shape, k), [K.key_emitted(shape, k), 0, 0, at])
            g[1] += 1
            g[2] += at
            at += 1
    return {g[0]: (g[1] * times, g[2] * times, g[3]) for g in groups.values()}


def result_of(shape, pages, hashed=False, lead_types=None):
    """output pages -> ({emitted key: the other columns}, number of rows); block types checked"""
    out, n = {}, 0
    for p in pages:
        p = p if p.mem == abi.MEM_HOST else download_page(p)
        want = [int(K.type_of(q.label)) for q in shape.parts] + ([int(abi.BIGINT)] if hashed else [])
        assert [int(b.type) for b in p.blocks[:len(want)]] == want, ([b.type for b in p.blocks], want)
        assert all(int(b.type) == int(abi.BIGINT) for b in p.blocks[len(want):])
        cols = [K.column_patterns(b, q.label) for b, q in zip(p.blocks, shape.parts)]
        rest = [b.to_pylist() for b in p.blocks[len(shape.parts):]]
        for i in range(p.position_count):
            out[tuple(c[i] for c in cols)] = tuple(c[i] for c in rest)
            n += 1
    return out, n


def assert_same(got, rows, want, where):
    assert rows == len(got), ("a group came out more than once", rows, len(got)) + where
    missing = [k for k in want if k not in got]
    extra = [k for k in got if k not in want]
    assert not missing and not extra, ("missing", missing[:4], "unexpected", extra[:4]) + where
    wrong = [(k, got[k], want[k]) for k in want if got[k] != want[k]]
    assert not wrong, (len(wrong), wrong[:4]) + where


def run(plan, tier, pages, device_pages=False, output_mem=abi.MEM_HOST, oracle=None, expected_groups=None):
    """-> ({emitted key: (count, sum, min)} or with the hash in front, rows, kernel name)"""
    op = plan.operator(tier, output_mem=output_mem, expected_groups=expected_groups)
    try:
        host, at = [], 0
        for keys in pages:
            host.append(plan.page(keys, at, oracle))
            at += len(keys)
        out = to_pages(op, [upload_page(p) for p in host] if device_pages else host)
        got, rows = result_of(plan.shape, out, plan.hashed)
        return got, rows, op.kernelName()
    finally:
        op.close()


def compare(plan, tier, keys, layout, kernel_tier=None, oracle=None, **kw):
    pages = lay_out(keys, layout, tier)
    got, rows, kernel = run(plan, tier, pages, oracle=oracle, **kw)
    where = (plan.shape.name, tier, layout, kernel)
    assert kernel.startswith(PREFIX[kernel_tier or tier]), where
    want = expected_of(plan.shape, pages)
    if plan.hashed:
        ks = list(want)
        back = {K.key_emitted(plan.shape, k): k for page in pages for k in page}
        hashes = K.hash_of(oracle, plan.shape, [back[k] for k in ks])
        want = {k: (h,) + want[k] for k, h in zip(ks, hashes)}
    assert_same(got, rows, want, where)


# ---- leg 1: every cell ---------------------------------------------------------------------------------------------------------------------------------
def run_cell(monkeypatch, name, tier):
    state, other, _ = CELLS[(name, tier)]
    shape = K.SHAPES[name]
    tier_env(monkeypatch, tier)
    plan = Plan(shape)
    if state == REFUSED:
        with pytest.raises(PrestoAmdError) as e:
            compare(plan, tier, batches(name, tier)[0], "adjacent")
        assert e.value.status == NOT_SUPPORTED, e.value
        return
    kernel_tier = tier if state == EXACT else other
    for n, keys in enumerate(batches(name, tier)):
        keys = list(keys)
        for k, layout in enumerate(LAYOUTS):
            if tier in ("lds", "ldsh") and n and (n + k) % 2:
                continue                    # (several small lists: the first takes every layout, the others every second one)
            compare(plan, tier, keys, layout, kernel_tier)
        compare(plan, tier, keys, "strided" if n % 2 else "workgroups", kernel_tier, device_pages=True)


@on_gpu
@pytest.mark.parametrize("name,tier", cells("single"))
def test_single_key(gpu, monkeypatch, name, tier):
    run_cell(monkeypatch, name, tier)


@on_gpu
@pytest.mark.parametrize("name,tier", cells("multi"))
def test_multi_key(gpu, monkeypatch, name, tier):
    run_cell(monkeypatch, name, tier)


# ---- leg 2: the device emitter (4096 groups and more; never VARCHAR or DECIMAL keys) ------------------------------------------------------------------
DEVICE_EMITTED = ["bigint", "bigint_nn", "integer_nn", "integer", "date", "double", "real", "integer_integer_nn", "integer_date_boolean", "bigint_x8_nn"]


@on_gpu
@pytest.mark.parametrize("tier", ["ldsp", "gt"])
@pytest.mark.parametrize("name", DEVICE_EMITTED)
def test_device_emitter(gpu, oracle, monkeypatch, name, tier):
    """the result decoded from the packed key words by gt_emit_value, into device and into host memory, and once more with $hashvalue
    rebuilt from the key by type"""
    tier_env(monkeypatch, tier)
    keys = list(batches(name, tier, EMITTER_FILLERS)[0])
    assert len({K.key_identity(K.SHAPES[name], k) for k in keys}) >= 5000
    for hashed in (False, True):
        if hashed and len(K.SHAPES[name].parts) > 1 and tier == "ldsp":
            continue                        # (the multi-key shapes: their tiers are thinned first)
        plan = Plan(K.SHAPES[name], hashed)
        compare(plan, tier, keys, "workgroups", oracle=oracle, output_mem=abi.MEM_DEVICE)
        compare(plan, tier, keys, "strided", oracle=oracle, output_mem=abi.MEM_HOST, device_pages=True)


@on_gpu
@pytest.mark.parametrize("name", list(K.SHAPES))
def test_host_emitter_hash(gpu, oracle, monkeypatch, name):
    """below 4096 groups the host decodes the key words (assemble_output) and rebuilds $hashvalue from the decoded key by type: every
    shape, the VARCHAR and DECIMAL keys the device emitter never sees among them"""
    tier_env(monkeypatch, "gt")
    keys = list(batches(name, "gt")[0])
    assert len({K.key_identity(K.SHAPES[name], k) for k in keys}) < 4096
    compare(Plan(K.SHAPES[name], hashed=True), "gt", keys, "strided", oracle=oracle)


# ---- leg 3: growth from the planner's default estimate -------------------------------------------------------------------------------------------------
GROWN = [s.name for s in K.SINGLE if s.name not in ("boolean", "varchar1")] + ["integer_integer_nn"]


GROWTH_ROWS = (1 << 18) + 8000      # past the launch that tells the cardinality (op_fused.hpp: kProbeRows = 2^18 rows)


# A plan remembers between operators what the first launch of the few-groups tier found (op_fused.hpp: Compiled::lds_verdict), and an
# operator that finds "it fitted" sends its first launch out whole and learns late that it did not (confirm_oldest's redo).  So the leg
# says which of the two an operator finds: a run of a few groups, or of more than the tier's 8 slots, goes first.
HISTORIES = collections.OrderedDict([("after_an_overflow", "ldsh"), ("after_a_fit", "lds")])


@on_gpu
@pytest.mark.parametrize("history", list(HISTORIES))
@pytest.mark.parametrize("name", GROWN)
def test_growth(gpu, monkeypatch, name, history):
    """about 20 000 groups under the default expected_groups, every edge key among them, a key's rows in different pages.  The few-groups
    tier gives up on the first rows; the workgroups' LDS tables take the first 2^18 rows, flush into the HBM table -- which is made for
    10 000 groups, spills, grows by rehashing and replays what it spilled -- and find more groups than they have room for; the rows past
    2^18 go to the HBM table's own kernel, whose name the operator has at the end.  (Pages below 2^21 rows are collected and launched
    together, so the leg takes more than 2^18 rows: fewer never leave the workgroups' tables.)  after_a_fit: the same rows behind a first
    launch that went out whole; the redo ends in the workgroups' tables or in the HBM table's kernel."""
    monkeypatch.setenv("PRESTO_AMD_NO_PARTITIONED", "1")
    shape = K.SHAPES[name]
    plan = Plan(shape)
    first = HISTORIES[history]
    compare(plan, first, list(batches(name, "lds")[0]) if first == "lds" else list(batches(name, "gt", 48)[0])[-48:], "strided")
    keys = list(batches(name, "gt", 20000)[0])
    assert len(keys) > 15000, len(keys)
    seq = keys * -(-GROWTH_ROWS // len(keys))
    pages = [seq[i:i + 65537] for i in range(0, len(seq), 65537)]
    op = plan.operator("lds")
    try:
        host, at = [], 0
        for page in pages:
            host.append(plan.page(page, at))
            at += len(page)
        got, rows = result_of(shape, to_pages(op, host))
        kernel = op.kernelName()
    finally:
        op.close()
    assert_same(got, rows, expected_of(shape, pages), (name, kernel))
    assert kernel.startswith(PREFIX["gt"]) or (history == "after_a_fit" and kernel.startswith(PREFIX["ldsh"])), kernel


@on_gpu
def test_growth_on_a_scrubbed_pool(gpu):
    """every recycled HBM block overwritten with 0xA5 before it is handed out -- the pattern new key arrays are cleared with, and the
    key that BIGINT and (INTEGER, INTEGER) hold among their edges: a table that took a block's content for keys fails here.  (The shapes
    whose keys hold the pattern, whole or in a half, and one of each other width.)"""
    env = dict(os.environ, PRESTO_AMD_POOL_SCRUB="0xA5")
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider", "tests/test_gpu_group_key_edges.py", "-k",
                        "test_growth and after_an_overflow and (bigint or integer or double or varchar15)"], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    tail = r.stdout.decode()[-3000:]
    assert r.returncode == 0, tail
    assert " passed" in tail and "failed" not in tail


# ---- leg 4: equal tags ----------------------------------------------------------------------------------------------------------------------------------
@on_gpu
@pytest.mark.parametrize("tier", ["gt", "ldsp"])
def test_equal_tags(gpu, monkeypatch, tier):
    """300 000 random 64-bit keys and the edges, each on two rows.  A table's tag is a 32-bit hash of the key: whatever the hash, n^2 / 2^33
    (about 10) pairs of these keys share all 32 bits (none with probability e^-10) and are told apart by their key words alone"""
    tier_env(monkeypatch, tier)
    rng = np.random.default_rng(20260)
    edges = np.asarray(K.KEY_EDGES["BIGINT"], dtype=np.int64)
    keys = np.unique(np.concatenate([edges, rng.integers(-2 ** 63, 2 ** 63 - 1, 300000, dtype=np.int64, endpoint=True)]))
    keys = keys[rng.permutation(len(keys))]
    n = len(keys)
    assert n >= 300000
    column = np.concatenate([keys, keys])
    plan = Plan(K.SHAPES["bigint"])
    op = plan.operator(tier)
    try:
        pages = []
        for at in range(0, 2 * n, 1 << 17):
            m = min(1 << 17, 2 * n - at)
            pages.append(Page([Block(abi.BIGINT, abi.FLAT, m, values=np.ascontiguousarray(column[at:at + m]), nulls=np.zeros(m, dtype=np.uint8)),
                               Block.bigint(np.arange(at, at + m, dtype=np.int64))], m))
        out = to_pages(op, pages)
        kernel = op.kernelName()
    finally:
        op.close()
    assert kernel.startswith(PREFIX[tier]), kernel
    cols = [[], [], [], []]
    for p in out:
        for c, b in zip(cols, p.blocks):
            assert b.nulls is None or not b.nulls.any()
            c.append(np.asarray(b.values[:p.position_count]))
    got_keys, counts, sums, mins = [np.concatenate(c) for c in cols]
    order = np.argsort(got_keys, kind="stable")
    want = np.argsort(keys, kind="stable")
    assert len(got_keys) == n and np.array_equal(got_keys[order], keys[want])
    assert (counts == 2).all()
    assert np.array_equal(mins[order], want) and np.array_equal(sums[order], 2 * want + n)


# ---- leg 5: PARTIAL per page -> FINAL ------------------------------------------------------------------------------------------------------------------
def run_partial_final(plan, tier, pages):
    """every page through a PARTIAL operator of its own; the keys it emitted are packed again by one FINAL operator over all states, the
    states repeated until there are 300 rows of them (a page below 256 rows goes row by row and leaves no kernel name)
    -> (result, rows, times the states were repeated)"""
    shape, parts, at = plan.shape, [], 0
    for keys in pages:
        op = plan.operator(tier, step=abi.STEP_PARTIAL)
        try:
            parts += to_pages(op, [plan.page(keys, at)])
            assert len(keys) < 256 or op.kernelName().startswith(PREFIX[tier]), (tier, op.kernelName())
        finally:
            op.close()
        at += len(keys)
    ptypes, faggs = partial_layout([K.type_of(p.label) for p in shape.parts], plan.aggregates)
    nk = plan.nkeys
    key_cols, state_cols = [[] for _ in range(nk)], [[] for _ in range(len(ptypes) - nk)]
    for p in parts:
        assert [int(b.type) for b in p.blocks] == [int(t) for t in ptypes]
        for i, q in enumerate(shape.parts):
            vals = K.column_patterns(p.blocks[i], q.label)
            if K.base(q.label) in ("DOUBLE", "REAL"):
                vals = [None if v is None else (K.F64 if K.base(q.label) == "DOUBLE" else K.F32)(v) for v in vals]
            key_cols[i] += vals
        for c, b in zip(state_cols, p.blocks[nk:]):
            c += b.to_pylist()
    times = max(1, -(-300 // len(key_cols[0])))
    blocks = [K.key_block(q.label, key_cols[i] * times, True) for i, q in enumerate(shape.parts)]
    for c in state_cols:
        b = Block.bigint(c * times)
        b.nulls = np.zeros(b.position_count, dtype=np.uint8)
        blocks.append(b)
    kw = dict(expected_groups=MANY) if tier == "gt" else {}
    fin = FusedAggregationOperator(ptypes, None, [field(i, t) for i, t in enumerate(ptypes)], list(range(nk)), faggs, step=abi.STEP_FINAL,
                                   type_params=[K.type_param(q.label) for q in shape.parts] + [0] * (len(ptypes) - nk), **kw)
    try:
        out = to_pages(fin, [Page(blocks, len(blocks[0].nulls))])
        assert fin.kernelName().startswith(PREFIX[tier]), (tier, fin.kernelName())
        return result_of(shape, out) + (times,)
    finally:
        fin.close()


@on_gpu
@pytest.mark.parametrize("name,tier", [(s.name, "gt") for s in K.SINGLE] + [("double", "lds"), ("integer", "lds")])
def test_partial_final(gpu, monkeypatch, name, tier):
    """the FINAL step packs the keys the PARTIAL steps emitted once more: the canonical zero and NaN stay what they are (every NaN
    and both zeros of the input end in one group each), NULL stays NULL"""
    tier_env(monkeypatch, tier)
    shape = K.SHAPES[name]
    plan = Plan(shape)
    for keys in batches(name, tier):
        pages = lay_out(list(keys), "strided", tier)
        got, rows, times = run_partial_final(plan, tier, pages)
        assert_same(got, rows, expected_of(shape, pages, times), (name, tier, "FINAL"))


# ---- leg 6: the probe tier: group keys from build columns ----------------------------------------------------------------------------------------------------
BUILD = ["INTEGER", "DATE", "DOUBLE", "BOOLEAN"]          # the build column types the probe kernel loads (fused_tier_probe.cpp probe_build_loads)
# a build column of another type among the group keys: OTHER -- refused by the one-kernel form when the operator is created
# (fused_plan.cpp make_spec, build_proj: "the fused probe reads BIGINT / INTEGER / DATE / DOUBLE / BOOLEAN build columns"), so the
# FilterAndProject -> LookupJoin -> HashAggregation chain computes it (op_fused_join.cpp: "run as the chain"), exactly
BUILD_OTHER = ["REAL", "DECIMAL"]


def probe_case(groups, labels):
    """build rows: join key 1000 + 3 i (unique), build columns walking their edge values and NULL at strides of their own; every build row is
    probed twice, one probe key in four matches nothing"""
    cols = []
    for c, label in enumerate(labels):
        vals = K.KEY_EDGES[label] + [None]
        cols.append([vals[(i * (c + 1) + i // len(vals)) % len(vals)] for i in range(groups)])
    join_keys = [1000 + 3 * i for i in range(groups)]
    probe = join_keys + [k + 1 for k in join_keys[::2]] + join_keys
    return join_keys, cols, probe


def run_probe(groups, labels, in_probe_kernel=True):
    join_keys, cols, probe = probe_case(groups, labels)
    types = [K.type_of(label) for label in labels]
    bridge = LookupSourceFactory()
    builder = HashBuilderOperator(bridge, [abi.BIGINT] + types, [0], list(range(1, len(labels) + 1)))
    probe_types = [abi.BIGINT, abi.BIGINT]
    joined = probe_types + types
    aggs = [(abi.AGG_COUNT_STAR, -1, None), (abi.AGG_SUM, 1, abi.BIGINT), (abi.AGG_MIN, 1, abi.BIGINT)]
    op = None
    try:
        build_page = Page([Block.bigint(join_keys)] + [K.key_block(label, col, True) for label, col in zip(labels, cols)], groups)
        Driver([build_page], [builder]).run()
        op = FusedJoinAggregationOperator(bridge, probe_types, None, [field(0, abi.BIGINT), field(1, abi.BIGINT)], [0], [0, 1], joined,
                                          [0] + list(range(2, 2 + len(labels))), aggs, type_params=[0, 0])
        pages = []
        for at in range(0, len(probe), 4099):
            part = probe[at:at + 4099]
            pages.append(Page([Block.bigint(part), Block.bigint(np.arange(at, at + len(part), dtype=np.int64))], len(part)))
        out = to_pages(op, pages)
        kernel = op.kernelName()
    finally:
        if op is not None:
            op.close()
        builder.close()
    assert kernel.startswith("pa_fused_") and kernel.startswith(PREFIX["probe"]) == in_probe_kernel, kernel
    shape = K.Shape("probe", [K.Part("BIGINT", True)] + [K.Part(label, True) for label in labels])
    got, rows = result_of(shape, out)
    want = {}
    for i, k in enumerate(join_keys):
        key = (k,) + tuple(K.emitted(label, col[i]) for label, col in zip(labels, cols))
        want[key] = (2, i + (len(probe) - groups + i), i)
    assert_same(got, rows, want, ("probe", groups, kernel))


@on_gpu
@pytest.mark.parametrize("groups", [3000, 6000])
def test_probe_tier(gpu, groups):
    """group keys that are build columns (pa_brow_keys packs them once per group): below 4096 groups the host decodes the key words,
    from there on the device emits the result"""
    run_probe(groups, BUILD)


@on_gpu
@pytest.mark.parametrize("label", BUILD_OTHER)
def test_probe_tier_other_build_columns(gpu, label):
    run_probe(6000, BUILD + [label], in_probe_kernel=False)


# ---- leg 7: limits ----------------------------------------------------------------------------------------------------------------------------------------
def refused_run(plan, pages, tier="lds"):
    """NOT_SUPPORTED from the creation or from a page; no row comes out"""
    out = []
    with pytest.raises(PrestoAmdError) as e:
        op = plan.operator(tier)
        try:
            out += to_pages(op, pages)
        finally:
            op.close()
    assert e.value.status == NOT_SUPPORTED, e.value
    assert not out


@on_gpu
def test_nine_key_words_are_refused(gpu):
    nine = K.Shape("bigint_x9_nn", [K.Part("BIGINT", False)] * 9)
    plan = Plan(nine)
    refused_run(plan, [plan.page([(1,) * 9] * 300, 0)])
    # eight keys without null arrays are eight words; a page that brings one null array needs a ninth for the flag
    plan = Plan(K.SHAPES["bigint_x8_nn"])
    first = plan.page([tuple(range(8))] * 300, 0)
    second = plan.page([tuple(range(8))] * 300, 300)
    second.blocks[3].nulls = np.zeros(300, dtype=np.uint8)
    second.blocks[3].nulls[7] = 1
    refused_run(plan, [first, second])


@on_gpu
@pytest.mark.parametrize("label,long_one", [("VARCHAR3", b"abcd"), ("VARCHAR7", b"abcdefgh"), ("VARCHAR15", b"0123456789abcdef")])
@pytest.mark.parametrize("tier", ["lds", "gt"])
def test_a_string_beyond_its_bound_fails_the_page(gpu, monkeypatch, label, long_one, tier):
    """a producer that violates the declared VARCHAR(n): NOT_SUPPORTED (pa_short_bytes and the two-word packing raise -3), never a group
    with the string cut to its bound"""
    tier_env(monkeypatch, tier)
    shape = K.Shape("long", [K.Part(label, True)])
    plan = Plan(shape)
    keys = [(long_one[:-1],), (long_one,), (b"a",)] * 100
    refused_run(plan, [plan.page(keys, 0)], tier)
