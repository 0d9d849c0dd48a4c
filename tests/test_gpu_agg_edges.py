"""The accumulators of the fused aggregation at edge values, against the aggregate model (tests/agg_model.py) -- not the C oracle: every
compared row of agg_model.CASES goes through the device operators in every tier (each leg asserts the tier by the kernel's name), values
compared exactly, floats by bit pattern (a NaN as NaN), result types checked.

One JIT compilation costs far more than a launch, so one operator carries count(*) / count / sum / avg / min / max of every type of a
FAMILY over channels of their own ([key,] then a value and a mask channel per type; its kernel serves every page: plan cache).  The
value lists of CASES that share a type, values and mask are one GROUP: its rows hold the list in the channels of its type and benign
values in the others, so every aggregate of every type is compared for every group.  A list that makes an aggregate of the family raise
runs alone in an operator of its own (test_errors_*, test_divergence_*); its other aggregates are compared in the family's operator
without sums.

A group's rows are laid out so that the combination steps are crossed: LAYOUTS below.

DIVERGENCES (agg_model) lists the `either` rows and the deliberate differences from the reference; every tag is an entry of DESIGN.md
section 5 and every row asserts what the device does: the exact total or NUMERIC_VALUE_OUT_OF_RANGE, never a wrapped or truncated value.
"""
import collections
import functools
import os
import re
import struct

import numpy as np
import pytest

from presto_amd import abi
from presto_amd._lib import PrestoAmdError
from presto_amd.exchange import partial_layout
from presto_amd.expr import field
from presto_amd.operators import (Driver, FusedAggregationOperator, FusedJoinAggregationOperator, HashAggregationOperator, HashBuilderOperator,
                                  LookupSourceFactory, to_pages, upload_page)
from presto_amd.page import Block, Page
from tests import agg_model as M

on_gpu = pytest.mark.gpu
OUT_OF_RANGE = abi.ERR_NUMERIC_VALUE_OUT_OF_RANGE

TIERS = ["global", "lds", "ldsh", "ldsp", "gt", "probe"]
# the types of a family side by side in one operator; each fits the 16 accumulator words of the few-groups tier (count(*), count, the
# sum words -- one per 30-bit limb for a DECIMAL --, min, max per type), so no tier splits a family
FAMILIES = collections.OrderedDict([
    ("integers", [abi.BIGINT, abi.INTEGER, abi.DATE]),
    ("fp_bool", [abi.DOUBLE, abi.REAL, abi.BOOLEAN]),
    ("decimals_1_2", [M.D82, M.D122]),          # 1 and 2 limbs
    ("decimals_3_4", [M.D182, M.D274]),         # 3 and 4 limbs
    ("decimals_5", [M.D380, M.D3810]),          # 5 limbs
    ("varchar", [abi.VARCHAR]),                 # no declared bound: min / max go by the rank of the string
    ("varchar7", [abi.VARCHAR]),                # VARCHAR(7): min / max over the 7-byte image
])
TYPE_PARAMS = {"varchar7": [7]}                 # the type parameter of a family's types where it is not a DECIMAL's
D, B = abi.DOUBLE, abi.BOOLEAN
# the types of a family that run in a tier, where not all of them together: split where a tier refuses the whole for capacity
# (the partition-owned tables take a key and 15 words at most when they start from the planner's estimate), cut down to what the
# tier takes otherwise -- ELSEWHERE says what becomes of the rest
SPLIT = {
    ("integers", "ldsp"): [[abi.BIGINT, abi.INTEGER], [abi.DATE]],
    ("fp_bool", "probe"): [[D, B]],
    ("decimals_3_4", "ldsp"): [[M.D182]],
}
# (family, tier) -> the types that do not run in the tier, and what becomes of them: REFUSED (NOT_SUPPORTED when the first page arrives)
# or OTHER (computed, and computed right, by the kernel of another tier)
REFUSED, OTHER = "refused", "other"
ELSEWHERE = {
    ("fp_bool", "probe"): ([abi.REAL], REFUSED),           # the probe's lazily loaded channels: BIGINT, INTEGER, DATE, DOUBLE, BOOLEAN, VARCHAR(n <= 7)
    ("decimals_1_2", "probe"): ([M.D82, M.D122], REFUSED),
    ("decimals_3_4", "probe"): ([M.D182, M.D274], REFUSED),
    ("decimals_5", "probe"): ([M.D380, M.D3810], REFUSED),
    ("varchar", "probe"): ([abi.VARCHAR], OTHER),          # min / max by rank: the probe is not fused, the aggregation walks the HBM table
    ("varchar", "lds"): ([abi.VARCHAR], OTHER),
    ("varchar", "ldsh"): ([abi.VARCHAR], OTHER),
    ("varchar", "ldsp"): ([abi.VARCHAR], OTHER),
    ("decimals_3_4", "ldsp"): ([M.D274], OTHER),           # the partition-owned tables regroup 1-, 4- and 8-byte columns: others keep a position list
    ("decimals_5", "ldsp"): ([M.D380, M.D3810], OTHER),
    ("varchar7", "ldsp"): ([abi.VARCHAR], OTHER),
}


def parts(family, tier):
    if (family, tier) in SPLIT:
        return SPLIT[(family, tier)]
    return [] if (family, tier) in ELSEWHERE else [FAMILIES[family]]
BENIGN = {"BIGINT": 3, "INTEGER": -2, "DATE": 11, "DOUBLE": 1.5, "REAL": np.float32(-0.25), "BOOLEAN": True, "VARCHAR": b"ok"}
GROUP_KEY, FILLER_KEY = 1000, 10 ** 9

# name -> (order, rows between two rows of a group at least, rows per page; None: every round of rows is a page)
LAYOUTS = collections.OrderedDict([
    ("adjacent", ("group", 1, 255)),          # a group's rows next to each other: one lane's quad and its neighbours; pages below 256 rows take the row-by-row tail
    ("lanes", ("round", 5, 1027)),            # different lanes of a wave; a ragged end
    ("waves", ("round", 261, 1027)),          # different waves of a workgroup
    ("workgroups", ("round", 1031, 4099)),    # different workgroups (4 rows per lane, 256 lanes), a page of a little over 4096 rows
    ("pages", ("round", 523, None)),          # different pages
])


def benign(t):
    return 7 if M.is_decimal(t) else BENIGN[M.label(t)]


def slot_fns(t, sums=True):
    fns = ["count_star", "count"]
    if sums and (t in (abi.BIGINT, abi.INTEGER, abi.DOUBLE, abi.REAL) or M.is_decimal(t)):
        fns += ["sum", "avg"]
    elif t in (abi.BIGINT, abi.INTEGER):
        fns += ["avg"]                        # without sums: the DOUBLE average of an integer raises nothing
    if t != abi.LONG_DECIMAL:                 # (no order on the sign-magnitude words of a long decimal: min / max are refused)
        fns += ["min", "max"]
    return fns


# ---- groups: the value lists of CASES ----------------------------------------------------------------------------------------------------------
Group = collections.namedtuple("Group", "name type values masks cases")   # cases: {fn name: [CASES row names]}


def list_key(c):
    """(raw bit patterns: two NaNs are two values here)"""
    raw = lambda v: struct.pack("<d", float(v)) if M.is_fp(c.type) and v is not None else v
    return (M.label(c.type), tuple(raw(v) for v in c.values), None if c.mask is None else tuple(c.mask))


@functools.lru_cache(maxsize=None)
def groups():
    by_key = collections.OrderedDict()
    for c in M.CASES:
        k = list_key(c)
        if k not in by_key:
            masks = [True] * len(c.values) if c.mask is None else list(c.mask)
            by_key[k] = Group(c.name.split(":", 1)[1], c.type, list(c.values), masks, {})
        by_key[k].cases.setdefault(M.FN_NAMES[c.fn], []).append(c.name)
    return list(by_key.values())


def group_outcomes(g, fns):
    return {fn: M.aggregate(fn, g.type, g.values, g.masks) for fn in fns}


def quiet(g, sums):
    """every aggregate of the group's slot gives a value or NULL in every order of addition"""
    return all(r.outcome[0] in ("value", "null") for r in group_outcomes(g, slot_fns(g.type, sums)).values())


def family_of(t):
    return next(name for name, types in FAMILIES.items() if any(M.label(t) == M.label(u) for u in types))


def in_family(g, family):
    if family == "varchar7":
        return g.type == abi.VARCHAR and all(v is None or len(v) <= 7 for v in g.values)
    return family_of(g.type) == family


@functools.lru_cache(maxsize=None)
def family_groups(family, sums):
    """sums=True: the groups the family's operator with all aggregates takes; False: the groups that make one of its sums raise (or depend
    on the order), for the operator without sums"""
    mine = [g for g in groups() if in_family(g, family) and g.values]
    if sums:
        return [g for g in mine if quiet(g, True)]
    return [g for g in mine if not quiet(g, True) and quiet(g, False)]


def test_every_compared_case_runs_in_a_family_operator():
    """on the CPU: no row of CASES is dropped silently"""
    ran = set()
    for family in FAMILIES:
        for sums in (True, False):
            for g in family_groups(family, sums):
                ran |= {name for fn, names in g.cases.items() if fn in slot_fns(g.type, sums) for name in names}
    refused = {c.name for c in M.CASES if c.type == abi.LONG_DECIMAL and c.fn in (abi.AGG_MIN, abi.AGG_MAX)}
    alone = {c.name for c in M.CASES if M.case_result(c).outcome[0] in ("error", "either")}
    empty = {c.name for c in M.CASES if not c.values}
    missing = {c.name for c in M.CASES} - ran - refused - alone - empty
    assert not missing, sorted(missing)[:10]
    assert alone == {c.name for c in error_cases()} | {c.name for c in either_cases()}
    assert len(ran) > 1000 and len(empty) > 20
    for tag, names in M.DIVERGENCES.items():
        assert names, tag


# ---- operators ------------------------------------------------------------------------------------------------------------------------------
class Plan:
    """[key,] (value, mask) per type -> projections of every channel, the aggregates of every slot over them"""

    def __init__(self, types, sums=True, keyed=True, masked=True, params=None, only=None):
        """only: the aggregates kept besides the counts (all of them when None)"""
        self.types, self.sums, self.keyed, self.masked = list(types), sums, keyed, masked
        self.params = list(params) if params else [abi.type_param(t) for t in self.types]
        self.input_types = [abi.BIGINT] if keyed else []
        self.type_params = [0] if keyed else []
        self.slots = []                     # (value channel, mask channel or None)
        for t in self.types:
            self.slots.append((len(self.input_types), len(self.input_types) + 1 if masked else None))
            self.input_types += [t] + ([abi.BOOLEAN] if masked else [])
            self.type_params += [self.params[len(self.slots) - 1]] + ([0] if masked else [])
        self.projections = [field(i, t) for i, t in enumerate(self.input_types)]
        self.aggregates, self.columns = [], []      # columns: (slot, fn name) of every aggregate output
        for s, t in enumerate(self.types):
            v, m = self.slots[s]
            for fn in slot_fns(t, sums):
                if only is not None and fn not in ("count_star", "count") and fn not in only:
                    continue
                a = (M.FNS[fn], -1, None) if fn == "count_star" else (M.FNS[fn], v, t)
                self.aggregates.append(a + ((m,) if masked else ()))
                self.columns.append((s, fn))

    def operator(self, tier, step=abi.STEP_SINGLE, state_format=abi.STATES_FLAT):
        """-> (operator, the builder to close behind it or None)"""
        kw = dict(step=step, state_format=state_format, type_params=self.type_params)
        gb = [0] if self.keyed else []
        if tier == "global":
            assert not self.keyed
            return FusedAggregationOperator(self.input_types, None, self.projections, [], self.aggregates, **kw), None
        if tier in ("lds", "ldsh"):
            return FusedAggregationOperator(self.input_types, None, self.projections, gb, self.aggregates, **kw), None
        if tier in ("gt", "ldsp"):
            # "many groups" from the planner: the HBM table at once, with the partition-owned LDS tables in front of it unless switched off
            return FusedAggregationOperator(self.input_types, None, self.projections, gb, self.aggregates, expected_groups=(1 << 20) + 1, **kw), None
        assert tier == "probe" and step == abi.STEP_SINGLE
        bridge = LookupSourceFactory()
        builder = HashBuilderOperator(bridge, [abi.BIGINT, abi.BIGINT], [0], [1])
        joined = [p.type for p in self.projections] + [abi.BIGINT]
        op = FusedJoinAggregationOperator(bridge, self.input_types, None, self.projections, [0], list(range(len(self.projections))), joined, gb, self.aggregates,
                                          type_params=self.type_params)
        return op, (bridge, builder)

    def page(self, rows):
        """rows: (key, [(value, mask) per slot]); every channel with a valueIsNull array when masked (one layout signature), none otherwise"""
        blocks = [Block.bigint([r[0] for r in rows])] if self.keyed else []
        if self.keyed and self.masked:
            blocks[0].nulls = np.zeros(len(rows), dtype=np.uint8)
        for s, t in enumerate(self.types):
            blocks.append(M.block_of(t, [r[1][s][0] for r in rows], nullable=self.masked))
            if self.masked:
                blocks.append(M.block_of(abi.BOOLEAN, [r[1][s][1] for r in rows], nullable=True))
        return Page(blocks, len(rows))


def tier_env(monkeypatch, tier):
    if tier == "gt":
        monkeypatch.setenv("PRESTO_AMD_NO_PARTITIONED", "1")     # the HBM table's own kernel
    else:
        monkeypatch.delenv("PRESTO_AMD_NO_PARTITIONED", raising=False)


PREFIX = {"global": "pa_fused_global_", "lds": "pa_fused_lds_", "ldsh": "pa_fused_ldsh_", "ldsp": "pa_fused_ldsp_", "gt": "pa_fused_gt_",
          "probe": "pa_fused_probe_"}


def check_name(tier, name, *where):
    assert name.startswith(PREFIX[tier]), (tier, name) + where


# ---- pages ----------------------------------------------------------------------------------------------------------------------------------
def group_rows(plan, g, key):
    """the group's list in the channels of its type, benign values under a true mask in the others"""
    s = next(i for i, t in enumerate(plan.types) if M.label(t) == M.label(g.type))
    rows = []
    for v, m in zip(g.values, g.masks):
        cells = [(benign(t), True) for t in plan.types]
        cells[s] = (v, m)
        rows.append((key, cells))
    return rows


def filler_row(plan, key, live):
    """a row of another group; ungrouped there is no other group: the row is masked out of every aggregate (false, or a NULL mask)"""
    return (key, [(benign(t), True if live else (False if key % 2 else None)) for t in plan.types])


def lay_out(plan, batch, layout, many_fillers):
    """-> pages (lists of rows) that hold every group of the batch [(group, key)], filler rows around them"""
    order, gap, page_rows = LAYOUTS[layout]
    per_group = [group_rows(plan, g, key) for g, key in batch]
    fillers = iter(range(FILLER_KEY, FILLER_KEY + 10 ** 7))

    def filler():
        # grouped: one other group, or a group per row; ungrouped: dead rows (the key only alternates the two ways of masking a row out)
        key = next(fillers)
        return filler_row(plan, key if (many_fillers or not plan.keyed) else FILLER_KEY, plan.keyed)

    rounds = []
    if order == "group":
        rounds.append([r for rows in per_group for r in rows])
    else:
        for j in range(max(len(rows) for rows in per_group)):
            rnd = [rows[j] for rows in per_group if j < len(rows)]
            rnd += [filler() for _ in range(gap - len(rnd))]
            rounds.append(rnd)
    if many_fillers:
        rounds.append([filler() for _ in range(3001)])             # thousands of other groups next to them
    if page_rows is None:
        return rounds
    seq = [r for rnd in rounds for r in rnd]
    pages = [seq[i:i + page_rows] for i in range(0, len(seq), page_rows)]
    if plan.keyed and not many_fillers and all(len(p) < 256 for p in pages):
        # the row-by-row kernel of pages below 256 rows leaves no name behind: a last page of the other group names the tier
        pages.append([filler() for _ in range(300)])
    return pages


def expected_of(plan, g):
    """the model's outcome per output column for a group: its own slot from its list, the others from as many benign values"""
    out = []
    for s, fn in plan.columns:
        t = plan.types[s]
        own = M.label(t) == M.label(g.type)
        if own:
            r = M.aggregate(fn, g.type, g.values, g.masks)
        else:
            r = M.aggregate(fn, t, [benign(t)] * len(g.values))
            assert M.order_free(M.FNS[fn], t, [benign(t)] * len(g.values))       # benign values are always compared
        assert r.outcome[0] in ("value", "null"), (g.name, fn, r.outcome)
        if own and fn in ("sum", "avg") and not M.order_free(M.FNS[fn], g.type, M.counted(M.FNS[fn], g.values, g.masks)):
            out.append((int(r.type), ANY))      # the group's own list gives an answer that depends on the order of addition: not compared
            continue
        out.append((int(r.type), M.bits(r.type, r.outcome[1]) if r.outcome[0] == "value" else None))
    return out


ANY = object()


def run(plan, tier, pages, device_pages=False, keys=None):
    """-> (rows, block types, kernel name)"""
    op, join = plan.operator(tier)
    try:
        if join is not None:
            ks = np.asarray(sorted(keys), dtype=np.int64)
            Driver([Page([Block.bigint(ks), Block.bigint(ks * 10)], len(ks))], [join[1]]).run()
        host = [plan.page(rows) for rows in pages]
        out = to_pages(op, [upload_page(p) for p in host] if device_pages else host)
        return [r for p in out for r in p.to_rows()], [[b.type for b in p.blocks] for p in out], op.kernelName()
    finally:
        op.close()
        if join is not None:
            join[1].close()


def compare(plan, tier, batch, layout, device_pages=False, many_fillers=False, entered=True):
    pages = lay_out(plan, batch, layout, many_fillers)
    keys = {r[0] for rows in pages for r in rows}
    got, types, kernel = run(plan, tier, pages, device_pages, keys)
    if entered:
        check_name(tier, kernel, layout, len(batch))
    else:
        assert kernel.startswith("pa_fused_") and not kernel.startswith(PREFIX[tier]), (tier, kernel)
    lead = 1 if plan.keyed else 0
    by_key = {(r[0] if plan.keyed else batch[0][1]): r[lead:] for r in got}
    assert len(by_key) == len(got) == (len(keys) if plan.keyed else 1), (tier, layout, len(got), len(keys))
    wrong = []
    for g, key in batch:
        want = expected_of(plan, g)
        row = by_key[key]
        for i, ((s, fn), (rtype, bits)) in enumerate(zip(plan.columns, want)):
            have = M.bits(M.result_type(M.FNS[fn], plan.types[s]), row[i])
            if bits is not ANY and have != bits:
                wrong.append((g.name, M.label(plan.types[s]), fn, row[i], bits))
            for tt in types:
                assert tt[lead + i] == rtype, (fn, M.label(plan.types[s]), tt[lead + i], rtype)
    assert not wrong, (tier, layout, "device" if device_pages else "host", len(wrong), wrong[:6])


BATCH = {"global": 1, "lds": 6, "ldsh": 48, "ldsp": 10 ** 6, "gt": 10 ** 6, "probe": 10 ** 6}
TIER_LAYOUTS = {"global": ["adjacent", "workgroups", "pages"], "lds": ["adjacent", "lanes", "waves", "workgroups", "pages"],
                "ldsh": ["adjacent", "waves", "workgroups", "pages"], "ldsp": ["adjacent", "workgroups", "pages"],
                "gt": ["adjacent", "lanes", "workgroups", "pages"], "probe": ["adjacent", "workgroups", "pages"]}


def batches(gs, tier):
    """batches of about BATCH[tier] groups, all of one size (a last batch of a few groups would stay in a tier below)"""
    keyed = [(g, GROUP_KEY + 7 * i) for i, g in enumerate(gs)]
    count = max(1, -(-len(keyed) // BATCH[tier]))
    size = -(-len(keyed) // count)
    return [keyed[i:i + size] for i in range(0, len(keyed), size)]


def compare_family(family, tier, sums, types):
    gs = [g for g in family_groups(family, sums) if any(M.label(g.type) == M.label(t) for t in types)]
    if not gs:
        return 0
    plan = Plan(types, sums=sums, keyed=tier != "global", params=TYPE_PARAMS.get(family))
    many = tier in ("ldsp", "gt", "probe")
    for n, batch in enumerate(batches(gs, tier)):
        for k, layout in enumerate(TIER_LAYOUTS[tier]):
            if tier in ("global", "lds") and (n + k) % 2 and layout not in ("adjacent", "pages"):
                continue                    # (small batches: every second one takes the layouts in between)
            compare(plan, tier, batch, layout, device_pages=False, many_fillers=many)
        compare(plan, tier, batch, "workgroups" if n % 2 else "adjacent", device_pages=True, many_fillers=many)
    return len(gs)


@on_gpu
@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("family", list(FAMILIES))
def test_values(gpu, monkeypatch, family, tier):
    tier_env(monkeypatch, tier)
    for types in parts(family, tier):
        assert compare_family(family, tier, True, types) > 0
        compare_family(family, tier, False, types)
    if (family, tier) in ELSEWHERE:
        rest, what = ELSEWHERE[(family, tier)]
        plan = Plan(rest, keyed=True, params=TYPE_PARAMS.get(family))
        gs = [g for g in family_groups(family, True) if any(M.label(g.type) == M.label(t) for t in rest)]
        batch = batches(gs, "ldsh")[0]
        if what == OTHER:
            compare(plan, tier, batch, "adjacent", many_fillers=tier in ("ldsp", "probe"), entered=False)
        else:
            with pytest.raises(PrestoAmdError) as e:
                compare(plan, tier, batch, "adjacent", many_fillers=True, entered=False)
            assert e.value.status == abi.ERR_NOT_SUPPORTED, e.value


# ---- without any null arrays: no mask, no valueIsNull -- grouped, the count word is implicit (cw == -1) ------------------------------------------
@on_gpu
@pytest.mark.parametrize("family,tier", [(f, t) for f in FAMILIES for t in ("lds", "gt") if parts(f, t)])
def test_values_without_null_arrays(gpu, monkeypatch, family, tier):
    tier_env(monkeypatch, tier)
    gs = [g for g in family_groups(family, True) if all(m is True for m in g.masks) and None not in g.values]
    assert gs
    plan = Plan(FAMILIES[family], keyed=True, masked=False, params=TYPE_PARAMS.get(family))
    for batch in batches(gs, tier):
        compare(plan, tier, batch, "adjacent", many_fillers=tier == "gt")
        compare(plan, tier, batch, "workgroups", device_pages=True, many_fillers=tier == "gt")


# ---- PARTIAL per page -> FINAL -------------------------------------------------------------------------------------------------------------------
def final_plan(plan):
    key_types = [abi.BIGINT] if plan.keyed else []
    ptypes, faggs = partial_layout(key_types, plan.aggregates)
    return ptypes, faggs


def run_partial_final(plan, tier, pages, state_format=abi.STATES_FLAT):
    """every page through a PARTIAL operator of its own, the states through one FINAL operator -> (rows, partial pages, kernel names)"""
    parts, names = [], set()
    for rows in pages:
        if state_format == abi.STATES_FLAT:
            op, _ = plan.operator(tier, step=abi.STEP_PARTIAL)
        else:       # the reference's form is made by the plain operator (the same kernels behind identity projections)
            op = HashAggregationOperator(plan.input_types, [0], plan.aggregates, step=abi.STEP_PARTIAL, state_format=state_format, type_params=plan.type_params)
        try:
            parts += to_pages(op, [plan.page(rows)])
            names.add(op.kernelName())
        finally:
            op.close()
    if state_format != abi.STATES_FLAT:
        return None, parts, names
    ptypes, faggs = final_plan(plan)
    for p in parts:
        assert [b.type for b in p.blocks] == [int(t) for t in ptypes]
    kw = dict(expected_groups=(1 << 20) + 1) if tier == "gt" else {}
    bound = next((p for t, p in zip(plan.types, plan.params) if t == abi.VARCHAR), 0)
    kw["type_params"] = [bound if t == abi.VARCHAR else abi.type_param(t) for t in ptypes]
    fin = FusedAggregationOperator(ptypes, None, [field(i, t) for i, t in enumerate(ptypes)], [0] if plan.keyed else [], faggs, step=abi.STEP_FINAL, **kw)
    try:
        out = to_pages(fin, final_input(plan, ptypes, parts))
        check_name(final_tier(plan, tier), fin.kernelName(), "FINAL")
        return [r for p in out for r in p.to_rows()], parts, names
    finally:
        fin.close()


def final_input(plan, ptypes, parts):
    """ungrouped: the state pages as they are (one row each).  Grouped: all states in one page of 256 rows or more, so that the FINAL step
    combines them in the tier's own kernel and not in the row-by-row kernel of short pages alone -- where the groups are few, the other
    group's states are repeated (only that group's result changes, and it is not compared)"""
    if not plan.keyed:
        return parts
    rows = [r for p in parts for r in p.to_rows()]
    other = [r for r in rows if r[0] >= FILLER_KEY]
    while len(rows) < 300:
        rows += other
    return [Page([M.block_of(t, [r[i] for r in rows], nullable=True) for i, t in enumerate(ptypes)], len(rows))]


def final_tier(plan, tier):
    """the FINAL step keeps a count word and the value words per aggregate (5 limbs for a DECIMAL(38, s) state): a family of more than 16
    such words is past the few-groups tier's capacity and starts on the LDS table"""
    if tier != "lds":
        return tier
    words = 0
    for s, fn in plan.columns:
        words += 1 if fn in ("count", "count_star") else (2 if fn in ("min", "max") or not M.is_decimal(plan.types[s]) else 6)
    return "lds" if words <= 16 else "ldsh"


@on_gpu
@pytest.mark.parametrize("family,tier", [(f, t) for f in FAMILIES for t in ("global", "lds", "gt") if parts(f, t)])
def test_partial_final(gpu, monkeypatch, family, tier):
    """the combine path with edge-valued states (limb states re-cut from DECIMAL(38, s) values among them): a group's rows in different
    pages, every page a PARTIAL step, one FINAL step over the flat states"""
    tier_env(monkeypatch, tier)
    plan = Plan(FAMILIES[family], keyed=tier != "global", params=TYPE_PARAMS.get(family))
    lead = 1 if plan.keyed else 0
    for batch in batches(family_groups(family, True), tier):
        pages = lay_out(plan, batch, "pages", tier == "gt")
        got, _, names = run_partial_final(plan, tier, pages)
        for name in names:
            check_name(tier, name)
        by_key = {(r[0] if plan.keyed else batch[0][1]): r[lead:] for r in got}
        wrong = []
        for g, key in batch:
            for i, ((s, fn), (rtype, bits)) in enumerate(zip(plan.columns, expected_of(plan, g))):
                t = plan.types[s]
                rt = abi.BIGINT if (fn == "sum" and t == abi.INTEGER) else M.result_type(M.FNS[fn], t)   # the FINAL sum of BIGINT states is a BIGINT
                if bits is not ANY and M.bits(rt, by_key[key][i]) != bits:
                    wrong.append((g.name, M.label(t), fn, by_key[key][i], bits))
        assert not wrong, (tier, len(wrong), wrong[:6])


@on_gpu
@pytest.mark.parametrize("family", ["integers", "fp_bool"])
def test_partial_states_in_the_reference_form(gpu, family):
    """STATES_REFERENCE: the intermediate row against the model's (count, value): sum -> ROW(count, false-null flags kept true, value,
    true), avg -> ROW(double sum, count), min / max -> the value (a long for INTEGER / DATE), NULL while none was seen.  The integer,
    DOUBLE and BOOLEAN states only: the operator refuses the form for REAL, and the model does not state the reference's serialized form
    of the DECIMAL states (a VARBINARY of the sum and its overflow counter), so the decimal families are not run in it."""
    types = [t for t in FAMILIES[family] if t != abi.REAL]      # (reference-format states over REAL are refused: not on the device path)
    plan = Plan(types, keyed=True)
    gs = [g for g in family_groups(family, True) if g.type != abi.REAL]
    for batch in batches(gs, "lds"):
        pages = lay_out(plan, batch, "adjacent", False)
        _, parts, names = run_partial_final(plan, "lds", [[r for rows in pages for r in rows]], abi.STATES_REFERENCE)
        for name in names:
            assert name == "" or name.startswith("pa_fused_"), name     # (the plain operator in front of the kernels: the values are what is pinned here)
        by_key = {r[0]: r[1:] for p in parts for r in p.to_rows()}
        for g, key in batch:
            for i, (s, fn) in enumerate(plan.columns):
                t = plan.types[s]
                own = M.label(t) == M.label(g.type)
                r = M.aggregate(fn, t, g.values if own else [benign(t)] * len(g.values), g.masks if own else None)
                inter, have = r.intermediate, by_key[key][i]
                if fn in ("sum", "avg") and own and not M.order_free(M.FNS[fn], t, M.counted(M.FNS[fn], g.values, g.masks)):
                    continue
                if fn in ("count", "count_star"):
                    assert have == inter[0], (g.name, fn, have, inter)
                elif fn == "sum":
                    st = abi.DOUBLE if M.is_fp(t) else abi.BIGINT
                    assert (have[0], have[1], M.bits(st, have[2]), have[3]) == (inter[0], True, M.bits(st, inter[1]), True), (g.name, M.label(t), have, inter)
                elif fn == "avg":
                    assert (M.bits(abi.DOUBLE, have[0]), have[1]) == (M.bits(abi.DOUBLE, inter[1]), inter[0]), (g.name, M.label(t), have, inter)
                else:
                    assert M.bits(t, have) == M.bits(t, inter[1]), (g.name, M.label(t), fn, have, inter)


# ---- no rows at all ---------------------------------------------------------------------------------------------------------------------------------
@on_gpu
@pytest.mark.parametrize("family", list(FAMILIES))
def test_no_rows(gpu, family):
    """ungrouped: one row with count 0 and NULLs; grouped: no rows"""
    plan = Plan(FAMILIES[family], keyed=False)
    op, _ = plan.operator("global")
    try:
        rows = [r for p in to_pages(op, []) for r in p.to_rows()]
    finally:
        op.close()
    want = tuple(0 if fn in ("count", "count_star") else None for _, fn in plan.columns)
    assert rows == [want]
    for s, fn in plan.columns:
        assert M.aggregate(fn, plan.types[s], []).outcome == (("value", 0) if fn in ("count", "count_star") else ("null",))
    plan = Plan(FAMILIES[family], keyed=True)
    op, _ = plan.operator("lds")
    try:
        assert [r for p in to_pages(op, []) for r in p.to_rows()] == []
    finally:
        op.close()


# ---- errors: each order-free "error" row alone in an operator of its own, among benign groups ----------------------------------------------------------
def error_cases():
    return [c for c in M.CASES if M.case_result(c).outcome[0] == "error"]


def either_cases():
    return [c for c in M.CASES if M.case_result(c).outcome[0] == "either"]


def group_of_case(c):
    masks = [True] * len(c.values) if c.mask is None else list(c.mask)
    return Group(c.name, c.type, list(c.values), masks, {M.FN_NAMES[c.fn]: [c.name]})


def twin_of(g):
    """the same values short of the bound: the last counted value one nearer to zero"""
    at = max(i for i, (v, m) in enumerate(zip(g.values, g.masks)) if m is True and v is not None)
    values = list(g.values)
    values[at] += -1 if sum(M.counted(abi.AGG_SUM, g.values, g.masks)) > 0 else 1
    return Group(g.name + "/twin", g.type, values, g.masks, {})


def benign_neighbours(family, tier):
    """few enough for the few-groups tier, too many for it elsewhere"""
    return [g for g in family_groups(family, True) if len(g.values) >= 2][:5 if tier == "lds" else 24]


def plan_for(t, tier, only=None):
    """-> (the plan of the part of t's family that runs in the tier, True) or (the plan of what does not, False)"""
    family = family_of(t)
    for types in parts(family, tier):
        if any(M.label(t) == M.label(u) for u in types):
            return Plan(types, keyed=tier != "global", only=only), True
    return Plan(ELSEWHERE[(family, tier)][0], keyed=True, only=only), False


def outcome_alone(plan, tier, g, layout):
    """the group among benign ones in a fresh operator -> ('error', status) | ('value', the row of its key), and the kernel's name"""
    near = [n for n in benign_neighbours(family_of(g.type), tier) if any(M.label(n.type) == M.label(t) for t in plan.types)]
    batch = [(n, GROUP_KEY + 7 * (i + 1)) for i, n in enumerate(near)] if plan.keyed else []
    batch.insert(min(2, len(batch)), (g, GROUP_KEY))
    pages = lay_out(plan, batch, layout, tier in ("ldsp", "gt", "probe"))
    keys = {r[0] for rows in pages for r in rows}
    try:
        got, _, kernel = run(plan, tier, pages, keys=keys)
    except PrestoAmdError as e:
        return ("error", e.status), None
    lead = 1 if plan.keyed else 0
    return ("value", next(r[lead:] for r in got if not plan.keyed or r[0] == GROUP_KEY)), kernel


ERROR_CASES = error_cases()


@on_gpu
@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("name", [c.name for c in ERROR_CASES])
def test_errors(gpu, monkeypatch, name, tier):
    tier_env(monkeypatch, tier)
    c = M.CASE[name]
    g = group_of_case(c)
    plan, entered = plan_for(c.type, tier)
    col = plan.columns.index((next(i for i, t in enumerate(plan.types) if M.label(t) == M.label(c.type)), M.FN_NAMES[c.fn]))
    twin = twin_of(g)
    want = M.aggregate(c.fn, twin.type, twin.values, twin.masks)
    assert want.outcome[0] == "value" and M.case_result(c).outcome == ("error", OUT_OF_RANGE)
    for layout in ("adjacent", "workgroups"):
        got, _ = outcome_alone(plan, tier, g, layout)
        if not entered and got == ("error", abi.ERR_NOT_SUPPORTED):
            continue                        # the tier refuses the type (test_values says which)
        assert got == ("error", OUT_OF_RANGE), (name, tier, layout, got)
        # the benign twin in the same layout does not raise, and gives the total
        got, kernel = outcome_alone(plan, tier, twin, layout)
        assert got[0] == "value", (name, tier, layout, got)
        if entered:
            check_name(tier, kernel, layout)
        assert M.bits(want.type, got[1][col]) == M.bits(want.type, want.outcome[1]), (name, tier, layout, got[1][col], want.outcome)


# ---- documented divergences ---------------------------------------------------------------------------------------------------------------------
def design_divergence_tags():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "DESIGN.md")).read()
    section = text[text.index("## 5. Parity"):text.index("## 6. Measurement")]
    return set(re.findall(r"`(agg-[a-z-]+)`", section))


def test_design_lists_exactly_the_divergences_of_the_table():
    assert design_divergence_tags() == set(M.DIVERGENCES)


def test_divergences_differ_from_the_reference_as_stated():
    for name in M.DIVERGENCES["agg-bigint-sum-order"] + M.DIVERGENCES["agg-decimal-sum-order"]:
        c = M.CASE[name]
        r = M.case_result(c)
        assert r.outcome[0] == "either" and r.outcome[2] == OUT_OF_RANGE, name
        if ":back" in name:     # the running sum overflows and comes back: refused by the reference, the exact total fits
            assert r.row_order == ("error", OUT_OF_RANGE) and r.outcome[1] == sum(M.counted(c.fn, c.values, c.mask)), name
    for name in M.DIVERGENCES["agg-integer-sum-column"]:
        c = M.CASE[name]
        total = sum(M.counted(c.fn, c.values, c.mask))
        assert M.aggregate("sum", abi.BIGINT, c.values, c.mask).outcome == ("value", total)      # the reference: sum(CAST(x AS BIGINT))
        assert M.case_result(c).outcome == ("error", OUT_OF_RANGE) and not M.I32_MIN <= total <= M.I32_MAX


EITHER_CASES = either_cases()


@on_gpu
@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("name", [c.name for c in EITHER_CASES])
def test_divergence_is_the_exact_total_or_out_of_range(gpu, monkeypatch, name, tier):
    """an `either` row: the device returns the exact total (average) or raises NUMERIC_VALUE_OUT_OF_RANGE, never a wrapped or truncated
    value; a DECIMAL one in a SINGLE step is always exact (the limb sums are)"""
    tier_env(monkeypatch, tier)
    c = M.CASE[name]
    assert any(name in rows for rows in M.DIVERGENCES.values())
    r = M.case_result(c)
    g = group_of_case(c)
    # (an average next to the sum of the same values would share the sum's fate: the row's own aggregate and the counts only)
    plan, entered = plan_for(c.type, tier, only=[M.FN_NAMES[c.fn]])
    col = plan.columns.index((next(i for i, t in enumerate(plan.types) if M.label(t) == M.label(c.type)), M.FN_NAMES[c.fn]))
    for layout in ("adjacent", "workgroups", "pages"):
        got, _ = outcome_alone(plan, tier, g, layout)
        if not entered and got == ("error", abi.ERR_NOT_SUPPORTED):
            continue
        if got[0] == "error":
            assert got[1] == OUT_OF_RANGE and not M.is_decimal(c.type), (name, tier, layout, got)
        else:
            assert got[1][col] == r.outcome[1], (name, tier, layout, got[1][col], r.outcome)


@on_gpu
@pytest.mark.parametrize("name", [c.name for c in EITHER_CASES if M.is_decimal(c.type)])
def test_divergence_partial_states_hold_the_exact_total_or_refuse(gpu, name):
    """PARTIAL of all rows in one page: the flat state is a DECIMAL(38, s), which holds the exact total or nothing"""
    c = M.CASE[name]
    g = group_of_case(c)
    plan = Plan(FAMILIES[family_of(c.type)], keyed=True, only=[M.FN_NAMES[c.fn]])
    pages = lay_out(plan, [(g, GROUP_KEY)], "adjacent", False)
    assert len(pages[0]) == len(g.values)          # every row of the group in the first page
    r = M.case_result(c)
    col = plan.columns.index((next(i for i, t in enumerate(plan.types) if M.label(t) == M.label(c.type)), M.FN_NAMES[c.fn]))
    try:
        got, _, _ = run_partial_final(plan, "lds", pages)
    except PrestoAmdError as e:
        assert e.status == OUT_OF_RANGE and r.intermediate == ("error", OUT_OF_RANGE), (name, e.status, r.intermediate)
        return
    assert r.intermediate[0] != "error", (name, r.intermediate)
    row = next(x for x in got if x[0] == GROUP_KEY)
    assert row[1 + col] == r.outcome[1], (name, row[1 + col], r.outcome)
