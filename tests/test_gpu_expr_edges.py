"""The row function csrc/exprgen.cpp generates, at edge values, against the expression model (tests/expr_model.py) -- not the C oracle:

  a. every cell of expr_model.CELLS through FilterAndProject: compared bit for bit (value pages at two lengths, host and device pages;
     every raising row alone in a page, at three positions, with exactly the model's status) or REFUSED when the operator is created;
  b. laziness and NULL logic: fixed expressions with the rows of their truth tables;
  c. the same row function inside the fused kernels: ungrouped plain and staged, few-groups, HBM table, fused join probe -- each leg
     asserts the tier by the kernel's name.

One JIT compilation costs far more than a launch, so operands come from columns and a kernel serves every page of its cell (plan
cache); the fused legs bundle the six operators of a type, and the expressions of (b), into one kernel per tier: every item of a
bundle reads channels of its own, the other items' channels hold benign operands.

DIVERGENCES lists what the device deliberately computes differently from the reference; every row names its entry in DESIGN.md
section 5 and asserts the device's actual behaviour.
"""
import collections
import functools
import os
import re

import numpy as np
import pytest

from presto_amd import abi
from presto_amd._lib import PrestoAmdError
from presto_amd.expr import and_, call, coalesce, constant, field, if_, or_
from presto_amd.operators import (Driver, FilterAndProjectOperator, FusedAggregationOperator, FusedJoinAggregationOperator, HashBuilderOperator,
                                  LookupSourceFactory, to_pages, upload_page)
from presto_amd.page import Block, Page
from tests import expr_model as M

on_gpu = pytest.mark.gpu
PAGE = 1027                      # whole quads plus a ragged end
POSITIONS = (0, 514, PAGE - 1)   # first row, inside a quad, last row

# ---- classification -------------------------------------------------------------------------------------------------------------------------
# Cells the device generator rejects (PA_ERR_NOT_SUPPORTED when the operator is created).  Every other cell is compared.
REFUSED = {c.name for c in M.CELLS if not c.modelled} | {
    "cast:BIGINT->INTEGER",                      # the reference has it (toIntExact); not on the device path
    "cast:VARCHAR->VARCHAR", "if:VARCHAR", "coalesce:VARCHAR",   # a VARCHAR projection is a plain input reference
}
COMPARED = [c for c in M.CELLS if c.name not in REFUSED]
RAISING = [c for c in COMPARED if c.raises]


def test_every_cell_is_classified():
    names = {c.name for c in M.CELLS}
    assert REFUSED <= names, REFUSED - names
    for c in M.CELLS:
        assert c.modelled or c.name in REFUSED, c.name       # nothing the model does not state is ever compared
    assert {c.name for c in COMPARED} | REFUSED == names and not {c.name for c in COMPARED} & REFUSED
    # what the project requires to be compared: all arithmetic, comparisons and forms of the types with operators on the device path
    for name in ("BIGINT", "INTEGER", "DATE", "DOUBLE", "REAL"):
        for label, _ in M.ARITH_OPS:
            assert "%s:%s" % (label, name) not in REFUSED
    for name in M.ALL_TYPES:
        for label, _ in M.COMPARE_OPS:
            assert "%s:%s" % (label, name) not in REFUSED
        for form in ("is_null", "between", "in"):
            assert "%s:%s" % (form, name) not in REFUSED
    for label in ("add", "subtract", "multiply", "negate"):
        assert "%s:DECIMAL" % label not in REFUSED


# ---- helpers --------------------------------------------------------------------------------------------------------------------------------
def rows_of(op, pages):
    try:
        return [r for p in to_pages(op, pages) for r in p.to_rows()]
    finally:
        op.close()


def status_of(make_op, pages):
    op = make_op()
    try:
        with pytest.raises(PrestoAmdError) as e:
            to_pages(op, pages)
        return e.value.status
    finally:
        op.close()


def tile(rows, n=PAGE):
    return [rows[k % len(rows)] for k in range(n)]


def value_pages(rows):
    """the rows as they are, in pages of fewer than 256 rows (the row-by-row tail path), and in pages of 1027 rows, the last one tiled"""
    out = [rows[i:i + 255] for i in range(0, len(rows), 255)]
    for i in range(0, len(rows), PAGE):
        out.append(tile(rows[i:i + PAGE]))
    return out


def page_of(columns, rows):
    """every channel with a valueIsNull array: one column-layout signature, so one kernel, for all pages of a bundle"""
    return M.page_of(columns, rows, nullable=True)


# ---- bundles: several expressions in one kernel, each over channels of its own -----------------------------------------------------------------
Item = collections.namedtuple("Item", "name columns expr rows")   # expr over channels 0 .. len(columns) - 1; rows: operand tuples of the item


class Bundle:
    """columns: the items' channels side by side, each item's expression moved to its own (expr_model.rebase).  embed(k, r) is the bundle
    row that holds r in item k's channels and a benign (non-raising, NULL-free where there is one) row of every other item in theirs."""

    def __init__(self, name, items, row_filter=None):
        self.name = name
        self.items = list(items)
        self.columns = []
        self.projections = []
        self.offsets = []
        benign = []
        for it in self.items:
            self.offsets.append(len(self.columns))
            self.projections.append(M.rebase(it.expr, len(self.columns)))
            self.columns += list(it.columns)
            ok = [tuple(r) for r in it.rows if M.outcome(it.expr, r)[0] == "value"]
            benign.append(next((r for r in ok if None not in r), ok[0]))
        self.filter = row_filter(*[field(i, M.TYPES[n]) for i, n in enumerate(self.columns)]) if row_filter else None
        self.benign = tuple(v for r in benign for v in r)

    def embed(self, k, r):
        at = self.offsets[k]
        return self.benign[:at] + tuple(r) + self.benign[at + len(r):]

    def outcome(self, row):
        """('value', selected, outputs) | ('error', status): the filter first, then the projections in turn (expr_model.page)"""
        try:
            if self.filter is not None and M.evaluate(self.filter, row) is not True:
                return "value", False, None
            return "value", True, tuple(M.write(p.type, M.evaluate(p, row)) for p in self.projections)
        except M.ModelError as err:
            return "error", err.status

    @functools.lru_cache(maxsize=None)
    def split(self):
        """every row of every item, embedded: (rows with their outcome that give values, rows that raise)"""
        values, errors = [], []
        for k, it in enumerate(self.items):
            for r in it.rows:
                row = self.embed(k, r)
                o = self.outcome(row)
                (values if o[0] == "value" else errors).append((row, o))
        return values, errors

    def types(self):
        return M.input_types(self.columns)

    def out_types(self):
        return [p.type for p in self.projections]

    def operator(self):
        return FilterAndProjectOperator(self.types(), self.filter, self.projections)

    def parts(self, tier):
        """the few-groups kernel keeps at most 16 accumulator words per group in LDS (count(*), and count / min / max per projection):
        a bundle of more than 5 projections goes there as two kernels"""
        if tier != "few_groups" or len(self.items) <= 5:
            return [self]
        half = (len(self.items) + 1) // 2
        return [Bundle(self.name + "/1", self.items[:half]), Bundle(self.name + "/2", self.items[half:])]


def compared_cells(group):
    return [c for c in M.GROUPS[group] if c.name not in REFUSED]


@functools.lru_cache(maxsize=None)
def group_bundle(group):
    """the compared cells of a group in one operator: one kernel serves every page of every cell of the group"""
    return Bundle(group, [Item(c.name, c.columns, c.expr, M.cell_rows(c)) for c in compared_cells(group)])


# ---- a. FilterAndProject, every cell ----------------------------------------------------------------------------------------------------------
@on_gpu
@pytest.mark.parametrize("cell", COMPARED, ids=[c.name for c in COMPARED])
def test_filter_project_values(gpu, cell):
    b = group_bundle(cell.group)
    k = [it.name for it in b.items].index(cell.name)
    values, _ = M.split_rows(cell)
    assert values
    for part in value_pages(values):
        want = [M.bits(cell.out_type, v) for _, v in part]
        host = page_of(b.columns, [b.embed(k, r) for r, _ in part])
        for page in (host, upload_page(host)):
            got = [M.bits(cell.out_type, r[k]) for r in rows_of(b.operator(), [page])]
            wrong = [(r, g, w) for (r, _), g, w in zip(part, got, want) if g != w]
            assert len(got) == len(want) and not wrong, (cell.name, len(part), page.mem, len(wrong), wrong[:5])
    # channels without a valueIsNull array are another column-layout signature, so another kernel (no NULL guards): the NULL-free rows
    part = tile([(r, v) for r, v in values if None not in r])
    got = [M.bits(cell.out_type, r[k]) for r in rows_of(b.operator(), [M.page_of(b.columns, [b.embed(k, r) for r, _ in part])])]
    wrong = [(r, g, M.bits(cell.out_type, v)) for (r, v), g in zip(part, got) if g != M.bits(cell.out_type, v)]
    assert len(got) == len(part) and not wrong, (cell.name, "no NULL arrays", len(wrong), wrong[:5])


@on_gpu
@pytest.mark.parametrize("cell", RAISING, ids=[c.name for c in RAISING])
def test_filter_project_errors(gpu, cell):
    b = group_bundle(cell.group)
    k = [it.name for it in b.items].index(cell.name)
    values, errors = M.split_rows(cell)
    assert errors
    base = tile([b.embed(k, r) for r, _ in values])
    for r, status in errors:
        for pos in POSITIONS:
            rows = list(base)
            rows[pos] = b.embed(k, r)
            got = status_of(b.operator, [page_of(b.columns, rows)])
            assert got == status, (cell.name, r, pos, got, status)


@on_gpu
@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refused_at_creation(gpu, name):
    cell = M.CELL[name]
    with pytest.raises(PrestoAmdError) as e:
        FilterAndProjectOperator(M.input_types(cell.columns), None, [cell.expr])
    assert e.value.status == abi.ERR_NOT_SUPPORTED, e.value


def _div(a, b):
    return (a / b) > constant(0, abi.BIGINT)


TF = [True, False, None]
DIVS = [(6, 2), (-6, 2), (6, 0), (None, 0), (6, None), (M.I64_MIN, -1)]     # true, false, DIVISION_BY_ZERO, NULL, NULL, OUT_OF_RANGE
PAB = [(p, a, b) for p in TF for a, b in DIVS]
NAN = float("nan")


def item(name, columns, build, rows):
    return Item(name, columns, build(*[field(i, M.TYPES[n]) for i, n in enumerate(columns)]), [tuple(r) for r in rows])


def laziness_bundles():
    B, I, D, BOOL = "BIGINT", "INTEGER", "DOUBLE", "BOOLEAN"
    first = [
        # a deciding left operand hides the right one's error; a NULL left operand does not (AndCodeGenerator / OrCodeGenerator)
        item("and_raising_right", [BOOL, B, B], lambda p, a, b: and_(p, _div(a, b)), PAB),
        item("or_raising_right", [BOOL, B, B], lambda p, a, b: or_(p, _div(a, b)), PAB),
        item("and_raising_left", [BOOL, B, B], lambda p, a, b: and_(_div(a, b), p), PAB),
        # the untaken branch is not evaluated; a NULL condition takes the else branch (IfCodeGenerator)
        item("if_raising_then", [BOOL, B, B], lambda p, a, b: if_(p, a / b, a), PAB),
        item("if_raising_else", [BOOL, B, B], lambda p, a, b: if_(p, a, a / b), PAB),
        # arguments after the first non-NULL one are not evaluated (CoalesceCodeGenerator)
        item("coalesce_raising_later", [B, B, B], lambda c, a, b: coalesce(c, a / b), [(c, a, b) for c in (5, None) for a, b in DIVS]),
    ]
    xs = [0, 5, 10, None]
    second = [
        item("coalesce_raising_first", [B, B, B], lambda c, a, b: coalesce(a / b, c), [(c, a, b) for c in (5, None) for a, b in DIVS]),
        # a NULL bound against a FALSE other half is FALSE, against a TRUE one NULL (BetweenCodeGenerator: AND of the two halves)
        item("between_null_bounds", [B, B, B], lambda x, lo, hi: x.between(lo, hi), [(x, lo, hi) for x in xs for lo in (3, None) for hi in (7, None)]),
        # a NULL in the list: a match is TRUE, a miss NULL (InCodeGenerator)
        item("in_null_in_list", [B, B], lambda x, y: x.isin(y, constant(None, abi.BIGINT), constant(3, abi.BIGINT)),
             [(x, y) for x in (3, 4, 5, None) for y in (5, None)]),
        # NaN equals nothing, not even a NaN in the list; -0.0 equals 0.0
        item("in_nan_and_zeros", [D, D], lambda x, y: x.isin(y, constant(0.0, abi.DOUBLE), constant(NAN, abi.DOUBLE)),
             [(x, y) for x in (NAN, 0.0, -0.0, 1.5, None) for y in (NAN, -0.0, 1.5, None)]),
        item("between_nan_and_zeros", [D, D, D], lambda x, lo, hi: x.between(lo, hi),
             [(x, lo, hi) for x in (NAN, 0.0, -0.0, 1.5) for lo in (NAN, -0.0, 0.0, None) for hi in (NAN, 0.0, 2.0, None)]),
        # INTEGER MIN / -1 does not raise and is written as MIN (IntegerOperators.java:81-89); MIN % -1 is 0
        item("integer_min_by_minus_one", [I, I], lambda a, b: a / b, [(M.I32_MIN, -1), (M.I32_MIN, 1), (M.I32_MAX, -1), (7, 0), (None, -1), (-7, 2)]),
    ]
    return [Bundle("laziness_1", first), Bundle("laziness_2", second)]


def rejecting_filter_bundle():
    """the filter rejects exactly the rows on which the projection would raise: nothing is raised (PageProcessor projects selected rows)"""
    rows = [(6, 2), (6, 0), (None, 0), (7, None), (M.I64_MIN, -1), (M.I64_MIN, 1), (-9, 4)]
    zero, minus_one = constant(0, abi.BIGINT), constant(-1, abi.BIGINT)
    return Bundle("rejecting_filter", [item("divide_where_defined", ["BIGINT", "BIGINT"], lambda a, b: a / b, rows)],
                  row_filter=lambda a, b: and_(b.ne(zero), b.ne(minus_one)))


@functools.lru_cache(maxsize=None)
def bundles():
    out = {b.name: b for b in laziness_bundles() + [rejecting_filter_bundle()] + [group_bundle("arith:" + n) for n in ("BIGINT", "INTEGER", "DATE")]}
    return out


LAZINESS = ["laziness_1", "laziness_2", "rejecting_filter"]
ARITH = ["arith:BIGINT", "arith:INTEGER", "arith:DATE"]


def test_bundles_hold_what_they_are_for():
    """on the model alone: every laziness item has rows where the raising operand is hidden, and rows where it raises"""
    for name in ("laziness_1", "laziness_2"):
        b = bundles()[name]
        values, errors = b.split()
        assert values and errors
        statuses = {o[1] for _, o in errors}
        assert abi.ERR_DIVISION_BY_ZERO in statuses
    b1 = bundles()["laziness_1"]
    assert {o[1] for _, o in b1.split()[1]} == {abi.ERR_DIVISION_BY_ZERO, abi.ERR_NUMERIC_VALUE_OUT_OF_RANGE}
    # a NULL left operand does not hide the error; FALSE (AND) and TRUE (OR) do
    p, a, b = field(0, abi.BOOLEAN), field(1, abi.BIGINT), field(2, abi.BIGINT)
    assert M.outcome(and_(p, _div(a, b)), (None, 6, 0)) == ("error", abi.ERR_DIVISION_BY_ZERO)
    assert M.outcome(and_(p, _div(a, b)), (False, 6, 0)) == ("value", False)
    assert M.outcome(or_(p, _div(a, b)), (True, 6, 0)) == ("value", True)
    assert M.outcome(or_(p, _div(a, b)), (None, 6, 0)) == ("error", abi.ERR_DIVISION_BY_ZERO)
    rf = bundles()["rejecting_filter"]
    assert not rf.split()[1] and sum(1 for _, o in rf.split()[0] if o[1]) == 3


# ---- b. laziness and NULL logic through FilterAndProject ---------------------------------------------------------------------------------------
def out_bits(types, row):
    return tuple(M.bits(t, v) for t, v in zip(types, row))


@on_gpu
@pytest.mark.parametrize("name", LAZINESS)
def test_laziness_filter_project(gpu, name):
    b = bundles()[name]
    values, errors = b.split()
    make = b.operator
    rows = [r for r, _ in values]
    for page_rows in value_pages(rows):
        want = [out_bits(b.out_types(), b.outcome(r)[2]) for r in page_rows if b.outcome(r)[1]]
        host = page_of(b.columns, page_rows)
        for page in (host, upload_page(host)):
            got = [out_bits(b.out_types(), r) for r in rows_of(make(), [page])]
            assert got == want, (name, page.mem, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:5])
    base = tile(rows)
    for r, (_, status) in errors:
        for pos in POSITIONS:
            page_rows = list(base)
            page_rows[pos] = r
            assert status_of(make, [page_of(b.columns, page_rows)]) == status, (name, r, pos)


# ---- c. the same row function inside the fused kernels ---------------------------------------------------------------------------------------
# Two channels are added behind a bundle's: `live` (the filter is live > 0 AND the bundle's own: a dead row is rejected before anything
# of it is evaluated, so raising rows ride along dead in the value pages and must not raise) and `key` (the group key of the tier).
TIERS = ["plain", "staged", "few_groups", "hbm_table", "join_probe"]
BUILD_KEYS = 8


def fused_plan(b):
    n = len(b.columns)
    live, key = field(n, abi.BIGINT), field(n + 1, abi.BIGINT)
    alive = live > constant(0, abi.BIGINT)
    flt = alive if b.filter is None else and_(alive, b.filter)
    aggs = [(abi.AGG_COUNT_STAR, -1, None)]
    return n, key, flt, aggs


def fused_operator(b, tier):
    """-> (operator, closer)"""
    n, key, flt, aggs = fused_plan(b)
    types = b.types() + [abi.BIGINT, abi.BIGINT]
    if tier in ("plain", "staged"):
        for j, p in enumerate(b.projections):
            aggs += [(abi.AGG_MIN, j, p.type), (abi.AGG_MAX, j, p.type), (abi.AGG_COUNT, j, p.type)]
        return FusedAggregationOperator(types, flt, b.projections, [], aggs), None
    projections = [key] + b.projections
    for j, p in enumerate(b.projections):
        aggs += [(abi.AGG_MIN, j + 1, p.type), (abi.AGG_MAX, j + 1, p.type), (abi.AGG_COUNT, j + 1, p.type)]
    if tier == "few_groups":
        return FusedAggregationOperator(types, flt, projections, [0], aggs), None
    if tier == "hbm_table":
        return FusedAggregationOperator(types, flt, projections, [0], aggs, expected_groups=(1 << 20) + 1), None
    bridge = LookupSourceFactory()
    builder = HashBuilderOperator(bridge, [abi.BIGINT, abi.BIGINT], [0], [1])
    joined = [p.type for p in projections] + [abi.BIGINT]
    op = FusedJoinAggregationOperator(bridge, types, flt, projections, [0], list(range(len(projections))), joined, [0], aggs)
    keys = np.arange(BUILD_KEYS, dtype=np.int64)
    Driver([Page([Block.bigint(keys), Block.bigint(keys * 10)], BUILD_KEYS)], [builder]).run()
    return op, builder


def key_of(tier, index):
    return index if tier == "hbm_table" else index % BUILD_KEYS


def fused_page(b, tier, rows, lives, first_index):
    ext = [tuple(r) + (lv, key_of(tier, first_index + i)) for i, (r, lv) in enumerate(zip(rows, lives))]
    return page_of(list(b.columns) + ["BIGINT", "BIGINT"], ext)


def aggregate(types, outputs):
    """count(*), then min / max / count of every projection over the selected rows' written values (NULLs are not counted)"""
    row = [len(outputs)]
    for j, t in enumerate(types):
        vs = [o[j] for o in outputs if o[j] is not None]
        row += [min(vs) if vs else None, max(vs) if vs else None, len(vs)]
    return tuple(row)


def expected_groups_of(b, tier, rows, lives, first_index, acc):
    for i, (r, lv) in enumerate(zip(rows, lives)):
        o = b.outcome(r) if lv > 0 else ("value", False, None)
        assert o[0] == "value"
        if o[1]:
            acc.setdefault(key_of(tier, first_index + i), []).append(o[2])


def check_name(tier, name):
    if tier == "plain":
        assert name.startswith("pa_fused_global_") and "staged" not in name, name
    elif tier == "staged":
        assert name.startswith("pa_fused_global_staged_"), name
    elif tier == "few_groups":
        assert name.startswith("pa_fused_lds_"), name
    elif tier == "hbm_table":
        assert name.startswith("pa_fused_gt_"), name
    else:
        assert name.startswith("pa_fused_probe_"), name


def run_fused(b, tier, pages):
    op, builder = fused_operator(b, tier)
    try:
        rows = [r for p in to_pages(op, pages) for r in p.to_rows()]
        return rows, op.kernelName()
    finally:
        op.close()
        if builder is not None:
            builder.close()


def tier_env(monkeypatch, tier):
    monkeypatch.setenv("PRESTO_AMD_STAGED", "1" if tier == "staged" else "0")
    if tier == "hbm_table":
        monkeypatch.setenv("PRESTO_AMD_NO_PARTITIONED", "1")   # the HBM table's own kernel, not the partition-owned LDS tables in front of it


# the probe leg takes the expressions of (b) and BIGINT arithmetic; the other legs also INTEGER and DATE arithmetic
FUSED_CASES = [(name, tier) for name in ARITH + LAZINESS for tier in TIERS if tier != "join_probe" or name not in ("arith:INTEGER", "arith:DATE")]
FUSED_IDS = ["%s-%s" % c for c in FUSED_CASES]


def out_bits_agg(types, row):
    """count(*), then (min, max, count) per projection: floats as bit patterns"""
    out = [row[0]]
    for j, t in enumerate(types):
        lo, hi, n = row[1 + 3 * j:4 + 3 * j]
        out += [M.bits(t, lo), M.bits(t, hi), n]
    return tuple(out)


@on_gpu
@pytest.mark.parametrize("name,tier", FUSED_CASES, ids=FUSED_IDS)
def test_fused_values(gpu, monkeypatch, name, tier):
    tier_env(monkeypatch, tier)
    for b in bundles()[name].parts(tier):
        values, errors = b.split()
        rows = [(r, 1) for r, _ in values] + [(r, 0) for r, _ in errors]      # raising rows ride along dead
        types = b.out_types()
        if tier in ("plain", "staged"):
            # slices of at most 8 rows to a fresh operator each, so that min / max / count pin few rows at a time (the kernel is cached)
            for at in range(0, len(rows), 8):
                part = rows[at:at + 8]
                got, kernel = run_fused(b, tier, [fused_page(b, tier, [r for r, _ in part], [lv for _, lv in part], 0)])
                check_name(tier, kernel)
                outputs = [b.outcome(r)[2] for r, lv in part if lv > 0 and b.outcome(r)[1]]
                assert [out_bits_agg(types, g) for g in got] == [out_bits_agg(types, aggregate(types, outputs))], (b.name, tier, at, part)
            continue
        pages, acc, at = [], {}, 0
        for i in range(0, len(rows), PAGE):
            part = tile(rows[i:i + PAGE])
            pages.append(fused_page(b, tier, [r for r, _ in part], [lv for _, lv in part], at))
            expected_groups_of(b, tier, [r for r, _ in part], [lv for _, lv in part], at, acc)
            at += PAGE
        got, kernel = run_fused(b, tier, pages)
        check_name(tier, kernel)
        want = {k: out_bits_agg(types, aggregate(types, outs)) for k, outs in acc.items()}
        have = {g[0]: out_bits_agg(types, g[1:]) for g in got}
        assert len(got) == len(have)
        wrong = [(k, have.get(k), w) for k, w in sorted(want.items()) if have.get(k) != w]
        assert sorted(have) == sorted(want) and not wrong, (b.name, tier, len(wrong), wrong[:3])


@on_gpu
@pytest.mark.parametrize("name,tier", [c for c in FUSED_CASES if c[0] != "rejecting_filter"], ids=[i for c, i in zip(FUSED_CASES, FUSED_IDS) if c[0] != "rejecting_filter"])
def test_fused_errors(gpu, monkeypatch, name, tier):
    tier_env(monkeypatch, tier)
    for b in bundles()[name].parts(tier):
        values, errors = b.split()
        base = tile([r for r, _ in values])
        assert errors
        for k, (r, (_, status)) in enumerate(errors):
            rows = list(base)
            rows[POSITIONS[k % 3]] = r       # one offending row per page: the status is determined
            page = fused_page(b, tier, rows, [1] * PAGE, 0)
            op, builder = fused_operator(b, tier)
            try:
                with pytest.raises(PrestoAmdError) as e:
                    to_pages(op, [page])
                assert e.value.status == status, (b.name, tier, r, e.value.status, status)
            finally:
                op.close()
                if builder is not None:
                    builder.close()


# ---- the staged NULL case -------------------------------------------------------------------------------------------------------------------
def staged_divide_operator():
    """the filter of divide_operator in tests/test_gpu_staged.py; the first channel is nullable here"""
    filt = and_(field(0, abi.BIGINT) >= constant(0, abi.BIGINT), (constant(100, abi.BIGINT) / field(1, abi.BIGINT)) > constant(1, abi.BIGINT))
    return FusedAggregationOperator([abi.BIGINT, abi.BIGINT], filt, [field(0, abi.BIGINT)], [], [(abi.AGG_SUM, 0, abi.BIGINT), (abi.AGG_COUNT_STAR, -1, None)])


def staged_divide_page(special, pos):
    """benign rows: a >= 0 with divisor 5 (selected: 100 / 5 > 1), a < 0 with divisor 0 (FALSE first conjunct: the division is hidden),
    a NULL with divisor 5 (NULL AND TRUE: not selected); `special` = (a, b) goes to `pos`"""
    a = [(i % 7) - 3 if i % 11 else None for i in range(PAGE)]
    b = [0 if (v is not None and v < 0) else 5 for v in a]
    if special is not None:
        a[pos], b[pos] = special
    return a, b, Page([M.block_of("BIGINT", a), M.block_of("BIGINT", b)], PAGE)


@on_gpu
@pytest.mark.parametrize("mode", ["0", "1"], ids=["plain", "staged"])
def test_staged_null_first_conjunct_does_not_hide_the_second(gpu, monkeypatch, mode):
    monkeypatch.setenv("PRESTO_AMD_STAGED", mode)
    flt = and_(field(0, abi.BIGINT) >= constant(0, abi.BIGINT), (constant(100, abi.BIGINT) / field(1, abi.BIGINT)) > constant(1, abi.BIGINT))
    # the page without a special row, and with a FALSE first conjunct over a zero divisor: no error; values by the model
    for special in (None, (-1, 0)):
        for pos in POSITIONS:
            a, b, page = staged_divide_page(special, pos)
            selected = [x for x, y in zip(a, b) if M.evaluate(flt, (x, y)) is True]
            op = staged_divide_operator()
            try:
                got = [r for p in to_pages(op, [page]) for r in p.to_rows()]
                kernel = op.kernelName()
            finally:
                op.close()
            assert ("staged" in kernel) == (mode == "1") and kernel.startswith("pa_fused_global_"), kernel
            assert got == [(sum(selected), len(selected))] and selected
    # a NULL first conjunct does not hide the division by zero (AndCodeGenerator: only FALSE decides)
    assert M.outcome(flt, (None, 0)) == ("error", abi.ERR_DIVISION_BY_ZERO)
    for pos in POSITIONS:
        _, _, page = staged_divide_page((None, 0), pos)
        assert status_of(staged_divide_operator, [page]) == abi.ERR_DIVISION_BY_ZERO, pos


# ---- documented divergences -------------------------------------------------------------------------------------------------------------------
def _fp_outcome(types, columns, expr, row):
    make = lambda: FilterAndProjectOperator(types, None, [expr])
    page = M.page_of(columns, [row])
    op = make()
    try:
        out = [r for p in to_pages(op, [page]) for r in p.to_rows()]
        return "value", out[0][0]
    except PrestoAmdError as e:
        return "error", e.status
    finally:
        op.close()


def _two_integers():
    return field(0, abi.INTEGER), field(1, abi.INTEGER)


def _three_bigints():
    return field(0, abi.BIGINT), field(1, abi.BIGINT), field(2, abi.BIGINT)


# name (the tag of the entry in DESIGN.md section 5) -> [(columns, expression, row, the reference's outcome (= the model's), the device's)]
def divergences():
    a, b = _two_integers()
    x, y, z = _three_bigints()
    I2, B3 = ["INTEGER", "INTEGER"], ["BIGINT", "BIGINT", "BIGINT"]
    MIN = M.I32_MIN
    return {
        "expr-integer-division-narrows": [
            (I2, (a / b).eq(a), (MIN, -1), ("value", False), ("value", True)),                      # 2147483648 = MIN is false; narrowed, MIN = MIN
            (I2, (a / b).cast(abi.BIGINT), (MIN, -1), ("value", 2147483648), ("value", MIN)),
            (I2, (a / b) / b, (MIN, -1), ("value", MIN), ("value", MIN)),                           # 2147483648 / -1 written as MIN; MIN / -1 narrowed again
        ],
        "expr-eager-operands": [
            (B3, x + (y / z), (None, 6, 0), ("value", None), ("error", abi.ERR_DIVISION_BY_ZERO)),   # a NULL argument ends the reference's call
            (B3, x.between(y, y / z), (1, 6, 0), ("value", False), ("error", abi.ERR_DIVISION_BY_ZERO)),   # min <= value is FALSE: max is not evaluated
            (B3, x.isin(y, y / z), (6, 6, 0), ("value", True), ("error", abi.ERR_DIVISION_BY_ZERO)),       # matched before the raising candidate
        ],
        "expr-invalid-cast-status": [
            (["BIGINT"], field(0, abi.BIGINT).cast(M.D82), (10 ** 6,), ("error", M.INVALID_CAST_ARGUMENT), ("error", abi.ERR_NUMERIC_VALUE_OUT_OF_RANGE)),
        ],
    }


def design_divergence_tags():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "DESIGN.md")).read()
    section = text[text.index("## 5. Parity"):text.index("## 6. Measurement")]
    return set(re.findall(r"`(expr-[a-z-]+)`", section))


def test_design_lists_exactly_the_divergences_of_the_table():
    assert design_divergence_tags() == set(divergences())


def test_divergences_differ_from_the_reference_as_stated():
    for name, rows in divergences().items():
        for columns, expr, row, reference, device in rows:
            assert M.outcome(expr, row) == reference, (name, row)
    assert M.INVALID_CAST_ARGUMENT == abi.ERR_NUMERIC_VALUE_OUT_OF_RANGE    # the ABI has one status for the two


@on_gpu
@pytest.mark.parametrize("name", sorted(divergences()))
def test_divergence_is_what_design_says(gpu, name):
    assert name in design_divergence_tags()
    for columns, expr, row, reference, device in divergences()[name]:
        assert _fp_outcome(M.input_types(columns), columns, expr, row) == device, (name, row)
