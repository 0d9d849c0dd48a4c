"""GPU checks of NestedLoopBuildOperator + NestedLoopJoinOperator against tests/nested_loop_model.py (two plain loops in probe-major
order, the filter evaluated by tests/expr_model.py).  Comparisons are exact: integers by value, DOUBLE / REAL by bits, VARCHAR by
bytes -- the output columns are flat copies, so every value is compared as the bit pattern its input block held.  Everything with a
filter runs under both lane mappings of the pair kernels (PRESTO_AMD_NL_VARIANT=0 and 1) and must give identical pages.  Every product
stays under about 2 * 10^6 pairs."""
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

from presto_amd import abi
from presto_amd._lib import PrestoAmdError
from presto_amd.expr import and_, call, constant, field, or_
from presto_amd.operators import (HashBuilderOperator, LookupJoinOperator, LookupSourceFactory, NestedLoopBuildOperator, NestedLoopJoinBridge,
                                  NestedLoopJoinOperator, download_page, to_pages, upload_page)
from presto_amd.page import Block, Page
from tests import expr_model as M
from tests import nested_loop_model as NL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = int(re.search(r"kNestedLoopLdsChunk\s*=\s*(\d+)", open(os.path.join(ROOT, "presto_amd", "csrc", "nested_loop_kernels.hpp")).read()).group(1))
VARIANTS = ["0", "1"]
FUZZ_SEEDS = int(os.environ.get("PA_FUZZ_SEEDS", "8"))


def lt(a, b):
    return call(abi.OP_LESS_THAN, abi.BOOLEAN, a, b)


def eq(a, b):
    return call(abi.OP_EQUAL, abi.BOOLEAN, a, b)


# ---- pages, and rows as the bit patterns their blocks hold -------------------------------------------------------------------------------
def pages_of(columns, rows, cuts=None):
    """host pages of `rows` (one channel per type name of expr_model.TYPES), cut at the row numbers in `cuts`"""
    edges = [0] + list(cuts or []) + [len(rows)]
    return [M.page_of(columns, rows[a:b]) for a, b in zip(edges, edges[1:])]


def raw_column(block, n):
    nulls = block.nulls
    if block.type == abi.VARCHAR:
        data, off = block.values.tobytes(), block.offsets.tolist()
        out = [data[off[i]:off[i + 1]] for i in range(n)]
    elif block.type == abi.LONG_DECIMAL:
        out = [tuple(w) for w in np.asarray(block.values).reshape(-1, 2)[:n].tolist()]
    else:
        v = np.ascontiguousarray(block.values[:n])
        out = v.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[v.dtype.itemsize]).tolist()
    return [None if nulls is not None and nulls[i] else out[i] for i in range(n)]


def raw_rows(pages):
    """every row of host pages of flat blocks, each value as the bits the block holds (None for NULL)"""
    rows = []
    for p in pages:
        cols = [raw_column(b, p.position_count) for b in p.blocks]
        rows += [tuple(c[i] for c in cols) for i in range(p.position_count)]
    return rows


def host(page):
    return page if page.mem == abi.MEM_HOST else download_page(page)


# ---- the join ----------------------------------------------------------------------------------------------------------------------------
def build_side(build_columns, build_pages):
    bridge = NestedLoopJoinBridge()
    builder = NestedLoopBuildOperator(bridge, M.input_types(build_columns))
    assert to_pages(builder, build_pages) == []
    return bridge, builder


def drain(join, page, log=None):
    """one probe page through the join: its output pages; log collects needsInput as seen before every delivered page"""
    assert join.needsInput()
    join.addInput(page)
    out = []
    while True:
        waiting = join.needsInput()
        p = join.getOutput()
        if p is None:
            return out
        if log is not None:
            log.append(waiting)
        out.append(host(p))


def join_pages(bridge, probe_columns, probe_pages, probe_out, build_out, filter_expr, variant, monkeypatch, output_mem=abi.MEM_HOST, log=None):
    """the output pages (on the host) of the probe pages under one lane mapping"""
    if variant is None:
        monkeypatch.delenv("PRESTO_AMD_NL_VARIANT", raising=False)
    else:
        monkeypatch.setenv("PRESTO_AMD_NL_VARIANT", variant)
    join = NestedLoopJoinOperator(bridge, M.input_types(probe_columns), probe_out, build_out, filter=filter_expr, output_mem=output_mem)
    out = []
    for page in probe_pages:
        if page.position_count > 0:
            out += drain(join, page, log)
    join.finish()
    assert join.isFinished() and join.getOutput() is None
    join.close()
    return out


def check_join(monkeypatch, probe_columns, probe_rows, build_columns, build_rows, probe_out, build_out, filter_expr, probe_cuts=None, build_cuts=None,
               expected=None):
    """model == device under both lane mappings (and the default), page for page identical between them; returns the output pages"""
    probe_pages, build_pages = pages_of(probe_columns, probe_rows, probe_cuts), pages_of(build_columns, build_rows, build_cuts)
    raw_p, raw_b = raw_rows(probe_pages), raw_rows(build_pages)
    if expected is None:
        expected = NL.pairs(probe_rows, build_rows, filter_expr)
    want = [tuple(raw_p[i][c] for c in probe_out) + tuple(raw_b[j][c] for c in build_out) for i, j in expected]
    bridge, builder = build_side(build_columns, build_pages)
    assert bridge.rows() == len(build_rows)
    first = None
    for variant in (VARIANTS + [None] if filter_expr is not None else [None]):
        out = join_pages(bridge, probe_columns, probe_pages, probe_out, build_out, filter_expr, variant, monkeypatch)
        got = raw_rows(out)
        assert len(got) == len(want), (variant, len(got), len(want))
        assert got == want, variant
        sizes = [p.position_count for p in out]
        if first is None:
            first = sizes
        assert sizes == first, variant
    builder.close()
    bridge.destroy()
    return out


# ---- known answers, by hand ----------------------------------------------------------------------------------------------------------------
def test_three_by_two_without_a_filter(gpu, monkeypatch):
    out = check_join(monkeypatch, ["BIGINT", "VARCHAR"], [(1, b"a"), (2, b"b"), (3, None)], ["BIGINT"], [(10,), (20,)], [0, 1], [0], None,
                     expected=[(0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 1)])
    assert [r for p in out for r in p.to_rows()] == [(1, b"a", 10), (1, b"a", 20), (2, b"b", 10), (2, b"b", 20), (3, None, 10), (3, None, 20)]


def test_less_than_with_nulls_on_both_sides(gpu, monkeypatch):
    """p.x < b.y: NULL is not a match"""
    f = lt(field(1, abi.BIGINT), field(0, abi.BIGINT))
    out = check_join(monkeypatch, ["BIGINT"], [(1,), (None,), (5,)], ["BIGINT"], [(3,), (None,), (6,)], [0], [0], f, expected=[(0, 0), (0, 2), (2, 2)])
    assert [r for p in out for r in p.to_rows()] == [(1, 3), (1, 6), (5, 6)]


def test_scalar_subquery_shape(gpu, monkeypatch):
    """M = 1: p.x > b.v, the build column not in the output"""
    f = call(abi.OP_GREATER_THAN, abi.BOOLEAN, field(1, abi.DOUBLE), field(0, abi.DOUBLE))
    out = check_join(monkeypatch, ["DOUBLE", "BIGINT"], [(1.5, 0), (2.5, 1), (float("nan"), 2), (3.0, 3), (None, 4), (1e300, 5)], ["DOUBLE"], [(2.5,)], [1, 0], [],
                     f, expected=[(3, 0), (5, 0)])
    assert [r[0] for p in out for r in p.to_rows()] == [3, 5]


def test_empty_sides_give_no_page(gpu, monkeypatch):
    f = lt(field(1, abi.BIGINT), field(0, abi.BIGINT))
    assert check_join(monkeypatch, ["BIGINT"], [(1,), (2,)], ["BIGINT"], [], [0], [0], f, expected=[]) == []
    assert check_join(monkeypatch, ["BIGINT"], [(1,), (2,)], ["BIGINT"], [], [0], [0], None, expected=[]) == []
    assert check_join(monkeypatch, ["BIGINT"], [], ["BIGINT"], [(1,)], [0], [0], f, expected=[]) == []


# ---- tile edges ----------------------------------------------------------------------------------------------------------------------------
BUILD_SIZES = [0, 1, 63, 64, 65, 255, 256, 257, CHUNK + 1]
PROBE_SIZES = [1, 63, 64, 65, 255, 256, 257, 1025]
X_LT_Y = lt(field(1, abi.BIGINT), field(0, abi.BIGINT))


def int_rows(rng, n, nulls=False):
    return [(None if nulls and rng.random() < 0.1 else rng.randrange(-50, 50),) for _ in range(n)]


@pytest.mark.parametrize("m", BUILD_SIZES)
def test_build_row_counts_at_tile_edges(gpu, monkeypatch, m):
    rng = random.Random(m)
    check_join(monkeypatch, ["BIGINT"], int_rows(rng, 65, True), ["BIGINT"], int_rows(rng, m, True), [0], [0], X_LT_Y)


@pytest.mark.parametrize("n", PROBE_SIZES)
def test_probe_row_counts_at_tile_edges(gpu, monkeypatch, n):
    rng = random.Random(n)
    check_join(monkeypatch, ["BIGINT"], int_rows(rng, n, True), ["BIGINT"], int_rows(rng, 65, True), [0], [0], X_LT_Y)


@pytest.mark.parametrize("n,m", [(257, 257), (130, CHUNK + 1)])
@pytest.mark.parametrize("keep", ["nothing", "everything", "last_pair", "one_probe_row"])
def test_filters_that_keep_the_corners(gpu, monkeypatch, n, m, keep):
    """x < y keeps nothing, everything, exactly the pair in the last lane of the last wave, every pair of one probe row only"""
    x, y = [5] * n, [0] * m
    if keep == "everything":
        x, y = [0] * n, [5] * m
    elif keep == "last_pair":
        x[-1], y[-1] = 0, 1
    elif keep == "one_probe_row":
        x[n // 2 + 1] = -1
    # pair channels: 0 b.y, 1 b's row number, 2 p.x, 3 p's row number
    out = check_join(monkeypatch, ["BIGINT", "BIGINT"], [(v, i) for i, v in enumerate(x)], ["BIGINT", "BIGINT"], [(v, j) for j, v in enumerate(y)], [1], [1],
                     lt(field(2, abi.BIGINT), field(0, abi.BIGINT)))
    rows = [r for p in out for r in p.to_rows()]
    assert len(rows) == {"nothing": 0, "everything": n * m, "last_pair": 1, "one_probe_row": m}[keep]
    if keep == "last_pair":
        assert rows == [(n - 1, m - 1)]
    if keep == "one_probe_row":
        assert rows == [(n // 2 + 1, j) for j in range(m)]


# ---- output paging -------------------------------------------------------------------------------------------------------------------------
def check_paging(monkeypatch, bound, probe_rows, build_rows, filter_expr, devices=(False, True)):
    """same rows, same order, more than one page, no page over the bound, needs_input 0 while pages are pending"""
    probe_pages, build_pages = pages_of(["BIGINT"], probe_rows), pages_of(["BIGINT"], build_rows)
    want = NL.nested_loop(probe_rows, build_rows, [0], [0], filter_expr)
    bridge, builder = build_side(["BIGINT"], build_pages)
    sizes = None
    for variant in (VARIANTS if filter_expr is not None else [None]):
        monkeypatch.delenv("PRESTO_AMD_JOIN_MAX_OUTPUT_ROWS", raising=False)
        whole = join_pages(bridge, ["BIGINT"], probe_pages, [0], [0], filter_expr, variant, monkeypatch)
        assert len(whole) == 1
        monkeypatch.setenv("PRESTO_AMD_JOIN_MAX_OUTPUT_ROWS", str(bound))
        log = []
        for device in devices:            # (a device page that comes out as several is kept by the operator)
            pages = [upload_page(p) for p in probe_pages] if device else probe_pages
            out = join_pages(bridge, ["BIGINT"], pages, [0], [0], filter_expr, variant, monkeypatch, log=log)
            assert [r for p in out for r in p.to_rows()] == want, (variant, device)
            assert len(out) > 1 and max(p.position_count for p in out) <= bound
            assert sizes in (None, [p.position_count for p in out])
            sizes = [p.position_count for p in out]
        assert log and not any(log)
    builder.close()
    bridge.destroy()


@pytest.mark.parametrize("bound", [700, 7])
def test_paging_of_a_plain_product(gpu, monkeypatch, bound):
    # (18006 pages at the bound of 7: from a device page only, which is the case that makes the operator keep the page)
    check_paging(monkeypatch, bound, [(i,) for i in range(3001)], [(j,) for j in range(40)], None, devices=(False, True) if bound > 7 else (True,))


@pytest.mark.parametrize("bound", [700, 7])
def test_paging_of_a_filtered_product(gpu, monkeypatch, bound):
    rng = random.Random(bound)
    check_paging(monkeypatch, bound, int_rows(rng, 400), int_rows(rng, 40), X_LT_Y)


@pytest.mark.parametrize("bound", [700, 7])
@pytest.mark.parametrize("filtered", [False, True])
def test_one_probe_row_is_cut_between_build_rows(gpu, monkeypatch, bound, filtered):
    """M = 1500 build rows exceed the bound"""
    rng = random.Random(bound)
    check_paging(monkeypatch, bound, int_rows(rng, 5), int_rows(rng, 1500), X_LT_Y if filtered else None)


# ---- types ---------------------------------------------------------------------------------------------------------------------------------
def edge_values(name, k=9):
    values = list(M.EDGES[name])
    step = max(1, len(values) // k)
    return values[::step][:k] + [None]


def test_every_carried_type_on_either_side(gpu, monkeypatch):
    """every type as a probe and as a build output channel, NULLs, a long decimal and empty / long VARCHARs included; the filter reads BIGINTs"""
    names = M.ALL_TYPES
    rng = random.Random(7)
    long_text = bytes(range(256)) * 5
    def rows(n):
        cols = []
        for name in names:
            pool = edge_values(name) + ([b"", long_text] if name == "VARCHAR" else [])
            cols.append([rng.choice(pool) for _ in range(n)])
        cols.append([rng.randrange(-5, 5) for _ in range(n)])
        return [tuple(c[i] for c in cols) for i in range(n)]
    columns = names + ["BIGINT"]
    k = len(names)
    f = lt(field(len(columns) + k, abi.BIGINT), field(k, abi.BIGINT))
    check_join(monkeypatch, columns, rows(70), columns, rows(33), list(range(k + 1)), list(range(k + 1)), f)
    check_join(monkeypatch, columns, rows(9), columns, rows(5), list(range(k)), list(range(k)), None)


@pytest.mark.parametrize("name", M.ALL_TYPES)
def test_filters_over_each_compared_type(gpu, monkeypatch, name):
    """p.v < b.v (BOOLEAN: =) over the type's edge values and NULL on both sides"""
    t = M.TYPES[name]
    compare = eq if name == "BOOLEAN" else lt
    values = edge_values(name, 12)
    rows = [(v, i) for i, v in enumerate(values)]
    check_join(monkeypatch, [name, "BIGINT"], rows, [name, "BIGINT"], list(reversed(rows)), [0, 1], [1, 0], compare(field(2, t), field(0, t)))


def test_and_or_with_a_null_operand(gpu, monkeypatch):
    rng = random.Random(3)
    probe, build = int_rows(rng, 40, True), int_rows(rng, 30, True)
    null = constant(None, abi.BOOLEAN)
    for f in (and_(X_LT_Y, null), or_(X_LT_Y, null), and_(null, X_LT_Y), or_(null, X_LT_Y), or_(and_(X_LT_Y, null), eq(field(0, abi.BIGINT), field(1, abi.BIGINT)))):
        check_join(monkeypatch, ["BIGINT"], probe, ["BIGINT"], build, [0], [0], f)


def test_like_over_a_build_varchar(gpu, monkeypatch):
    """b.name LIKE 'ab%' AND p.x < b.y: the expected pairs by hand (expr_model has no LIKE)"""
    build = [(b"abc", 5), (b"xab", 9), (None, 9), (b"ab", 1), (b"", 9), (b"abab", 3)]
    probe = [(0,), (2,), (4,), (None,)]
    f = and_(field(0, abi.VARCHAR).like("ab%"), lt(field(2, abi.BIGINT), field(1, abi.BIGINT)))
    expected = [(i, j) for i, (x,) in enumerate(probe) for j, (s, y) in enumerate(build) if s is not None and s.startswith(b"ab") and x is not None and x < y]
    assert expected == [(0, 0), (0, 3), (0, 5), (1, 0), (1, 5), (2, 0)]
    check_join(monkeypatch, ["BIGINT"], probe, ["VARCHAR", "BIGINT"], build, [0], [0, 1], f, expected=expected)


# ---- independence from page cuts and encodings --------------------------------------------------------------------------------------------
def test_page_cuts_and_encodings_do_not_change_the_rows(gpu, monkeypatch):
    rng = random.Random(11)
    columns = ["BIGINT", "VARCHAR"]
    words = [b"", b"a", b"bb", b"a longer string", None]
    probe = [(rng.choice([None] + list(range(-4, 4))), rng.choice(words)) for _ in range(300)]
    build = [(rng.choice([None] + list(range(-4, 4))), rng.choice(words)) for _ in range(90)]
    # pair channels: 0 b.k, 1 b.s, 2 p.k, 3 p.s
    f = or_(lt(field(2, abi.BIGINT), field(0, abi.BIGINT)), eq(field(1, abi.VARCHAR), field(3, abi.VARCHAR)))
    want = NL.nested_loop(probe, build, [0, 1], [1, 0], f)

    def encoded(rows, how):
        """the same rows as dictionary / RLE blocks: a dictionary of the distinct rows, runs as RLE pages"""
        if how == "dictionary":
            distinct = sorted(set(rows), key=repr)
            ids = [distinct.index(r) for r in rows]
            flat = M.page_of(columns, distinct)
            return [Page([Block.dictionary_block(b, ids) for b in flat.blocks], len(rows))]
        pages, at = [], 0
        while at < len(rows):      # runs of equal rows as RLE pages (most are one row long)
            run = 1
            while at + run < len(rows) and rows[at + run] == rows[at]:
                run += 1
            one = M.page_of(columns, rows[at:at + 1])
            pages.append(Page([Block.rle(b, run) for b in one.blocks], run))
            at += run
        return pages

    def empty():
        return M.page_of(columns, [])

    shapes = {
        "one page": (pages_of(columns, probe), pages_of(columns, build)),
        "small pages": (pages_of(columns, probe, list(range(7, 300, 7))), pages_of(columns, build, list(range(5, 90, 5)))),
        "empty pages between": ([empty()] + pages_of(columns, probe, [100, 200]) + [empty()], [empty()] + pages_of(columns, build, [1, 50]) + [empty()]),
        "dictionary": (encoded(probe, "dictionary"), encoded(build, "dictionary")),
        "rle": (encoded(sorted(probe, key=repr), "rle"), encoded(sorted(build, key=repr), "rle")),
    }
    for name, (probe_pages, build_pages) in shapes.items():
        expect = want if name != "rle" else NL.nested_loop(sorted(probe, key=repr), sorted(build, key=repr), [0, 1], [1, 0], f)
        for device in (False, True):
            bp = [upload_page(p) if device and p.position_count else p for p in build_pages]
            pp = [upload_page(p) if device and p.position_count else p for p in probe_pages]
            bridge = NestedLoopJoinBridge()
            builder = NestedLoopBuildOperator(bridge, M.input_types(columns))
            for p in bp:                       # (empty pages are accepted)
                builder.addInput(p)
            builder.finish()
            for variant in VARIANTS:
                for mem in (abi.MEM_HOST, abi.MEM_DEVICE):
                    out = join_pages(bridge, columns, pp, [0, 1], [1, 0], f, variant, monkeypatch, output_mem=mem)
                    assert [r for p in out for r in p.to_rows()] == expect, (name, device, variant, mem)
            builder.close()
            bridge.destroy()


# ---- errors --------------------------------------------------------------------------------------------------------------------------------
DIV = call(abi.OP_GREATER_THAN, abi.BOOLEAN, call(abi.OP_DIVIDE, abi.BIGINT, field(1, abi.BIGINT), field(0, abi.BIGINT)), constant(0, abi.BIGINT))


@pytest.mark.parametrize("variant", VARIANTS)
def test_division_by_zero_fails_the_rectangle(gpu, monkeypatch, variant):
    """p.x / b.y > 0 with one zero b.y: FilterAndProject's status on get_output, nothing of that rectangle emitted, earlier pages stand"""
    probe, build = [(i + 1,) for i in range(20)], [(2,), (0,), (1,)]
    assert NL.outcome(probe, build, [0], [0], DIV) == ("error", abi.ERR_DIVISION_BY_ZERO)
    bridge, builder = build_side(["BIGINT"], pages_of(["BIGINT"], build))
    monkeypatch.setenv("PRESTO_AMD_NL_VARIANT", variant)
    join = NestedLoopJoinOperator(bridge, [abi.BIGINT], [0], [0], filter=DIV)
    join.addInput(pages_of(["BIGINT"], probe)[0])
    with pytest.raises(PrestoAmdError) as e:
        join.getOutput()
    assert e.value.status == abi.ERR_DIVISION_BY_ZERO
    assert join.getOutput() is None            # nothing of the page is emitted afterwards
    join.close()
    # the rectangles before the failing one were delivered: the zero sits in the last of three build ranges of one probe row
    monkeypatch.setenv("PRESTO_AMD_JOIN_MAX_OUTPUT_ROWS", "1")
    join = NestedLoopJoinOperator(bridge, [abi.BIGINT], [0], [0], filter=DIV)
    join.addInput(pages_of(["BIGINT"], [(7,)])[0])
    first = join.getOutput()
    assert first.to_rows() == [(7, 2)]
    with pytest.raises(PrestoAmdError) as e:
        join.getOutput()
    assert e.value.status == abi.ERR_DIVISION_BY_ZERO
    join.close()
    builder.close()
    bridge.destroy()


def test_an_error_behind_a_false_conjunct_follows_the_model(gpu, monkeypatch):
    guarded = and_(call(abi.OP_NOT_EQUAL, abi.BOOLEAN, field(0, abi.BIGINT), constant(0, abi.BIGINT)), DIV)
    probe, build = [(4,), (8,), (None,), (-3,)], [(2,), (0,), (1,), (None,)]
    assert NL.outcome(probe, build, [0], [0], guarded)[0] == "rows"
    check_join(monkeypatch, ["BIGINT"], probe, ["BIGINT"], build, [0], [0], guarded)
    # ... and in the other order the division is evaluated first: every pair raises it
    unguarded = and_(DIV, call(abi.OP_NOT_EQUAL, abi.BOOLEAN, field(0, abi.BIGINT), constant(0, abi.BIGINT)))
    assert NL.outcome(probe, build, [0], [0], unguarded) == ("error", abi.ERR_DIVISION_BY_ZERO)
    bridge, builder = build_side(["BIGINT"], pages_of(["BIGINT"], build))
    for variant in VARIANTS:
        monkeypatch.setenv("PRESTO_AMD_NL_VARIANT", variant)
        join = NestedLoopJoinOperator(bridge, [abi.BIGINT], [0], [0], filter=unguarded)
        join.addInput(pages_of(["BIGINT"], probe)[0])
        with pytest.raises(PrestoAmdError) as e:
            join.getOutput()
        assert e.value.status == abi.ERR_DIVISION_BY_ZERO
        join.close()
    builder.close()
    bridge.destroy()


# ---- state machine and lifetime ------------------------------------------------------------------------------------------------------------
def status_of(fn):
    try:
        fn()
    except PrestoAmdError as e:
        return e.status
    return abi.OK


def test_state_machine(gpu):
    one = [abi.BIGINT]
    page = pages_of(["BIGINT"], [(1,), (2,)])[0]
    bridge = NestedLoopJoinBridge()
    assert status_of(lambda: NestedLoopJoinOperator(bridge, one, [0], [0])) == abi.ERR_ILLEGAL_STATE     # no builder yet
    assert status_of(bridge.rows) == abi.ERR_ILLEGAL_STATE
    builder = NestedLoopBuildOperator(bridge, one)
    assert status_of(lambda: NestedLoopBuildOperator(bridge, one)) == abi.ERR_ILLEGAL_STATE              # a second builder
    a, b = NestedLoopJoinOperator(bridge, one, [0], [0]), NestedLoopJoinOperator(bridge, one, [0], [0], filter=X_LT_Y)
    # blocked before publication
    for j in (a, b):
        assert j.isBlocked() and not j.needsInput() and not j.isFinished()
        assert status_of(lambda: check_add(j, page)) == abi.ERR_ILLEGAL_STATE
    assert builder.needsInput() and builder.getOutput() is None and not builder.isFinished()
    builder.addInput(pages_of(["BIGINT"], [(5,)])[0])
    builder.addInput(pages_of(["BIGINT"], [])[0])
    builder.addInput(pages_of(["BIGINT"], [(1,), (2,)])[0])
    assert builder.memoryBytes() > 0
    builder.finish()
    assert builder.isFinished() and not builder.needsInput() and bridge.rows() == 3
    assert status_of(lambda: check_add(builder, page)) == abi.ERR_ILLEGAL_STATE
    # two join operators share the handle
    for j in (a, b):
        assert not j.isBlocked() and j.needsInput()
    assert [r for p in drain(a, page) for r in p.to_rows()] == [(1, 5), (1, 1), (1, 2), (2, 5), (2, 1), (2, 2)]
    assert [r for p in drain(b, page) for r in p.to_rows()] == [(1, 5), (1, 2), (2, 5)]
    assert a.memoryBytes() > 0
    # a join created after the build holds what it reads (every channel was held: no join had registered a narrower need)
    c = NestedLoopJoinOperator(bridge, one, [0], [0])
    assert len(drain(c, page)[0].to_rows()) == 6
    for j in (a, b, c):
        j.finish()
        assert j.isFinished() and not j.needsInput()
        assert status_of(lambda: check_add(j, page)) == abi.ERR_ILLEGAL_STATE
        j.close()
    builder.close()
    bridge.destroy()


def check_add(op, page):
    """addInput without the mirror's wait for needsInput"""
    import ctypes as C
    from presto_amd._lib import check, lib
    cpage, keep = page.to_c()
    check(lib().pa_op_add_input(op._h, C.byref(cpage)))


def test_a_channel_nobody_reads_is_not_held(gpu):
    types = [abi.BIGINT, abi.VARCHAR]
    bridge = NestedLoopJoinBridge()
    builder = NestedLoopBuildOperator(bridge, types)
    join = NestedLoopJoinOperator(bridge, [abi.BIGINT], [0], [0])          # reads build channel 0 only
    builder.addInput(M.page_of(["BIGINT", "VARCHAR"], [(i, b"x" * 1000) for i in range(1000)]))
    builder.finish()
    assert builder.memoryBytes() < 500000                                  # the megabyte of strings is not held
    assert status_of(lambda: NestedLoopJoinOperator(bridge, [abi.BIGINT], [0], [1])) == abi.ERR_ILLEGAL_STATE
    assert len(drain(join, pages_of(["BIGINT"], [(1,)])[0])[0].to_rows()) == 1000
    for op in (join, builder):
        op.close()
    bridge.destroy()


@pytest.mark.parametrize("order", ["handle builder join", "join builder handle", "builder handle join", "join handle builder", "handle join builder"])
def test_destroy_in_each_order(gpu, order):
    bridge = NestedLoopJoinBridge()
    builder = NestedLoopBuildOperator(bridge, [abi.BIGINT])
    join = NestedLoopJoinOperator(bridge, [abi.BIGINT], [0], [0], filter=X_LT_Y)
    to_pages(builder, pages_of(["BIGINT"], [(3,), (9,)]))
    page = pages_of(["BIGINT"], [(5,)])[0]
    steps = {"handle": bridge.destroy, "builder": builder.close, "join": join.close}
    for k, name in enumerate(order.split()):
        if name == "join":
            assert drain(join, page)[0].to_rows() == [(5, 9)]      # still whole, whatever went before
        steps[name]()


# ---- refusals that need the build types, on the device ----------------------------------------------------------------------------------
def test_join_creation_checks(gpu):
    bridge = NestedLoopJoinBridge()
    builder = NestedLoopBuildOperator(bridge, [abi.BIGINT, abi.DOUBLE])
    one = [abi.BIGINT]
    make = lambda *a, **kw: status_of(lambda: NestedLoopJoinOperator(bridge, *a, **kw))
    assert make(one, [0], [2]) == abi.ERR_INVALID_ARGUMENT
    assert make(one, [0], [0], filter=lt(field(3, abi.BIGINT), field(0, abi.BIGINT))) == abi.ERR_INVALID_ARGUMENT
    assert make(one, [0], [0], filter=call(abi.OP_ADD, abi.BIGINT, field(2, abi.BIGINT), field(0, abi.BIGINT))) == abi.ERR_INVALID_ARGUMENT
    assert make(one, [], []) == abi.ERR_NOT_SUPPORTED
    assert make([abi.BIGINT, abi.ROW], [0], [0]) == abi.ERR_NOT_SUPPORTED
    assert make(one, [0], [0], filter=lt(field(2, abi.BIGINT), field(1, abi.DOUBLE))) == abi.ERR_NOT_SUPPORTED
    assert make([abi.ROW], [0], [5]) == abi.ERR_INVALID_ARGUMENT         # an invalid argument before a refusal
    assert make(one, [0], [1, 0]) == abi.OK
    builder.close()
    bridge.destroy()


# ---- a scrubbed pool, in a child process ---------------------------------------------------------------------------------------------------
def test_on_a_scrubbed_pool(gpu):
    """A filtered case and the paging once more with every recycled HBM block overwritten before it is handed out (PRESTO_AMD_POOL_SCRUB,
    pool.cpp): counts, offsets or position lists that relied on what a block's previous owner left behind fail here."""
    env = dict(os.environ, PRESTO_AMD_POOL_SCRUB="0xA5", PA_FUZZ_SEEDS="2")
    picks = ["test_less_than_with_nulls_on_both_sides", "test_paging_of_a_filtered_product", "test_fuzz", "test_and_or_with_a_null_operand"]
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider", "tests/test_gpu_nested_loop.py", "-k",
                        " or ".join(picks)], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    tail = r.stdout.decode()[-3000:]
    assert r.returncode == 0, tail
    assert " passed" in tail and "failed" not in tail


# ---- fuzz ----------------------------------------------------------------------------------------------------------------------------------
FUZZ_TYPES = ["BIGINT", "INTEGER", "DOUBLE", "REAL", "VARCHAR", "DECIMAL", "DATE"]


def fuzz_value(rng, name):
    if name == "VARCHAR":
        return rng.choice([b"", b"a", b"ab", b"b", b"ba", b"zz"])
    if name == "DOUBLE":
        return rng.choice([0.0, -0.0, 1.5, -2.25, float("nan"), float("inf"), 3.0])
    if name == "REAL":
        return M.f32(rng.choice([0.0, -0.0, 1.5, -2.25, float("nan"), 3.0]))
    return rng.randrange(-6, 7)


def fuzz_filter(rng, build_names, probe_names):
    """a comparison between a build and a probe channel of one type, or between arithmetic over two BIGINT channels; AND / OR of two"""
    nb = len(build_names)
    def leaf():
        pairs = [(j, i) for j, bn in enumerate(build_names) for i, pn in enumerate(probe_names) if bn == pn]
        j, i = rng.choice(pairs)
        t = M.TYPES[build_names[j]]
        b, p = field(j, t), field(nb + i, t)
        op = rng.choice([abi.OP_EQUAL, abi.OP_NOT_EQUAL, abi.OP_LESS_THAN, abi.OP_LESS_THAN_OR_EQUAL, abi.OP_GREATER_THAN, abi.OP_GREATER_THAN_OR_EQUAL])
        if build_names[j] == "BIGINT" and rng.random() < 0.5:
            arith = rng.choice([abi.OP_ADD, abi.OP_SUBTRACT, abi.OP_MULTIPLY, abi.OP_DIVIDE, abi.OP_MODULUS])
            return call(op, abi.BOOLEAN, call(arith, abi.BIGINT, p, b), constant(rng.randrange(-3, 4), abi.BIGINT))
        return call(op, abi.BOOLEAN, p, b) if rng.random() < 0.5 else call(op, abi.BOOLEAN, b, p)
    shape = rng.randrange(3)
    return leaf() if shape == 0 else (and_ if shape == 1 else or_)(leaf(), leaf())


@pytest.mark.parametrize("seed", list(range(FUZZ_SEEDS)))
def test_fuzz(gpu, monkeypatch, seed):
    rng = random.Random(1000 + seed)
    shared = rng.choice(FUZZ_TYPES)
    build_names = [shared, "BIGINT"] + [rng.choice(FUZZ_TYPES) for _ in range(rng.randrange(2))]
    probe_names = ["BIGINT", shared] + [rng.choice(FUZZ_TYPES) for _ in range(rng.randrange(2))]
    n, m = rng.choice([(rng.randrange(1, 2000), rng.randrange(0, 12)), (rng.randrange(1, 60), rng.randrange(0, 300)), (2000, 30), (200, 300)])
    null_rate = rng.choice([0.0, 0.1, 0.5])
    row = lambda names: tuple(None if rng.random() < null_rate else fuzz_value(rng, t) for t in names)
    probe, build = [row(probe_names) for _ in range(n)], [row(build_names) for _ in range(m)]
    f = fuzz_filter(rng, build_names, probe_names) if rng.random() < 0.9 else None
    cuts = lambda k: sorted(rng.sample(range(k + 1), min(k, rng.randrange(4))))
    kind, result = NL.outcome(probe, build, [0], [0], f)
    if kind == "rows":
        check_join(monkeypatch, probe_names, probe, build_names, build, list(range(len(probe_names))), list(range(len(build_names))), f, cuts(n), cuts(m))
        return
    # the product raises: some get_output of the first probe page that holds a raising pair reports the model's status
    bridge, builder = build_side(build_names, pages_of(build_names, build))
    for variant in VARIANTS:
        monkeypatch.setenv("PRESTO_AMD_NL_VARIANT", variant)
        join = NestedLoopJoinOperator(bridge, M.input_types(probe_names), [0], [0], filter=f)
        with pytest.raises(PrestoAmdError) as e:
            drain(join, pages_of(probe_names, probe)[0])
        assert e.value.status == result      # (the operands are small: a zero divisor is the only error these filters can raise)
        join.close()
    builder.close()
    bridge.destroy()


# ---- an equivalence that needs no model -------------------------------------------------------------------------------------------------
def test_equals_a_lookup_join_over_unique_keys(gpu, monkeypatch):
    """b.k = p.k over unique build keys: the rows of LookupJoinOperator on the same pages, in the same order"""
    rng = random.Random(5)
    build_keys = rng.sample(range(0, 3000), 700)
    build = [(k, float(k) / 4) for k in build_keys]
    probe = [(rng.randrange(0, 3000) if rng.random() > 0.05 else None, i) for i in range(1500)]
    build_pages, probe_pages = pages_of(["BIGINT", "DOUBLE"], build, [300]), pages_of(["BIGINT", "BIGINT"], probe, [400, 900])
    ls = LookupSourceFactory()
    hb = HashBuilderOperator(ls, [abi.BIGINT, abi.DOUBLE], [0], [1, 0])
    to_pages(hb, build_pages)
    lj = LookupJoinOperator(ls, [abi.BIGINT, abi.BIGINT], [0], [1, 0])
    want = [r for p in probe_pages for out in drain(lj, p) for r in out.to_rows()]
    assert len(want) > 100
    bridge, builder = build_side(["BIGINT", "DOUBLE"], build_pages)
    f = eq(field(0, abi.BIGINT), field(2, abi.BIGINT))
    for variant in VARIANTS:
        out = join_pages(bridge, ["BIGINT", "BIGINT"], probe_pages, [1, 0], [1, 0], f, variant, monkeypatch)
        assert [r for p in out for r in p.to_rows()] == want, variant
    for op in (lj, hb, builder):
        op.close()
    bridge.destroy()


# ---- the C++ mirror (include/presto_amd.hpp) ---------------------------------------------------------------------------------------
def test_cpp_mirror(gpu):
    """tests/cpp/test_nested_loop.cpp: a VARCHAR build column with a filter, and the builder -> bridge -> join order, through runDriver."""
    exe = os.path.join(ROOT, "tests", "cpp", "test_nested_loop")
    src = exe + ".cpp"
    deps = [src, os.path.join(ROOT, "include", "presto_amd.hpp"), os.path.join(ROOT, "include", "presto_amd.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(exe) < os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-L" + os.path.join(ROOT, "presto_amd"),
                               "-lpresto_amd", "-Wl,-rpath,$ORIGIN/../../presto_amd", "-Wl,--allow-shlib-undefined", "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode == 0, r.stdout.decode()[-2000:]
    assert "nested loop ok" in r.stdout.decode()
