"""Block.copyPositions of a VARCHAR channel through every operator that gathers rows by position: FilterAndProject, LookupJoin (inner and
probe-outer), LookupOuter, DistinctLimit, RowNumber with a cap, TopN, OrderBy and TopNRanking.

One VARCHAR column whose values cycle through NULL and the byte lengths 0, 1, 7, 8, 9, 15, 16, 17 and 33 (the byte copy moves 8 bytes at a
time: it turns over at 8 and 16), a BIGINT row id beside it.  Every position list P is expressed through an operator's own semantics -- a
flag channel, probe keys, unvisited build rows, first occurrences, a cap, sort keys -- and the expected output is plain Python indexing:
[rows[p] for p in P], a row of NULLs for a -1.  The lists hold 1, 1023, 1024, 1025 and (the small scan's limit + 1) positions: the
exclusive scan of the lengths takes its single-tile, small and tiled path.  Host and device input, host and device output.
Nothing here knows how the library gathers: the file passes on any build of it (PRESTO_AMD_LIB).
"""
import os
import re

import pytest

from presto_amd import abi
from presto_amd.expr import field
from presto_amd.operators import (DistinctLimitOperator, FilterAndProjectOperator, HashBuilderOperator, LookupJoinOperator, LookupOuterOperator,
                                  LookupSourceFactory, OrderByOperator, RowNumberOperator, TopNOperator, TopNRankingOperator, download_page, to_pages,
                                  upload_page)
from presto_amd.page import Block, DeviceBuffer, Page

on_gpu = pytest.mark.gpu
ASC = abi.ASC_NULLS_LAST
VARCHAR, BIGINT = abi.VARCHAR, abi.BIGINT
LENGTHS = [None, 0, 1, 7, 8, 9, 15, 16, 17, 33]
BUILD_ROWS = 257


def small_scan_max():
    """kSmallScanMax of csrc/scan_kernels.hip: the longest scan its one-workgroup kernel takes."""
    text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "presto_amd", "csrc", "scan_kernels.hip")).read()
    items = int(re.search(r"kSmallScanItems\s*=\s*(\d+)\s*;", text).group(1))
    return int(re.search(r"kSmallScanMax\s*=\s*(\d+)\s*\*\s*kSmallScanItems\s*;", text).group(1)) * items


COUNTS = [1, 1023, 1024, 1025, small_scan_max() + 1]
INPUTS = ["host_pages", "device_pages"]
OUTPUTS = [pytest.param(abi.MEM_HOST, id="host_output"), pytest.param(abi.MEM_DEVICE, id="device_output")]
DEVICE_OUTPUT = [pytest.param(abi.MEM_DEVICE, id="device_output")]


# ---- the column, the position lists and the expected rows: plain Python ------------------------------------------------------------------------
def string(i):
    length = LENGTHS[i % len(LENGTHS)]
    return None if length is None else bytes((i * 131 + j * 7) % 256 for j in range(length))


def spread(k):
    """k ascending positions with gaps, the first of them 0, and the row count of the input they index (its last row is not among them)."""
    positions = [0] + [i for i in range(1, 3 * k) if i % 3 != 0][:k - 1]
    return positions, positions[-1] + 2


def permutation(k):
    step = next(a for a in (7, 11, 13, 5, 3) if k % a != 0)
    return [(j * step + 2) % k for j in range(k)]


def plan_filter_project(k):
    """[VARCHAR, id, flag]: the filter is flag = 1"""
    positions, n = spread(k)
    chosen = set(positions)
    rows = [(string(i), i, 1 if i in chosen else 0) for i in range(n)]
    return rows, [rows[p][:2] for p in positions]


def plan_join(k, outer):
    """build [VARCHAR, id], probe [key, VARCHAR]: the probe keys are the positions -- descending, repeated when k > BUILD_ROWS --; with
    `outer` every fifth key is absent from the build side (position -1: that output row has a NULL build side)"""
    build = [(string(i), i) for i in range(BUILD_ROWS)]
    positions = [-1 if outer and j % 5 == 2 else (BUILD_ROWS - 1 - 3 * j) % BUILD_ROWS for j in range(k)]
    probe = [(p if p >= 0 else 1000 + j, string(j + 3)) for j, p in enumerate(positions)]
    return build, probe, [probe[j] + (build[p] if p >= 0 else (None, None)) for j, p in enumerate(positions)]


def plan_lookup_outer(k):
    """the positions are the build rows no probe key visits"""
    positions, n = spread(k)
    build = [(string(i), i) for i in range(n)]
    probe = [(i, string(i + 3)) for i in sorted(set(range(n)) - set(positions))]
    return build, probe, [(None, None) + build[p] for p in positions]


def plan_distinct_limit(k):
    """[VARCHAR, id], both distinct channels: a row outside the positions repeats row 0"""
    positions, n = spread(k)
    chosen = set(positions)
    rows = [(string(i), i) if i in chosen else (string(0), 0) for i in range(n)]
    return rows, [rows[p] for p in positions]


def plan_row_number(k):
    """[VARCHAR, id, partition] under a cap of 1: a row outside the positions is a later row of row 0's partition"""
    positions, n = spread(k)
    chosen = set(positions)
    rows = [(string(i), i, i if i in chosen else 0) for i in range(n)]
    return rows, [rows[p][:2] + (1,) for p in positions]


def plan_topn(k):
    """[VARCHAR, id], the k smallest ids: they sit at the positions, descending"""
    positions, n = spread(k)
    rank = {p: k - 1 - j for j, p in enumerate(positions)}
    rows = [(string(i), rank.get(i, k + i)) for i in range(n)]
    return rows, [rows[p] for p in reversed(positions)]


def plan_order_by(k):
    """[VARCHAR, id, sort key]: the sort key of row P[j] is j"""
    positions = permutation(k)
    place = {p: j for j, p in enumerate(positions)}
    rows = [(string(i), i, place[i]) for i in range(k)]
    return rows, [rows[p][:2] for p in positions]


def plan_topn_ranking(k):
    """[VARCHAR, id, partition, sort key], one partition, row_number() <= k: the survivors sit at the positions, descending"""
    positions, n = spread(k)
    rank = {p: k - 1 - j for j, p in enumerate(positions)}
    rows = [(string(i), i, 7, rank.get(i, k + i)) for i in range(n)]
    return rows, [rows[p][:2] + (j + 1,) for j, p in enumerate(reversed(positions))]


def test_the_model_reproduces_the_known_answers():
    """(the column, the position lists and the expected rows against rows written out by hand: no GPU work)"""
    assert [None if string(i) is None else len(string(i)) for i in range(10)] == LENGTHS and string(10) is None and string(11) == b""
    assert string(2) == b"\x06" and string(4) == bytes([12, 19, 26, 33, 40, 47, 54, 61]) and string(12) == b"$"
    assert spread(1) == ([0], 2) and spread(4) == ([0, 1, 2, 4], 6)
    assert permutation(1) == [0] and permutation(5) == [2, 4, 1, 3, 0] and sorted(permutation(1025)) == list(range(1025))
    rows, expected = plan_filter_project(4)
    assert [r[2] for r in rows] == [1, 1, 1, 0, 1, 0]
    assert expected == [(None, 0), (b"", 1), (b"\x06", 2), (bytes([12, 19, 26, 33, 40, 47, 54, 61]), 4)]
    build, probe, expected = plan_join(4, outer=True)
    assert [r[0] for r in probe] == [256, 253, 1002, 247] and len(build) == 257
    assert expected[0] == (256, string(3), string(256), 256) and expected[2] == (1002, string(5), None, None) and len(string(256)) == 15
    assert plan_join(300, outer=False)[1][257][0] == plan_join(300, outer=False)[1][0][0] == 256   # (a repeated position)
    build, probe, expected = plan_lookup_outer(4)
    assert [r[0] for r in probe] == [3, 5] and expected == [(None, None, None, 0), (None, None, b"", 1), (None, None, b"\x06", 2), (None, None, string(4), 4)]
    assert plan_distinct_limit(2) == ([(None, 0), (b"", 1), (None, 0)], [(None, 0), (b"", 1)])
    assert plan_row_number(2) == ([(None, 0, 0), (b"", 1, 1), (b"\x06", 2, 0)], [(None, 0, 1), (b"", 1, 1)])
    assert plan_topn(2) == ([(None, 1), (b"", 0), (b"\x06", 4)], [(b"", 0), (None, 1)])
    assert [r[1] for r in plan_order_by(5)[1]] == [2, 4, 1, 3, 0] and [r[2] for r in plan_order_by(5)[0]] == [4, 2, 0, 3, 1]
    assert plan_topn_ranking(2) == ([(None, 0, 7, 1), (b"", 1, 7, 0), (b"\x06", 2, 7, 4)], [(b"", 1, 1), (None, 0, 2)])
    assert COUNTS == [1, 1023, 1024, 1025, 16385]


# ---- pages in, rows out -----------------------------------------------------------------------------------------------------------------------
def page_of(types, rows):
    blocks = []
    for c, t in enumerate(types):
        values = [r[c] for r in rows]
        if t == VARCHAR:
            blocks.append(Block.varchar(values))
        else:
            blocks.append(Block.bigint([0 if v is None else v for v in values], [v is None for v in values] if None in values else None))
    return Page(blocks, len(rows))


def region(page, lo, n):
    """Page.getRegion: rows [lo, lo + n) of a page, its arrays read where they are (a VARCHAR block's first offset is then not 0)."""
    if page.mem == abi.MEM_HOST:
        return page.get_region(lo, n)
    blocks = []
    for b in page.blocks:
        nulls = DeviceBuffer(b.nulls.ptr + lo, n, b.nulls) if b.nulls is not None else None
        if b.encoding == abi.VARWIDTH:
            blocks.append(Block(b.type, abi.VARWIDTH, n, values=b.values, offsets=DeviceBuffer(b.offsets.ptr + 4 * lo, 4 * (n + 1), b.offsets), nulls=nulls))
        else:
            w = abi.TYPE_WIDTH[b.type]
            blocks.append(Block(b.type, abi.FLAT, n, values=DeviceBuffer(b.values.ptr + w * lo, w * n, b.values), nulls=nulls))
    return Page(blocks, n, abi.MEM_DEVICE)


def place(page, input_mem):
    return upload_page(page) if input_mem == "device_pages" else page


def drain(op, pages):
    """The operator over the pages -> its output rows (every output page is read before the operator goes on)."""
    rows = []

    def take():
        page = op.getOutput()
        if page is not None:
            rows.extend((download_page(page) if page.mem == abi.MEM_DEVICE else page).to_rows())
        return page is not None
    for page in pages:
        if not op.needsInput():   # (DistinctLimit has its limit)
            break
        op.addInput(page)
        while take():
            pass
    op.finish()
    for _ in range(1000):
        if op.isFinished():
            break
        take()
    assert op.isFinished()
    op.close()
    return rows


def build_side(build_rows, input_mem):
    bridge = LookupSourceFactory()
    page = page_of([VARCHAR, BIGINT], build_rows)
    cut = len(build_rows) // 3
    to_pages(HashBuilderOperator(bridge, [VARCHAR, BIGINT], [1], [0, 1]), [place(p, input_mem) for p in (page.get_region(0, cut), page.get_region(cut, len(build_rows) - cut)) if p.position_count])
    return bridge


# ---- the sites ------------------------------------------------------------------------------------------------------------------------------
@on_gpu
@pytest.mark.parametrize("k", COUNTS)
@pytest.mark.parametrize("input_mem", INPUTS)
@pytest.mark.parametrize("output_mem", OUTPUTS)
def test_filter_and_project(gpu, k, input_mem, output_mem):
    rows, expected = plan_filter_project(k)
    op = FilterAndProjectOperator([VARCHAR, BIGINT, BIGINT], field(2, BIGINT).eq(1), [field(0, VARCHAR), field(1, BIGINT)], output_mem=output_mem)
    assert drain(op, [place(page_of([VARCHAR, BIGINT, BIGINT], rows), input_mem)]) == expected


@on_gpu
@pytest.mark.parametrize("k", [1, 1025])
@pytest.mark.parametrize("input_mem", INPUTS)
@pytest.mark.parametrize("output_mem", OUTPUTS)
def test_filter_and_project_over_a_region_of_a_page(gpu, k, input_mem, output_mem):
    """the page is rows [5, 5 + n) of a larger one: its first VARCHAR offset is not 0"""
    rows, expected = plan_filter_project(k)
    larger = page_of([VARCHAR, BIGINT, BIGINT], [(b"before the region", -1, 1)] * 5 + rows + [(b"behind it", -2, 1)])
    assert int(larger.get_region(5, len(rows)).blocks[0].offsets[0]) == 5 * 17
    op = FilterAndProjectOperator([VARCHAR, BIGINT, BIGINT], field(2, BIGINT).eq(1), [field(0, VARCHAR), field(1, BIGINT)], output_mem=output_mem)
    assert drain(op, [region(place(larger, input_mem), 5, len(rows))]) == expected


@on_gpu
@pytest.mark.parametrize("k", COUNTS)
@pytest.mark.parametrize("join_type", [abi.JOIN_INNER, abi.JOIN_PROBE_OUTER], ids=["inner", "probe_outer"])
@pytest.mark.parametrize("input_mem", INPUTS)
@pytest.mark.parametrize("output_mem", OUTPUTS)
def test_lookup_join(gpu, k, join_type, input_mem, output_mem):
    build, probe, expected = plan_join(k, outer=join_type == abi.JOIN_PROBE_OUTER)
    bridge = build_side(build, input_mem)
    join = LookupJoinOperator(bridge, [BIGINT, VARCHAR], [0], [0, 1], output_mem=output_mem, join_type=join_type)
    assert drain(join, [place(page_of([BIGINT, VARCHAR], probe), input_mem)]) == expected


@on_gpu
@pytest.mark.parametrize("k", COUNTS)
@pytest.mark.parametrize("input_mem", INPUTS)
@pytest.mark.parametrize("output_mem", OUTPUTS)
def test_lookup_outer(gpu, k, input_mem, output_mem):
    build, probe, expected = plan_lookup_outer(k)
    bridge = build_side(build, input_mem)
    join = LookupJoinOperator(bridge, [BIGINT, VARCHAR], [0], [0, 1], output_mem=output_mem, join_type=abi.JOIN_LOOKUP_OUTER)
    joined = drain(join, [place(page_of([BIGINT, VARCHAR], probe), input_mem)])
    assert joined == [p + build[p[0]] for p in probe]
    outer = LookupOuterOperator(bridge, [BIGINT, VARCHAR], [0, 1], join_type=abi.JOIN_LOOKUP_OUTER, output_mem=output_mem)
    assert drain(outer, []) == expected


@on_gpu
@pytest.mark.parametrize("k", COUNTS)
@pytest.mark.parametrize("input_mem", INPUTS)
@pytest.mark.parametrize("output_mem", DEVICE_OUTPUT)
def test_distinct_limit(gpu, k, input_mem, output_mem):
    rows, expected = plan_distinct_limit(k)
    op = DistinctLimitOperator([VARCHAR, BIGINT], [0, 1], k, output_mem=output_mem)
    assert drain(op, [place(page_of([VARCHAR, BIGINT], rows), input_mem)]) == expected


@on_gpu
@pytest.mark.parametrize("k", COUNTS)
@pytest.mark.parametrize("input_mem", INPUTS)
@pytest.mark.parametrize("output_mem", DEVICE_OUTPUT)
def test_row_number_with_a_cap(gpu, k, input_mem, output_mem):
    rows, expected = plan_row_number(k)
    op = RowNumberOperator([VARCHAR, BIGINT, BIGINT], [0, 1], [2], 1, output_mem=output_mem)
    assert drain(op, [place(page_of([VARCHAR, BIGINT, BIGINT], rows), input_mem)]) == expected


@on_gpu
@pytest.mark.parametrize("k", COUNTS)
@pytest.mark.parametrize("input_mem", INPUTS)
@pytest.mark.parametrize("output_mem", DEVICE_OUTPUT)
def test_topn(gpu, k, input_mem, output_mem):
    rows, expected = plan_topn(k)
    op = TopNOperator([VARCHAR, BIGINT], k, [1], [ASC], output_mem)
    assert drain(op, [place(page_of([VARCHAR, BIGINT], rows), input_mem)]) == expected


@on_gpu
@pytest.mark.parametrize("k", COUNTS)
@pytest.mark.parametrize("input_mem", INPUTS)
@pytest.mark.parametrize("output_mem", DEVICE_OUTPUT)
def test_order_by(gpu, k, input_mem, output_mem):
    rows, expected = plan_order_by(k)
    op = OrderByOperator([VARCHAR, BIGINT, BIGINT], [0, 1], [2], [ASC], output_mem)
    assert drain(op, [place(page_of([VARCHAR, BIGINT, BIGINT], rows), input_mem)]) == expected


@on_gpu
@pytest.mark.parametrize("k", COUNTS)
@pytest.mark.parametrize("input_mem", INPUTS)
@pytest.mark.parametrize("output_mem", DEVICE_OUTPUT)
def test_topn_ranking_survivors_and_prune(gpu, k, input_mem, output_mem, monkeypatch):
    """every row but the last in the first page, with a prune threshold of 4 rows: the rows held are pruned behind it and behind the second"""
    monkeypatch.setenv("PRESTO_AMD_TOPN_RANKING_PRUNE_ROWS", "4")
    rows, expected = plan_topn_ranking(k)
    types = [VARCHAR, BIGINT, BIGINT, BIGINT]
    op = TopNRankingOperator(types, [0, 1], [2], [3], [ASC], k, output_mem=output_mem)
    assert drain(op, [place(page_of(types, part), input_mem) for part in (rows[:-1], rows[-1:])]) == expected
