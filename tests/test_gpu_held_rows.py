"""The seams of the store that operators collect rows in page by page (csrc/held_rows.hpp), with tiny inputs: pages that bring their
first NULL late, a page without rows, VARCHAR pages that add no bytes or start in the middle of a larger block, more output channels than
one gather launch takes, OrderBy's two ways round the gather, and TopNRanking's prune between pages.  Its users: OrderBy, Window and
TopNRanking (their input), HashBuilder (the build rows of a join: `hash_build`), LookupJoin (a probe page that comes out as several:
`kept_probe`) and FilterAndProject's MergePages buffer (`merge_pages`).

Every case is compared bit for bit (a float as its 8 bytes) with a plain Python model over Page.to_rows(): a stable `sorted`, a join
written as two loops, MergePages as a list that is flushed.  Channel 0 is a BIGINT key without NULLs -- OrderBy's first sort channel, the
partition channel of Window and TopNRanking, the join key -- and channel 1 an INTEGER sort channel with ties, so that arrival order shows.
The operators run over host pages and over device pages, into host and device output.
Nothing here knows how the library stores the rows: the file passes on any build of it (PRESTO_AMD_LIB).  One thing the join model does
take from the operator's contract (op_join.cpp's head comment, the reference's PagesHash position links): the matches of a probe row come
out latest build arrival first.  Every build side here is far below the size at which the builder changes its table build.
"""
import ctypes
import struct

import pytest

from presto_amd import abi
from presto_amd._lib import lib
from presto_amd.expr import constant, field
from presto_amd.operators import (FilterAndProjectOperator, FusedJoinOperator, HashBuilderOperator, LookupJoinOperator, LookupOuterOperator,
                                  LookupSourceFactory, OrderByOperator, TopNRankingOperator, WindowOperator, download_page, upload_page)
from presto_amd.page import Block, DeviceBuffer, Page

on_gpu = pytest.mark.gpu
ASC = abi.ASC_NULLS_LAST
LIMIT = 3
KINDS = ["order_by", "window", "topn_row_number", "topn_rank"]
kinds_and_memories = [pytest.mark.parametrize("kind", KINDS), pytest.mark.parametrize("input_mem", ["host_pages", "device_pages"]),
                      pytest.mark.parametrize("output_mem", [abi.MEM_HOST, abi.MEM_DEVICE], ids=["host_output", "device_output"])]
NAN, LONG = float("nan"), abi.decimal(38, 2)


def with_kinds_and_memories(test):
    for mark in kinds_and_memories:
        test = mark(test)
    return on_gpu(test)


def create(kind, types, output_mem):
    out = list(range(len(types)))
    if kind == "order_by":
        return OrderByOperator(types, out, [0, 1], [ASC, ASC], output_mem)
    if kind == "window":
        return WindowOperator(types, out, [abi.WINDOW_ROW_NUMBER], [0], [1], [ASC], output_mem=output_mem)
    ranking = abi.RANKING_RANK if kind == "topn_rank" else abi.RANKING_ROW_NUMBER
    return TopNRankingOperator(types, out, [0], [1], [ASC], LIMIT, ranking_type=ranking, output_mem=output_mem)


def model(kind, rows):
    """What the operator of `kind` gives for the input rows in arrival order."""
    if kind == "order_by":
        return sorted(rows, key=lambda r: (r[0], r[1]))
    out = []
    if kind == "window":   # partitions ascending, row_number() behind the channels
        place = {}
        for r in sorted(rows, key=lambda r: (r[0], r[1])):
            place[r[0]] = place.get(r[0], 0) + 1
            out.append(r + (place[r[0]],))
        return out
    for key in dict.fromkeys(r[0] for r in rows):   # partitions in first-seen order
        part = sorted((r for r in rows if r[0] == key), key=lambda r: r[1])
        for i, r in enumerate(part):
            ranking = i + 1 if kind == "topn_row_number" else 1 + sum(1 for o in part if o[1] < r[1])
            if ranking <= LIMIT:
                out.append(r + (ranking,))
    return out


def bits(rows):
    return [tuple(struct.pack("<d", v) if isinstance(v, float) else v for v in r) for r in rows]


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


def run(kind, types, host_pages, input_mem, output_mem, regions=None, after_page=None):
    """The operator over the pages (regions: {page index: (lo, n)} -- only those rows of the page are fed, as a region of it) -> its
    output rows, and the input rows it was given."""
    regions = regions or {}
    op = create(kind, types, output_mem)
    rows = []
    for i, host in enumerate(host_pages):
        page = upload_page(host) if input_mem == "device_pages" else host
        if i in regions:
            page, host = region(page, *regions[i]), host.get_region(*regions[i])
        rows += host.to_rows()
        assert op.needsInput()
        op.addInput(page)   # (also a page without rows: Driver.java never hands one over, other hosts of the library may)
        assert op.getOutput() is None
        if after_page:
            after_page(op, rows)
    op.finish()
    got = []
    while not op.isFinished():
        page = op.getOutput()
        if page is not None:
            got += (download_page(page) if page.mem == abi.MEM_DEVICE else page).to_rows()
    op.close()
    return got, rows


def check(kind, types, host_pages, input_mem, output_mem, **kw):
    got, rows = run(kind, types, host_pages, input_mem, output_mem, **kw)
    expected = model(kind, rows)
    assert len(expected) > 0 and bits(got) == bits(expected)
    return got


# ---- late NULLs and a page without rows -----------------------------------------------------------------------------------------------------
LATE_TYPES = [abi.BIGINT, abi.INTEGER, abi.VARCHAR, abi.DOUBLE, abi.BOOLEAN]


def late_null_pages():
    """5, 0, 1 and 7 rows.  The first and the last page carry no NULL arrays; the one-row page is NULL in every channel but the two that
    order the rows: the rows held before it get their flags then.  Partition 1 holds four rows after the first page."""
    def page(keys, seq, strings, doubles, booleans):
        return Page([Block.bigint(keys), Block.integer(seq), Block.varchar(strings), Block.double(doubles, [v is None for v in doubles]),
                     Block.boolean([bool(v) for v in booleans], [v is None for v in booleans])], len(keys))
    pages = [page([1, 1, 2, 1, 1], [5, 3, 7, 3, 1], [b"apple", b"", b"kiwi", b"fig", b"banana"], [1.5, -0.0, NAN, 2.5, 0.0], [True, False, True, False, True]),
             page([], [], [], [], []),
             page([2], [2], [None], [None], [None]),
             page([3, 2, 1, 3, 2, 3, 3], [4, 7, 2, 4, 1, 9, 4], [b"plum", b"a longer string than eight bytes", b"", b"pear", b"lime", b"\xff\x00", b"date"],
                  [-1.5, NAN, 5e-324, -0.0, 0.0, float("inf"), 3.0], [False, True, True, False, False, True, True])]
    assert [p.position_count for p in pages] == [5, 0, 1, 7]
    assert all(b.nulls is None for p in (pages[0], pages[3]) for b in p.blocks) and all(b.nulls is not None for b in pages[2].blocks[2:])
    return pages


@with_kinds_and_memories
def test_late_nulls_and_a_page_without_rows(gpu, kind, input_mem, output_mem):
    got = check(kind, LATE_TYPES, late_null_pages(), input_mem, output_mem)
    assert sum(1 for r in got if r[2] is None and r[3] is None and r[4] is None) == 1   # (the row of NULLs is among the rows of every result)


# ---- VARCHAR edges ----------------------------------------------------------------------------------------------------------------------------
VARCHAR_TYPES = [abi.BIGINT, abi.INTEGER, abi.VARCHAR]


def varchar_edge_pages():
    def page(keys, seq, strings):
        return Page([Block.bigint(keys), Block.integer(seq), Block.varchar(strings)], len(keys))
    larger = page([1, 2, 1, 2, 1, 2, 1], [9, 8, 7, 6, 5, 4, 3], [b"zero", b"one", b"", b"three", b"four", None, b"six6six6six"])
    return [larger,                                                    # fed as its rows [1, 3): the first page, first offset 4
            page([1, 2, 2], [2, 2, 1], [b"", b"x", b"yz"]),             # an empty string among others
            page([1, 2], [1, 3], [None, None]),                        # every string NULL: no bytes
            page([2, 1, 1], [5, 6, 4], [b"", b"", b""]),                # every string empty: no bytes
            larger]                                                    # fed as its rows [3, 7): behind held rows, first offset 7


@with_kinds_and_memories
def test_varchar_pages_that_add_no_bytes_or_start_inside_a_block(gpu, kind, input_mem, output_mem):
    pages = varchar_edge_pages()
    assert int(pages[2].blocks[2].offsets[-1]) == 0 and int(pages[3].blocks[2].offsets[-1]) == 0
    assert int(pages[0].get_region(1, 2).blocks[2].offsets[0]) == 4 and int(pages[4].get_region(3, 4).blocks[2].offsets[0]) == 7
    check(kind, VARCHAR_TYPES, pages, input_mem, output_mem, regions={0: (1, 2), 4: (3, 4)})


# ---- more output channels than one gather launch takes ----------------------------------------------------------------------------------------
def wide_pages(kind):
    """26 channels, all output: the two ordering channels, then BOOLEAN, INTEGER, DOUBLE and a 16-byte LONG_DECIMAL (TopNRanking refuses
    it: BIGINT there) in turn, every third of them with NULLs (each type both ways).  9 rows in pages of 5 and 4."""
    wide = abi.BIGINT if kind.startswith("topn") else LONG
    types = [abi.BIGINT, abi.INTEGER] + [(abi.BOOLEAN, abi.INTEGER, abi.DOUBLE, wide)[c % 4] for c in range(24)]
    keys, seq = [2, 1, 2, 1, 1, 2, 1, 2, 1], [3, 3, 1, 3, 2, 1, 9, 0, 1]

    def column(c, t, lo, hi):
        values = [(c + 1) * 1000 + i for i in range(lo, hi)]
        nulls = [(i + c) % 3 == 0 for i in range(lo, hi)] if c % 3 == 0 else None
        if t == abi.BOOLEAN:
            return Block.boolean([v % 2 == 0 for v in values], nulls)
        if t == abi.DOUBLE:
            return Block.double([v / 8.0 if v % 5 else -0.0 for v in values], nulls)
        if t == LONG:
            return Block.long_decimal([None if nulls and nulls[i] else (-1) ** v * (v << 70 | v) for i, v in enumerate(values)])
        return Block.flat(t, [-v if v % 2 else v for v in values], nulls)

    def page(lo, hi):
        return Page([Block.bigint(keys[lo:hi]), Block.integer(seq[lo:hi])] + [column(c, t, lo, hi) for c, t in enumerate(types[2:])], hi - lo)
    return types, [page(0, 5), page(5, 9)]


@with_kinds_and_memories
def test_26_output_channels(gpu, kind, input_mem, output_mem):
    types, pages = wide_pages(kind)
    assert len(types) == 26 and {abi.TYPE_WIDTH[t] for t in types} == ({1, 4, 8} if kind.startswith("topn") else {1, 4, 8, 16})
    assert any(b.nulls is not None for b in pages[0].blocks) and any(b.nulls is None for b in pages[0].blocks)
    check(kind, types, pages, input_mem, output_mem)


# ---- OrderBy: the channels that do not go through the gather ----------------------------------------------------------------------------------
@on_gpu
@pytest.mark.parametrize("input_mem", ["host_pages", "device_pages"])
@pytest.mark.parametrize("output_mem", [abi.MEM_HOST, abi.MEM_DEVICE], ids=["host_output", "device_output"])
def test_order_by_shortcuts_beside_the_gather(gpu, input_mem, output_mem, monkeypatch):
    """One sort channel, BIGINT without NULLs and an output channel (written from the sorted images); an 8-byte and a 4-byte channel without
    NULLs (they may ride along with the sort); a nullable channel and a VARCHAR channel (gathered).  With and without the riding payload."""
    types = [abi.BIGINT, abi.DOUBLE, abi.INTEGER, abi.DOUBLE, abi.VARCHAR]
    pages = [Page([Block.bigint([5, 3, 5, 1, 9]), Block.double([0.5, -0.0, NAN, 4.0, -2.0]), Block.integer([10, -11, 12, -13, 14]),
                   Block.double([1.0, 0.0, 3.0, 0.0, 5.0], [0, 1, 0, 0, 0]), Block.varchar([b"e", b"", None, b"abcdefghi", b"a"])], 5),
             Page([Block.bigint([3, -7, 5]), Block.double([6.0, 7.0, 8.0]), Block.integer([15, 16, -17]), Block.double([6.5, 7.5, 8.5]),
                   Block.varchar([b"tie of 3", b"first", b"tie of 5"])], 3)]
    rows = [r for p in pages for r in p.to_rows()]
    expected = sorted(rows, key=lambda r: r[0])
    assert len(rows) == 8
    results = []
    for no_payload in (False, True):
        if no_payload:
            monkeypatch.setenv("PRESTO_AMD_SORT_NO_PAYLOAD", "1")
        else:
            monkeypatch.delenv("PRESTO_AMD_SORT_NO_PAYLOAD", raising=False)
        op = OrderByOperator(types, [0, 1, 2, 3, 4], [0], [ASC], output_mem)
        op_pages = [upload_page(p) for p in pages] if input_mem == "device_pages" else pages
        for p in op_pages:
            op.addInput(p)
        op.finish()
        page = op.getOutput()
        results.append(bits((download_page(page) if page.mem == abi.MEM_DEVICE else page).to_rows()))
        assert op.getOutput() is None and op.isFinished()
        op.close()
    assert results[0] == results[1] == bits(expected)


# ---- TopNRanking: a prune between the pages -----------------------------------------------------------------------------------------------------
@on_gpu
@pytest.mark.parametrize("kind", ["topn_row_number", "topn_rank"])
@pytest.mark.parametrize("input_mem", ["host_pages", "device_pages"])
@pytest.mark.parametrize("output_mem", [abi.MEM_HOST, abi.MEM_DEVICE], ids=["host_output", "device_output"])
def test_topn_ranking_prunes_between_pages(gpu, kind, input_mem, output_mem, monkeypatch):
    """A prune threshold of 4 rows: the first page (5 rows) is pruned when it has been appended, and drops a row with a non-empty string.
    The rows of the later pages land behind the rows kept; the last page reaches the threshold again."""
    monkeypatch.setenv("PRESTO_AMD_TOPN_RANKING_PRUNE_ROWS", "4")
    held = []

    def after_page(op, rows):
        held.append((op.topNRankingStats()[2], len(rows)))
    got, rows = run(kind, LATE_TYPES, late_null_pages(), input_mem, output_mem, after_page=after_page)
    first = model(kind, rows[:5])
    assert len(first) < 5 and sum(len(r[2]) for r in first) < sum(len(r[2]) for r in rows[:5])
    # the rows held after a page: what the prune of the first page kept, one more row, then no more than survive in the end can be told
    # without knowing when the last prune ran -- only that the rows of the result are among them
    assert held[0] == (len(first), 5) and held[1] == (len(first), 5) and held[2] == (len(first) + 1, 6)
    assert len(model(kind, rows)) <= held[3][0] <= len(first) + 1 + 7
    assert bits(got) == bits(model(kind, rows))


# ---- hash_build: the pages above as the build side of a join ---------------------------------------------------------------------------------
PROBE_KEYS = [1, 2, 3, 99]   # (99: a miss in every build side below)


def drain(op, pages, after_first_output=None):
    """Driver order: a page in, then getOutput until the operator wants the next; finish; the rest.  Device output is read at once: its
    buffers are the operator's again with its next call."""
    rows, seen = [], 0

    def take(page):
        nonlocal seen
        if page is not None:
            rows.extend((download_page(page) if page.mem == abi.MEM_DEVICE else page).to_rows())
            seen += 1
            if seen == 1 and after_first_output:
                after_first_output()
    for p in pages:
        assert op.needsInput()
        op.addInput(p)
        for _ in range(64):
            page = op.getOutput()
            take(page)
            if page is None and op.needsInput():
                break
    op.finish()
    for _ in range(64):
        if op.isFinished():
            break
        take(op.getOutput())
    assert op.isFinished()
    return rows


def feed(host_pages, input_mem, regions=None):
    """The pages as the operator gets them (regions as in run) and the rows they hold, in arrival order."""
    pages, rows = [], []
    for i, host in enumerate(host_pages):
        page = upload_page(host) if input_mem == "device_pages" else host
        if regions and i in regions:
            page, host = region(page, *regions[i]), host.get_region(*regions[i])
        pages.append(page)
        rows += host.to_rows()
    return pages, rows


def build_side(types, host_pages, input_mem, expected_positions, regions=None):
    """A built lookup source over the pages, every channel a build output channel -> the bridge and the build rows in arrival order."""
    pages, rows = feed(host_pages, input_mem, regions)
    bridge = LookupSourceFactory()
    builder = HashBuilderOperator(bridge, types, [0], list(range(len(types))), expected_positions=expected_positions)
    for p in pages:
        assert builder.needsInput()
        builder.addInput(p)
    builder.finish()
    assert builder.isFinished() and bridge.positionCount() == len(rows)
    return bridge, builder, rows


def join_model(probe_rows, build_rows, probe_outer=False):
    """Per probe row its matches by build arrival, the latest first (the position chain of the reference's PagesHash, which the operator
    follows); probe_outer: a probe row without a match once, the build channels NULL."""
    out = []
    for p in probe_rows:
        matches = [b for b in reversed(build_rows) if p[0] is not None and b[0] == p[0]]
        out += [p + b for b in matches]
        if probe_outer and not matches:
            out.append(p + (None,) * len(build_rows[0]))
    return out


BUILD_SIDES = {"late_nulls": lambda: (LATE_TYPES, late_null_pages(), None), "varchar_edges": lambda: (VARCHAR_TYPES, varchar_edge_pages(), {0: (1, 2), 4: (3, 4)}),
               "wide": lambda: wide_pages("order_by") + (None,)}


@on_gpu
@pytest.mark.parametrize("side", list(BUILD_SIDES))
@pytest.mark.parametrize("expected_positions", ["none_expected", "exactly_expected", "1000_expected"])
@pytest.mark.parametrize("join_type", [abi.JOIN_INNER, abi.JOIN_FULL_OUTER], ids=["inner", "full_outer"])
@pytest.mark.parametrize("input_mem", ["host_pages", "device_pages"])
@pytest.mark.parametrize("output_mem", [abi.MEM_HOST, abi.MEM_DEVICE], ids=["host_output", "device_output"])
def test_hash_build_holds_every_page(gpu, side, expected_positions, join_type, input_mem, output_mem):
    """The builder's room for rows smaller than, equal to and larger than what arrives; read back by LookupJoin (by build position, in
    chain order) and, for a full outer join, by LookupOuter (the build rows no probe row reached, ascending)."""
    types, pages, regions = BUILD_SIDES[side]()
    count = sum(regions[i][1] if regions and i in regions else p.position_count for i, p in enumerate(pages))
    expected = {"none_expected": 0, "exactly_expected": count, "1000_expected": 1000}[expected_positions]
    bridge, builder, build_rows = build_side(types, pages, input_mem, expected, regions)
    assert len(build_rows) == count
    probe_rows = [(k,) for k in PROBE_KEYS]
    probe = Page([Block.bigint(PROBE_KEYS)], len(PROBE_KEYS))
    outer = join_type == abi.JOIN_FULL_OUTER
    join = LookupJoinOperator(bridge, [abi.BIGINT], [0], [0], join_type=join_type, output_mem=output_mem)
    got = drain(join, [upload_page(probe) if input_mem == "device_pages" else probe])
    want = join_model(probe_rows, build_rows, probe_outer=outer)
    assert len(want) >= len(build_rows) and bits(got) == bits(want)   # (every build key is among the probe keys)
    if outer:
        rest = drain(LookupOuterOperator(bridge, [abi.BIGINT], [0], join_type=join_type, output_mem=output_mem), [])
        assert bits(rest) == bits([(None,) + b for b in build_rows if b[0] not in PROBE_KEYS])
    join.close()
    builder.close()


@on_gpu
@pytest.mark.parametrize("input_mem", ["host_pages", "device_pages"])
@pytest.mark.parametrize("output_mem", [abi.MEM_HOST, abi.MEM_DEVICE], ids=["host_output", "device_output"])
def test_hash_build_read_by_the_fused_probe(gpu, input_mem, output_mem):
    """FilterAndProject + LookupJoin behind one handle reads the build columns inside its kernel: one integer key without duplicates (the
    arrival number in place of channel 0) and no VARCHAR channel.  The DOUBLE and BOOLEAN channels get their NULL flags with the third page."""
    types = [abi.BIGINT, abi.INTEGER, abi.DOUBLE, abi.BOOLEAN]
    pages, at = [], 0
    for p in late_null_pages():
        pages.append(Page([Block.bigint(range(at + 1, at + 1 + p.position_count)), p.blocks[1], p.blocks[3], p.blocks[4]], p.position_count))
        at += p.position_count
    bridge, builder, build_rows = build_side(types, pages, input_mem, 0)
    assert [r[0] for r in build_rows] == list(range(1, 14)) and build_rows[5][2:] == (None, None)
    keys = [13, 1, 99, 6, 5, 7]   # (both ends of the build side, a miss, the row of NULLs and its neighbours)
    probe = Page([Block.bigint(keys)], len(keys))
    op = FusedJoinOperator(bridge, [abi.BIGINT], None, [field(0, abi.BIGINT)], [0], [0], output_mem=output_mem)
    got = drain(op, [upload_page(probe) if input_mem == "device_pages" else probe])
    assert bits(got) == bits(join_model([(k,) for k in keys], build_rows)) and len(got) == 5
    op.close()
    builder.close()


# ---- kept_probe: a probe page that comes out as several, while its producer takes its buffers back ----------------------------------------
def overwrite(buf, byte):
    if buf is not None:
        fill = (ctypes.c_uint8 * buf.nbytes)(*([byte] * buf.nbytes))
        assert lib().pa_memcpy_h2d(buf.ptr, ctypes.addressof(fill), buf.nbytes, None) == 0


@on_gpu
@pytest.mark.parametrize("input_mem", ["host_pages", "device_pages"])
def test_kept_probe_page_outlives_its_buffers(gpu, input_mem, monkeypatch):
    """At most 3 rows per output page: the probe page -- rows [2, 12) of the 13 rows above as one block, so its VARCHAR channel starts at byte
    5 -- comes out over several getOutput calls.  A device page that is not PAGE_STABLE is its producer's again after the first of them:
    every array of the block is overwritten then (offsets of 0, flags of 0, other values), and the remaining pages must still be the join of
    the rows as they were.  Probe-outer: the rows with key 3 find no build row.  The host page is the control (it is staged, not kept).
    The last probe channel is a VARCHAR block of empty strings: no bytes, and on the device no values array at all (a null pointer)."""
    monkeypatch.setenv("PRESTO_AMD_JOIN_MAX_OUTPUT_ROWS", "3")
    rows = [r for p in late_null_pages() for r in p.to_rows()]
    columns = list(zip(*rows))
    whole = Page([Block.bigint(columns[0]), Block.integer(columns[1]), Block.varchar(columns[2]),
                  Block.double([0.0 if v is None else v for v in columns[3]], [v is None for v in columns[3]]),
                  Block.boolean([bool(v) for v in columns[4]], [v is None for v in columns[4]]), Block.varchar([b""] * len(rows))], len(rows))
    rows = [r + (b"",) for r in rows]
    assert bits(whole.to_rows()) == bits(rows) and int(whole.get_region(2, 10).blocks[2].offsets[0]) == 5
    bridge, builder, build_rows = build_side(LATE_TYPES, late_null_pages()[:3], "host_pages", 0, regions={0: (1, 3)})
    assert sorted(r[0] for r in build_rows) == [1, 1, 2, 2]   # (no probe row has more matches than an output page holds)
    page = upload_page(whole) if input_mem == "device_pages" else whole
    if input_mem == "device_pages":
        page.blocks[5].values = None
    probe, probe_rows = region(page, 2, 10), rows[2:12]
    assert not probe.stable

    def producer_takes_its_buffers_back():
        if input_mem == "device_pages":
            for b in page.blocks:
                overwrite(b.values, 0x23)
                overwrite(b.offsets, 0)
                overwrite(b.nulls, 0)
    join = LookupJoinOperator(bridge, LATE_TYPES + [abi.VARCHAR], [0], [2, 3, 0, 1, 4, 5], join_type=abi.JOIN_PROBE_OUTER)
    got = drain(join, [probe], after_first_output=producer_takes_its_buffers_back)
    want = [(p[2], p[3], p[0], p[1], p[4], p[5]) + tuple(m[6:]) for m in join_model(probe_rows, build_rows, probe_outer=True) for p in [m[:6]]]
    assert len(want) > 3 * 3 and any(r[6] is None for r in want) and any(r[0] is None and r[1] is None for r in want)
    assert bits(got) == bits(want)
    join.close()
    builder.close()


# ---- merge_pages: FilterAndProject's buffer of small output pages ------------------------------------------------------------------------------
def merge_model(types, pages_of_rows, min_rows, min_bytes, max_bytes):
    """MergePages over the non-empty pages: a page of min_rows rows or min_bytes bytes passes (behind what is buffered); a smaller one is
    buffered, and the buffer leaves when it holds max_bytes.  Bytes as Page.getSizeInBytes counts them: a fixed-width value and its flag,
    a string's bytes and 5 more."""
    out, held, size = [], [], 0
    for rows in pages_of_rows:
        if not rows:
            continue
        nbytes = sum(sum(len(r[c] or b"") for r in rows) + 5 * len(rows) if t == abi.VARCHAR else (abi.TYPE_WIDTH[t] + 1) * len(rows) for c, t in enumerate(types))
        if len(rows) >= min_rows or nbytes >= min_bytes:
            out += ([held] if held else []) + [rows]
            held, size = [], 0
            continue
        held, size = held + rows, size + nbytes
        if size >= max_bytes:
            out.append(held)
            held, size = [], 0
    return out + ([held] if held else [])


MERGE_INPUTS = {
    # the buffer leaves after the 7-row page, with the flags the one-row page brought; the second merged page holds no NULL
    "late_nulls": lambda: (LATE_TYPES, [late_null_pages()[i] for i in (0, 1, 2, 3, 0, 3)], None, 400),
    # the first merged page ends with a page of no bytes, the second begins with one
    "varchar_edges": lambda: (VARCHAR_TYPES, varchar_edge_pages(), {0: (1, 2), 4: (3, 4)}, 120)}


@on_gpu
@pytest.mark.parametrize("inputs", list(MERGE_INPUTS))
@pytest.mark.parametrize("projections", ["identity", "selective_filter"])
@pytest.mark.parametrize("input_mem", ["host_pages", "device_pages"])
@pytest.mark.parametrize("output_mem", [abi.MEM_HOST, abi.MEM_DEVICE], ids=["host_output", "device_output"])
def test_merge_pages_buffer(gpu, inputs, projections, input_mem, output_mem):
    """Identity projections of a fully selected page are views of the input page, appended as they are; behind a filter that drops rows
    the columns are the operator's own.  The merged pages are compared one by one: a flag left over from a flushed page would show as a NULL."""
    types, host_pages, regions, max_bytes = MERGE_INPUTS[inputs]()
    pages, _ = feed(host_pages, input_mem, regions)
    keep = (lambda r: True) if projections == "identity" else (lambda r: r[1] < 7)
    flt = None if projections == "identity" else field(1, abi.INTEGER) < constant(7, abi.INTEGER)
    op = FilterAndProjectOperator(types, flt, [field(c, t) for c, t in enumerate(types)], output_mem=output_mem, min_output_page_size=max_bytes,
                                  min_output_page_row_count=100, max_output_page_size=max_bytes)
    got = []
    for p in pages + [None]:
        if p is None:
            op.finish()
        else:
            assert op.needsInput()
            op.addInput(p)
        for _ in range(8):
            out = op.getOutput()
            if out is None:
                break
            got.append((download_page(out) if out.mem == abi.MEM_DEVICE else out).to_rows())
    assert op.isFinished()
    op.close()
    inputs_rows = [[r for r in (h.get_region(*regions[i]) if regions and i in regions else h).to_rows() if keep(r)] for i, h in enumerate(host_pages)]
    want = merge_model(types, inputs_rows, 100, max_bytes, max_bytes)
    assert len(want) >= 2 and all(len(page) > max(len(rows) for rows in inputs_rows) for page in want[:1])
    assert [bits(page) for page in got] == [bits(page) for page in want]
    if inputs == "late_nulls":
        assert any(v is None for r in want[0] for v in r) and not any(v is None for r in want[1] for v in r)
