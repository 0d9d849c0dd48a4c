"""VARCHAR(1) group keys whose offsets the vector loops no longer read ("VARCHAR(1) keys without offsets"): when the n
strings of a launch hold n bytes and the four key bytes of a quad are ASCII, the quad's offsets are computed.  FusedAggregationOperator
with two VARCHAR(1) keys -- the Q1 shape and a smaller one (two keys, an exact BIGINT sum, a count) -- against the oracle, over pages of
2^22 + 1003 rows (the vector loop runs, the row count is no multiple of 256): pages that qualify, pages that do not (an empty string;
ranges of a table that hold one), quads that do not (bytes >= 0x80), a page that violates the declared type and must go on failing."""
import numpy as np
import pytest

from presto_amd import abi, tpch
from presto_amd._lib import PrestoAmdError
from presto_amd.exchange import partial_layout
from presto_amd.expr import field
from presto_amd.operators import FusedAggregationOperator, HashAggregationOperator, to_pages, upload_page
from presto_amd.page import Block, Page
from tests.test_gpu_small_pages import bounds_of, stable_regions

pytestmark = pytest.mark.gpu

N = (1 << 22) + 1003
SMALL_TYPES = [abi.VARCHAR, abi.VARCHAR, abi.BIGINT]
SMALL_AGGS = [(abi.AGG_SUM, 2, abi.BIGINT), (abi.AGG_COUNT_STAR, -1, None)]
_cache = {}


def pick(rng, alphabet, n):
    return rng.choice(np.frombuffer(alphabet, dtype=np.uint8), n)


def unit(n, first=0):
    return np.arange(first, first + n + 1, dtype=np.int32)


def numbers(shape):
    """the channels behind the keys, host blocks and their device copies (shared by the cases of a shape)"""
    if shape not in _cache:
        rng = np.random.default_rng(11)
        if shape == "q1":
            host = [Block.double(rng.integers(1, 51, N).astype(np.float64)), Block.double(rng.random(N) * 1e5), Block.double(rng.integers(0, 11, N) / 100.0),
                    Block.double(rng.integers(0, 9, N) / 100.0), Block.date(rng.integers(10471 - 2000, 10471 + 100, N).astype(np.int32))]
        else:
            host = [Block.bigint(rng.integers(-1000, 1000, N))]
        _cache[shape] = (host, upload_page(Page(host, N)).blocks)
    return _cache[shape]


def pages_of(shape, rf, ls):
    """(host page, device page) of the shape with the key blocks rf, ls"""
    host, dev = numbers(shape)
    keys = upload_page(Page([rf, ls], N)).blocks
    return Page([rf, ls] + host, N), Page(keys + dev, N, abi.MEM_DEVICE)


def operator(shape, **kw):
    if shape == "q1":
        return FusedAggregationOperator(tpch.Q1_TYPES, tpch.q1_filter(), tpch.q1_projections(), tpch.Q1_GROUP_BY, tpch.Q1_AGGREGATES,
                                        type_params=tpch.Q1_TYPE_PARAMS, **kw)
    return FusedAggregationOperator(SMALL_TYPES, None, [field(i, t) for i, t in enumerate(SMALL_TYPES)], [0, 1], SMALL_AGGS, type_params=[1, 1, 0], **kw)


def expected_rows(oracle, shape, host):
    if shape == "q1":
        ref = oracle.HashAggregation([p.type for p in tpch.q1_projections()], tpch.Q1_GROUP_BY, tpch.Q1_AGGREGATES)
        ref.add_page(oracle.filter_project(host, tpch.q1_filter(), tpch.q1_projections()))
    else:
        ref = oracle.HashAggregation(SMALL_TYPES, [0, 1], SMALL_AGGS)
        ref.add_page(host)
    return ref.build_result().to_rows()


def run(shape, pages):
    op = operator(shape)
    rows = [r for p in to_pages(op, pages) for r in p.to_rows()]
    op.close()
    return rows


def assert_same(got, expected):
    g, e = {r[:2]: r for r in got}, {r[:2]: r for r in expected}
    assert len(g) == len(got) and set(g) == set(e), (sorted(g, key=repr), sorted(e, key=repr))
    for k, er in e.items():
        for gv, ev in zip(g[k][2:], er[2:]):
            if isinstance(ev, float):
                assert abs(gv - ev) <= 1e-9 * abs(ev), (k, g[k], er)   # DOUBLE sums: the order of the additions differs
            else:
                assert gv == ev, (k, g[k], er)


def ascii_keys(seed):
    rng = np.random.default_rng(seed)
    return pick(rng, b"ANR", N), pick(rng, b"FO", N)


@pytest.fixture(scope="module")
def ascii_case(gpu, oracle):
    """(a) per shape: host page, device page, the oracle's rows"""
    out = {}
    for shape in ("q1", "small"):
        rf, ls = ascii_keys(1)
        host, dev = pages_of(shape, Block.varwidth(rf, unit(N)), Block.varwidth(ls, unit(N)))
        out[shape] = (host, dev, expected_rows(oracle, shape, host))
    return out


@pytest.mark.parametrize("shape", ["q1", "small"])
def test_a_one_ascii_byte_per_string(gpu, ascii_case, shape):
    host, dev, expected = ascii_case[shape]
    assert len(expected) == 6
    assert_same(run(shape, [dev]), expected)


def test_b_first_offset_not_zero_and_unaligned_buffers(gpu, ascii_case):
    """the same strings behind 5 (and 32) bytes of another page's strings: P != 0; then the page without its first 3 rows, whose buffers
    are not 16-byte aligned (the row-by-row path, which reads the offsets)"""
    host, dev, expected = ascii_case["small"]
    rf, ls = ascii_keys(1)
    shifted_rf = Block.varwidth(np.concatenate([np.frombuffer(b"\xffzz\x80q", dtype=np.uint8), rf]), unit(N, 5))
    shifted_ls = Block.varwidth(np.concatenate([np.full(32, 0xC3, dtype=np.uint8), ls]), unit(N, 32))
    _, shifted = pages_of("small", shifted_rf, shifted_ls)
    assert_same(run("small", [shifted]), expected)
    assert_same(run("small", [host.get_region(0, 3)] + stable_regions(dev, [3, N])), expected)


def test_c_one_empty_string(gpu, oracle):
    """PB = n - 1: the launch that holds the empty string reads its offsets as before"""
    rf, ls = ascii_keys(2)
    offsets = unit(N)
    offsets[(1 << 21) + 77:] -= 1
    host, dev = pages_of("small", Block.varwidth(rf[:-1], offsets), Block.varwidth(ls, unit(N)))
    expected = expected_rows(oracle, "small", host)
    assert len(expected) == 7 and sum(1 for r in expected if r[0] == b"") == 1
    assert_same(run("small", [dev]), expected)


@pytest.mark.parametrize("shape", ["q1", "small"])
def test_d_single_bytes_beyond_ascii(gpu, oracle, shape):
    """every string one byte, one in 300 of them >= 0x80: quads that hold one fall back to their offsets, lane by lane"""
    rng = np.random.default_rng(3)
    rf, ls = pick(rng, b"A", N), pick(rng, b"FO", N)
    rf[rng.random(N) < 1 / 300] = 0xE9
    ls[rng.random(N) < 1 / 300] = 0x80
    host, dev = pages_of(shape, Block.varwidth(rf, unit(N)), Block.varwidth(ls, unit(N)))
    expected = expected_rows(oracle, shape, host)
    assert len(expected) == 6   # within the few-groups tier
    assert_same(run(shape, [dev]), expected)
    if shape == "small":
        # more groups than the few-groups tier holds: the launches are redone on the next tier
        rf[rf == ord("A")] = pick(rng, b"ANR", int((rf == ord("A")).sum()))
        host, dev = pages_of(shape, Block.varwidth(rf, unit(N)), Block.varwidth(ls, unit(N)))
        expected = expected_rows(oracle, shape, host)
        assert len(expected) == 12
        assert_same(run(shape, [dev]), expected)


# what the parent commit answers to the page of test_e (read off a run of this test against the parent's library: status -3,
# 'VARCHAR group key longer than its declared bound / the device key packing supports')
E_STATUS = abi.ERR_NOT_SUPPORTED
E_MESSAGE = "VARCHAR group key longer than its declared bound"


def test_e_two_byte_strings_balanced_by_empty_ones(gpu):
    """'é' (2 bytes) x 4, '' x 4, ...: n bytes over n strings, every launch window alike -- but no byte is ASCII, so every quad reads its
    offsets and the strings over the declared bound fail the query as they did"""
    lengths = np.tile(np.array([2, 2, 2, 2, 0, 0, 0, 0], dtype=np.int32), N // 8 + 1)[:N]
    lengths[N - N % 8:] = 1          # the rows behind the last whole group of 8: one byte each
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    assert offsets[-1] == N
    values = np.tile(np.frombuffer("é".encode(), dtype=np.uint8), N // 2 + 1)[:N]
    _, ls = ascii_keys(4)
    _, dev = pages_of("small", Block.varwidth(values, offsets), Block.varwidth(ls, unit(N)))
    op = operator("small")
    with pytest.raises(PrestoAmdError) as err:
        to_pages(op, [dev])
    op.close()
    assert err.value.status == E_STATUS
    assert E_MESSAGE in err.value.message


def test_f_null_keys_that_keep_their_byte(gpu, oracle):
    """a nullable key channel whose NULL rows keep a one-byte slot: PB == n with NULLs present"""
    rng = np.random.default_rng(5)
    rf, ls = ascii_keys(5)
    nulls = (rng.random(N) < 0.05).astype(np.uint8)
    host, dev = pages_of("small", Block.varwidth(rf, unit(N), nulls), Block.varwidth(ls, unit(N)))
    expected = expected_rows(oracle, "small", host)
    assert len(expected) == 8 and sum(1 for r in expected if r[0] is None) == 2
    assert_same(run("small", [dev]), expected)


def test_g_row_range_table_of_ranges_that_qualify_and_ranges_that_do_not(gpu, oracle):
    """stable pages of 8192 rows that do not continue each other: one table of row ranges.  One range in ten holds an empty string (it
    reads its offsets, and every range behind it starts at an offset that is not its row number), one in ten a byte >= 0x80"""
    rng = np.random.default_rng(6)
    n, page_rows = 1_000_003, 8192
    rf, ls = pick(rng, b"A", n), pick(rng, b"FO", n)   # (with '' and 0xE9: six groups, within the few-groups tier)
    lengths = np.ones(n, dtype=np.int32)
    bounds = bounds_of(n, page_rows)
    for i, lo in enumerate(bounds[:-1]):
        if i % 10 == 3:
            lengths[lo + int(rng.integers(0, min(page_rows, n - lo)))] = 0
        if i % 10 == 7:
            rf[lo + int(rng.integers(0, min(page_rows, n - lo)))] = 0xE9
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    host = Page([Block.varwidth(rf[lengths == 1], offsets), Block.varwidth(ls, unit(n)), Block.bigint(rng.integers(-1000, 1000, n))], n)
    expected = expected_rows(oracle, "small", host)
    assert len(expected) == 6
    dev = upload_page(host)
    regions = stable_regions(dev, bounds)
    order = rng.permutation(len(regions))
    assert_same(run("small", [regions[i] for i in order]), expected)


def test_h_partial_then_final(gpu, ascii_case):
    """two PARTIAL operators that each take the page of (a), one FINAL over their pages: every sum and count twice the oracle's (a
    doubling is exact), the averages the oracle's"""
    host, dev, expected = ascii_case["q1"]
    expected = [r[:2] + tuple(2 * v for v in r[2:6]) + r[6:9] + (2 * r[9],) for r in expected]
    parts = []
    for _ in range(2):
        op = operator("q1", step=abi.STEP_PARTIAL)
        parts += to_pages(op, [dev])
        op.close()
    ptypes, faggs = partial_layout([abi.VARCHAR, abi.VARCHAR], tpch.Q1_AGGREGATES)
    final = HashAggregationOperator(ptypes, [0, 1], faggs, step=abi.STEP_FINAL, type_params=[1, 1] + [0] * (len(ptypes) - 2))
    got = [r for p in to_pages(final, parts) for r in p.to_rows()]
    final.close()
    assert_same(got, expected)
