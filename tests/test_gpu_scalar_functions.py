"""LIKE, substr, length and year / month / day on the device, bit for bit against tests/scalar_model.py (the C oracle does not know them):

  a. FilterAndProject: every function as a filter and as a BOOLEAN / BIGINT projection; host and device pages, channels with and without a
     valueIsNull array, pages of 1, 65 and 257 rows (strings of mixed lengths inside a wave);
  b. a seeded random LIKE leg, 512 rows x 32 patterns;
  c. the same row function in every fused tier (plain, staged, few-groups, HBM table, join probe), each leg asserting its kernel by name;
  d. LIKE over a dictionary block (the dictionary-aware filter path), and the pinned SQL-definition behaviour at a line feed.

One JIT compilation costs far more than a launch: patterns ride as projections of one operator, operands come from columns, and the
filter legs reuse a handful of patterns.  A substr whose result is VARCHAR is checked through its consumers (eq against a column that
holds the model's string, IN, LIKE, length).
"""
import functools
import os
import random
import re

import numpy as np
import pytest

from presto_amd import abi
from presto_amd.expr import and_, constant, day, field, length, month, substr, year
from presto_amd.operators import (Driver, FilterAndProjectOperator, FusedAggregationOperator, FusedJoinAggregationOperator, HashBuilderOperator,
                                  LookupSourceFactory, to_pages, upload_page)
from presto_amd.page import Block, Page
from tests import expr_model as M
from tests import scalar_model as S

on_gpu = pytest.mark.gpu
SIZES = (1, 65, 257)
VC, DT, BI = abi.VARCHAR, abi.DATE, abi.BIGINT


def rows_of(op, pages):
    try:
        return [r for p in to_pages(op, pages) for r in p.to_rows()]
    finally:
        op.close()


def tile(rows, n, shift=0):
    return [rows[(k + shift) % len(rows)] for k in range(n)]


def pages_of(columns, rows, nullable):
    """(host page, rows) for pages of 1, 65 and 257 rows (up to 1285 rows: the 257-row pages together hold every row); without a valueIsNull
    array: the NULL-free rows"""
    if not nullable:
        rows = [r for r in rows if None not in r]
    out = []
    for n, most in zip(SIZES, (3, 2, 5)):
        for shift in list(range(0, len(rows), n))[-most:]:
            part = tile(rows, n, shift)
            out.append((M.page_of(columns, part, nullable=nullable), part))
    return out


def both(page):
    return (page, upload_page(page))


# ---- a. LIKE: values and patterns ----------------------------------------------------------------------------------------------------------
# No value holds a line feed (scalar-like-line-feed: test_line_feed_follows_the_sql_definition pins those).
LIKE_VALUES = ["", "a", "aa", "ab", "ba", "aba", "abba", "abxba", "ababa", "aab", "aaab", "xaab", "aabx", "aaba", "PROMO", "PROM", "PROMOX", "PROMO BRUSHED TIN",
               "xPROMO", "LARGE PROMO", "é", "名", "\U0001F600", "aé", "éa", "a名b", "a\U0001F600b", "aéb", "名名", "\U0001F600\U0001F600", "%", "_", "a%b",
               "a_b", "#", "a#b", "\\", "a.b", "a*b", None]
# (pattern, escape or None)
LIKE_PATTERNS = [("", None), ("%", None), ("%%", None), ("PROMO", None), ("PROMO%", None), ("%PROMO", None), ("%PROMO%", None), ("ab%ba", None),
                 ("%aab%", None), ("%a%a%", None), ("a%", None), ("%a", None), ("a%b%a", None), ("_", None), ("__", None), ("_%", None), ("%_", None),
                 ("a_b", None), ("_a", None), ("a_", None), ("%a_b%", None), ("_%_", None), ("%_a_%", None), ("a.b", None), ("a*b", None), ("\\", None),
                 ("a#%b", "#"), ("a#_b", "#"), ("a##b", "#"), ("#%%", "#"), ("%#_", "#"), ("_#%_", "#"), ("a#b", ""), ("a_b", "")]
FILTER_PATTERNS = [("PROMO", None), ("PROMO%", None), ("%PROMO", None), ("%aab%", None), ("ab%ba", None), ("%a_b%", None), ("a#%b", "#")]


def like_expr(x, pattern, escape):
    return x.like(pattern) if escape is None else x.like(pattern, escape)


def model_like(value, pattern, escape):
    return S.like(value, pattern, escape, has_escape=escape is not None)


def test_like_cases_hold_what_they_are_for():
    """on the model alone: the cases a matcher gets wrong are there and come out as SQL says"""
    assert model_like("aba", "ab%ba", None) is False and model_like("abba", "ab%ba", None) is True
    assert model_like("aaab", "%aab%", None) is True
    assert model_like("a", "%a%a%", None) is False and model_like("aa", "%a%a%", None) is True
    assert model_like("", "_%", None) is False and model_like("", "%_", None) is False and model_like("", "", None) is True and model_like("", "%", None) is True
    for c in ("a", "é", "名", "\U0001F600"):
        assert model_like(c, "_", None) is True and model_like(c, "__", None) is False
    assert model_like("PROM", "PROMO%", None) is False and model_like("PROMO", "PROMO%", None) is True and model_like("PROMOX", "PROMO%", None) is True
    assert model_like("a%b", "a#%b", "#") is True and model_like("aab", "a#%b", "#") is False and model_like("a#b", "a##b", "#") is True
    for pattern, escape in LIKE_PATTERNS:
        got = [model_like(v, pattern, escape) for v in LIKE_VALUES if v is not None]
        assert "\n" not in pattern and True in got and (False in got or pattern in ("%", "%%")), (pattern, got)


@on_gpu
@pytest.mark.parametrize("nullable", [True, False], ids=["nulls", "no_nulls"])
@pytest.mark.parametrize("half", [0, 1])
def test_like_projections(gpu, nullable, half):
    patterns = LIKE_PATTERNS[half::2]
    s = field(0, VC)
    make = lambda: FilterAndProjectOperator([VC], None, [like_expr(s, p, e) for p, e in patterns])
    for host, part in pages_of(["VARCHAR"], [(v,) for v in LIKE_VALUES], nullable):
        want = [tuple(model_like(v, p, e) for p, e in patterns) for v, in part]
        for page in both(host):
            got = rows_of(make(), [page])
            wrong = [(part[i][0], patterns[j], g[j], w[j]) for i, (g, w) in enumerate(zip(got, want)) for j in range(len(patterns)) if g[j] != w[j]]
            assert len(got) == len(want) and not wrong, (len(part), page.mem, len(wrong), wrong[:8])


@on_gpu
@pytest.mark.parametrize("pattern,escape", FILTER_PATTERNS, ids=[p for p, _ in FILTER_PATTERNS])
def test_like_filters(gpu, pattern, escape):
    rows = [(v, i) for i, v in enumerate(LIKE_VALUES)]
    for nullable in (True, False):
        make = lambda: FilterAndProjectOperator([VC, BI], like_expr(field(0, VC), pattern, escape), [field(1, BI), field(0, VC)])
        for host, part in pages_of(["VARCHAR", "BIGINT"], rows, nullable):
            want = [(i, v.encode()) for v, i in part if model_like(v, pattern, escape) is True]
            for page in both(host):
                assert rows_of(make(), [page]) == want, (pattern, nullable, len(part), page.mem)


def test_the_last_string_ends_at_the_last_byte_of_its_buffer():
    """the byte loops stop at the string's end: behind the last row's string there is nothing of the column left to read"""
    page = M.page_of(["VARCHAR"], [("ab",), ("PROMO",)])
    block = page.blocks[0]
    assert int(block.offsets[-1]) == len(block.values) == 7


# ---- b. the random leg --------------------------------------------------------------------------------------------------------------------------
ALPHABET = ["a", "b", "é", "名", "\U0001F600"]
SEED = 5


def random_like_case(seed=SEED):
    """512 values of 0 .. 40 bytes over ALPHABET, 32 patterns of up to 6 tokens from ALPHABET, `%` and `_`"""
    rng = random.Random(seed)
    values = []
    for _ in range(512):
        budget, v = rng.randint(0, 40), ""
        while True:
            c = rng.choice(ALPHABET[:2] if rng.random() < 0.5 else ALPHABET)
            if len((v + c).encode()) > budget:
                break
            v += c
        values.append(v)
    patterns = []
    while len(patterns) < 32:
        p = "".join(rng.choice(["%", "%", "%", "_", "_"] + ALPHABET[:2] * 2 + ALPHABET) for _ in range(rng.randint(1, 6)))
        if p not in patterns:
            patterns.append(p)
    return values, patterns


def test_random_leg_is_balanced():
    """chosen with the model alone: between 10 % and 90 % of the (row, pattern) pairs match, and the three kinds of code are all there"""
    values, patterns = random_like_case()
    hits = sum(S.like(v, p) for v in values for p in patterns)
    assert 0.10 * 512 * 32 <= hits <= 0.90 * 512 * 32, hits
    assert any("_" in p for p in patterns) and any("_" not in p and "%" in p for p in patterns)
    assert max(len(v.encode()) for v in values) <= 40 and min(len(v) for v in values) == 0


@on_gpu
@pytest.mark.parametrize("half", [0, 1])
def test_like_random(gpu, half):
    values, patterns = random_like_case()
    patterns = patterns[16 * half:16 * half + 16]
    want = [tuple(S.like(v, p) for p in patterns) for v in values]
    op = FilterAndProjectOperator([VC], None, [field(0, VC).like(p) for p in patterns])
    got = rows_of(op, [upload_page(M.page_of(["VARCHAR"], [(v,) for v in values]))])
    wrong = [(values[i], patterns[j], g[j], w[j]) for i, (g, w) in enumerate(zip(got, want)) for j in range(16) if g[j] != w[j]]
    assert len(got) == 512 and not wrong, (len(wrong), wrong[:8])


# ---- a. substr and length -------------------------------------------------------------------------------------------------------------------
SUBSTR_VALUES = ["", "a", "abc", "Quadratically", "é名\U0001F600a", "信念,爱,希望", "\U0001042Dend"]


def device_substr(value, start, length=None, has_length=False):
    """the model -- and, where the reference itself fails (the wrapped int addition of StringFunctions.java:360 asks Slice.slice for a
    negative length), the empty string: DESIGN.md section 5, scalar-substr-wrapped-length"""
    try:
        return S.substr(value, start, length, has_length)
    except S.ReferenceFails:
        return ""


@functools.lru_cache(maxsize=None)
def substr_rows():
    """(value, start, length, substr(value, start), substr(value, start, length)): every branch of :278-368"""
    rows = []
    for v in SUBSTR_VALUES + [None]:
        n = len(v) if v else 3
        starts = [0, 1, -1, 2, -2, n, -n, n + 1, -(n + 1), S.INT64_MIN, S.INT64_MAX, S.INT32_MAX + 1, None]
        lengths = [0, -1, 1, 2, n, n + 1, S.INT64_MAX, S.INT64_MIN, S.INT32_MAX, S.INT32_MAX - 1, None]
        for s in starts:
            for ln in lengths:
                rows.append((v, s, ln, device_substr(v, s), device_substr(v, s, ln, True)))
    return rows


def test_substr_rows_reach_every_branch():
    rows = substr_rows()
    wrapped = [(v, s, ln) for v, s, ln, _, _ in rows if None not in (v, s, ln) and v and s < 0 and -s <= len(v) and ln >= S.INT32_MAX - 1]
    assert ("abc", -2, S.INT64_MAX) in wrapped and ("abc", -3, S.INT64_MAX) in wrapped
    with pytest.raises(S.ReferenceFails):
        S.substr("abc", -2, S.INT64_MAX, True)
    assert S.substr("abc", -3, S.INT64_MAX, True) == "abc" and S.substr("abc", -2, S.INT32_MAX - 1, True) == "bc"   # no wrap: clipped
    assert {r[4] for r in rows if r[0] == "é名\U0001F600a"} >= {"", "é", "é名", "a", "\U0001F600a", "é名\U0001F600a", "名", None}


COLUMNS5 = ["VARCHAR", "BIGINT", "BIGINT", "VARCHAR", "VARCHAR"]


def substr_projections():
    v, s, ln, e2, e3 = field(0, VC), field(1, BI), field(2, BI), field(3, VC), field(4, VC)
    two, three = substr(v, s), substr(v, s, ln)
    return [two.eq(e2), three.eq(e3), length(two), length(three), length(v), three.isin("bc", "a", "", "é名"), three.like("%c"), three.like("_%"),
            two.like("%a_"), length(substr(three, 2, 1)), three.is_null_(), (two < e3)]


def substr_expected(row):
    v, s, ln, r2, r3 = row
    inner = device_substr(r3, 2, 1, True)
    return (None if r2 is None else True, None if r3 is None else True, S.length(r2), S.length(r3), S.length(v),
            None if r3 is None else r3 in ("bc", "a", "", "é名"), S.like(r3, "%c"), S.like(r3, "_%"), S.like(r2, "%a_"), S.length(inner), r3 is None,
            None if r2 is None or r3 is None else r2.encode() < r3.encode())


@on_gpu
@pytest.mark.parametrize("nullable", [True, False], ids=["nulls", "no_nulls"])
def test_substr_and_length_projections(gpu, nullable):
    make = lambda: FilterAndProjectOperator(M.input_types(COLUMNS5), None, substr_projections())
    rows = substr_rows()
    for host, part in pages_of(COLUMNS5, rows, nullable):
        want = [substr_expected(r) for r in part]
        for page in both(host):
            got = rows_of(make(), [page])
            wrong = [(part[i][:3], j, g[j], w[j]) for i, (g, w) in enumerate(zip(got, want)) for j in range(len(w)) if g[j] != w[j]]
            assert len(got) == len(want) and not wrong, (nullable, len(part), page.mem, len(wrong), wrong[:8])


@on_gpu
def test_substr_content_is_compared_byte_for_byte(gpu):
    """eq against the model's string passes above; against any other string it must not (a slice of the right length at the wrong place)"""
    rows = [(v, s, ln, (r3 or "") + "x", (r3[:-1] + "~") if r3 else "~") for v, s, ln, _, r3 in substr_rows() if r3 is not None]
    v, s, ln, e2, e3 = (field(i, t) for i, t in enumerate(M.input_types(COLUMNS5)))
    op = FilterAndProjectOperator(M.input_types(COLUMNS5), None, [substr(v, s, ln).eq(e2), substr(v, s, ln).eq(e3)])
    assert set(rows_of(op, [upload_page(M.page_of(COLUMNS5, rows))])) == {(False, False)}


@on_gpu
def test_substr_and_length_filters(gpu):
    rows = [(v, s, ln, i) for i, (v, s, ln, _, _) in enumerate(substr_rows())]
    cols = ["VARCHAR", "BIGINT", "BIGINT", "BIGINT"]
    v, s, ln, i = (field(k, t) for k, t in enumerate(M.input_types(cols)))
    filters = {
        "substr": (substr(v, s, ln).eq(constant("bc", VC)), lambda r: device_substr(r[0], r[1], r[2], True) == "bc"),
        "length": (length(v) > 3, lambda r: r[0] is not None and len(r[0]) > 3),
    }
    for name, (flt, keep) in filters.items():
        make = lambda: FilterAndProjectOperator(M.input_types(cols), flt, [i])
        host = M.page_of(cols, rows, nullable=True)
        want = [(r[3],) for r in rows if keep(r)]
        assert want
        for page in both(host):
            assert rows_of(make(), [page]) == want, (name, page.mem)


# ---- a. year / month / day ---------------------------------------------------------------------------------------------------------------------
DAYS = [0, -1, 59, 60, 11016, 11017, -719528, -719529, -719162, -719163, S.INT32_MIN, S.INT32_MAX, 365, 366, 730, 789, 2932896, 2932897, -141427, 9131, None]


def date_rows():
    rng = random.Random(11)
    return [(d,) for d in DAYS] + [(rng.randint(S.INT32_MIN, S.INT32_MAX),) for _ in range(200)] + [(rng.randint(-800000, 60000),) for _ in range(300)]


def test_date_rows_hold_the_edges():
    assert S.civil(59) == (1970, 3, 1) and S.civil(11016) == (2000, 2, 29) and S.civil(11017) == (2000, 3, 1)
    assert S.civil(-719528) == (0, 1, 1) and S.civil(-719529) == (-1, 12, 31)
    assert {0, -1, 59, 60, 11016, 11017, -719528, -719529, S.INT32_MIN, S.INT32_MAX} <= set(DAYS)


@on_gpu
@pytest.mark.parametrize("nullable", [True, False], ids=["nulls", "no_nulls"])
def test_date_field_projections(gpu, nullable):
    d = field(0, DT)
    make = lambda: FilterAndProjectOperator([DT], None, [year(d), month(d), day(d)])
    for host, part in pages_of(["DATE"], date_rows(), nullable):
        want = [(S.year(x), S.month(x), S.day(x)) for x, in part]
        for page in both(host):
            got = rows_of(make(), [page])
            wrong = [(part[i][0], g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
            assert len(got) == len(want) and not wrong, (nullable, len(part), page.mem, wrong[:8])


@on_gpu
def test_date_field_filters(gpu):
    rows = date_rows()
    d = field(0, DT)
    for name, flt, keep in (("year", year(d).eq(2000), lambda x: S.year(x) == 2000), ("month", month(d).eq(2), lambda x: S.month(x) == 2),
                            ("day", day(d) > 28, lambda x: S.day(x) > 28)):
        make = lambda: FilterAndProjectOperator([DT], flt, [d])
        want = [r for r in rows if r[0] is not None and keep(r[0])]
        assert want
        host = M.page_of(["DATE"], rows, nullable=True)
        for page in both(host):
            assert rows_of(make(), [page]) == want, (name, page.mem)


# ---- c. the same row function in every fused tier ---------------------------------------------------------------------------------------------
TIERS = ["plain", "staged", "few_groups", "hbm_table", "join_probe"]
BUILD_KEYS = 8
FUSED_PAGE = 256
FUSED_FILTERS = {"chain": "a%b%a", "general": "%a_b%"}
YEAR = 1995


@functools.lru_cache(maxsize=None)
def fused_rows():
    """(string, date) pairs: strings of 0 .. 12 bytes over ALPHABET, days around 1995, some NULLs"""
    rng = random.Random(5)
    first = 9131 - 100        # 9131 = 1995-01-01
    rows = []
    for i in range(2 * FUSED_PAGE):
        v = "".join(rng.choice(ALPHABET[:2] * 4 + ALPHABET) for _ in range(rng.randint(0, 7)))
        rows.append((None if i % 37 == 5 else v, None if i % 41 == 7 else first + rng.randint(0, 600)))
    return rows


def fused_operator(pattern, tier):
    """-> (operator, closer)"""
    s, d, key = field(0, VC), field(1, DT), field(2, BI)
    flt = and_(s.like(pattern), year(d).eq(YEAR))
    types = [VC, DT, BI]
    aggs = [(abi.AGG_COUNT_STAR, -1, None)]
    if tier in ("plain", "staged"):
        return FusedAggregationOperator(types, flt, [key], [], aggs), None
    if tier == "few_groups":
        return FusedAggregationOperator(types, flt, [key], [0], aggs), None
    if tier == "hbm_table":
        return FusedAggregationOperator(types, flt, [key], [0], aggs, expected_groups=(1 << 20) + 1), None
    bridge = LookupSourceFactory()
    builder = HashBuilderOperator(bridge, [BI, BI], [0], [1])
    op = FusedJoinAggregationOperator(bridge, types, flt, [key], [0], [0], [BI, BI], [0], aggs)
    keys = np.arange(BUILD_KEYS, dtype=np.int64)
    Driver([Page([Block.bigint(keys), Block.bigint(keys * 10)], BUILD_KEYS)], [builder]).run()
    return op, builder


def key_of(tier, index):
    return index if tier == "hbm_table" else index % BUILD_KEYS


def check_name(tier, name):
    prefix = {"plain": "pa_fused_global_", "staged": "pa_fused_global_staged_", "few_groups": "pa_fused_lds_", "hbm_table": "pa_fused_gt_",
              "join_probe": "pa_fused_probe_"}[tier]
    assert name.startswith(prefix) and (tier != "plain" or "staged" not in name), (tier, name)


def test_fused_rows_select_some_and_reject_some():
    for pattern in FUSED_FILTERS.values():
        kept = [r for r in fused_rows() if S.like(r[0], pattern) is True and r[1] is not None and S.year(r[1]) == YEAR]
        by_like = [r for r in fused_rows() if S.like(r[0], pattern) is True]
        assert 10 <= len(kept) < len(by_like) < len(fused_rows()) - 50, (pattern, len(kept), len(by_like))


@on_gpu
@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("shape", sorted(FUSED_FILTERS))
def test_fused_tiers(gpu, monkeypatch, shape, tier):
    monkeypatch.setenv("PRESTO_AMD_STAGED", "1" if tier == "staged" else "0")
    if tier == "hbm_table":
        monkeypatch.setenv("PRESTO_AMD_NO_PARTITIONED", "1")   # the HBM table's own kernel, not the partition-owned LDS tables in front of it
    pattern = FUSED_FILTERS[shape]
    rows = [r + (key_of(tier, i),) for i, r in enumerate(fused_rows())]
    pages = [M.page_of(["VARCHAR", "DATE", "BIGINT"], rows[at:at + FUSED_PAGE], nullable=True) for at in range(0, len(rows), FUSED_PAGE)]
    want = {}
    for v, d, k in rows:
        if S.like(v, pattern) is True and d is not None and S.year(d) == YEAR:
            want[k] = want.get(k, 0) + 1
    op, builder = fused_operator(pattern, tier)
    try:
        got = [r for p in to_pages(op, pages) for r in p.to_rows()]
        name = op.kernelName()
    finally:
        op.close()
        if builder is not None:
            builder.close()
    check_name(tier, name)
    if tier in ("plain", "staged"):
        assert got == [(sum(want.values()),)], (shape, tier, got)
    else:
        assert sorted(got) == sorted(want.items()), (shape, tier)


# ---- d. dictionary blocks, the line feed --------------------------------------------------------------------------------------------------------
@on_gpu
def test_like_over_a_dictionary_block(gpu):
    """a filter over one channel runs over the dictionary (DictionaryAwarePageFilter), the rows look their entry up"""
    words = ["PROMO BURNISHED COPPER", "LARGE BRUSHED BRASS", "PROMO", "STANDARD POLISHED TIN", "", "PROMOTION", None, "xPROMO"]
    n = 300
    ids = [(7 * i + 3) % len(words) for i in range(n)]
    page = Page([Block.dictionary_block(Block.varchar(words), ids), Block.bigint(np.arange(n, dtype=np.int64))], n)
    for pattern in ("PROMO%", "%R_S%", "%BR%S%"):
        op = FilterAndProjectOperator([VC, BI], field(0, VC).like(pattern), [field(1, BI)])
        want = [(i,) for i in range(n) if S.like(words[ids[i]], pattern) is True]
        assert want and rows_of(op, [page]) == want, pattern


def design_tags():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "DESIGN.md")).read()
    section = text[text.index("## 5. Parity"):text.index("## 6. Measurement")]
    return set(re.findall(r"`(scalar-[a-z-]+)`", section))


def test_design_names_the_scalar_divergences():
    assert design_tags() == {"scalar-like-line-feed", "scalar-substr-wrapped-length"}


@on_gpu
def test_line_feed_follows_the_sql_definition(gpu):
    """`scalar-like-line-feed`: the reference anchors its regular expression with `$`, which under its syntax may also
    match before a line feed; the device implements the SQL definition -- the whole value must match -- and `_` / `%` take a line feed
    like any other character.  Pinned so that a change is a decision."""
    cases = [("abc\nx", "abc", False), ("abc\n", "abc", False), ("abc\n", "abc_", True), ("abc\nx", "abc%", True), ("\n", "_", True), ("\n", "", False),
             ("a\nb", "a_b", True), ("a\nb", "a%b", True), ("a\nb", "%b", True), ("x\nabc", "abc", False), ("x\nabc", "%abc", True)]
    patterns = sorted({p for _, p, _ in cases})
    op = FilterAndProjectOperator([VC], None, [field(0, VC).like(p) for p in patterns])
    got = rows_of(op, [M.page_of(["VARCHAR"], [(v,) for v, _, _ in cases])])
    for (v, p, expected), g in zip(cases, got):
        assert S.like(v, p) is expected and g[patterns.index(p)] == expected, (v, p, g)
