"""The expression model (tests/expr_model.py) against the reference's own known answers, its coverage of every cell, and the C oracle
against the model cell by cell.  No GPU.

TT = core/trino-main/src/test/java/io/trino/type.  The reference states many floating-point answers as Java expressions (`37.7 % 17.1`,
`12.34f * 56.78f`); they are restated here as the exact rational result rounded once to the format (ieee below), not with the
floating-point operators the model itself uses.
"""
import fractions
import math

import numpy as np
import pytest

from tests import expr_model as M
from presto_amd import abi
from presto_amd.expr import call, constant

F = fractions.Fraction
NAN = float("nan")
OVERFLOW, DIV0 = ("error", M.OUT_OF_RANGE), ("error", M.DIVISION_BY_ZERO)


def ieee(x, real=False):
    """The rational x rounded once, to nearest even, to a double (or a float): normal range only."""
    if x == 0:
        return 0.0
    p = 24 if real else 53
    e = 0
    m = abs(F(x))
    while m >= 2 ** p:
        m /= 2
        e += 1
    while m < 2 ** (p - 1):
        m *= 2
        e -= 1
    q, rem = divmod(m, 1)
    q = int(q)
    if rem > F(1, 2) or (rem == F(1, 2) and q & 1):
        q += 1
    r = F(q) * F(2) ** e
    return float(-r if x < 0 else r)    # exact: r has at most 53 significant bits


def fmod_exact(a, b):
    a, b = F(a), F(b)
    return a - b * math.trunc(a / b)


def big(v): return constant(v, abi.BIGINT)
def i32(v): return constant(v, abi.INTEGER)
def dbl(v): return constant(v, abi.DOUBLE)
def real(v): return constant(float(np.float32(v)), abi.REAL)
def r32(v): return F(float(np.float32(v)))    # the float a REAL literal denotes, exactly


def val(v): return ("value", v)


def real_kats():
    """TT/TestRealOperators.java:57-124: + - * / % over three pairs of literals, by exact rational arithmetic rounded once to a float"""
    pairs = [(12.34, 56.78), (-17.34, -22.891), (-89.123, 754.0)]
    ops = [(abi.OP_ADD, lambda a, b: a + b, 57, 4), (abi.OP_SUBTRACT, lambda a, b: a - b, 69, 4), (abi.OP_MULTIPLY, lambda a, b: a * b, 81, 5),
           (abi.OP_DIVIDE, lambda a, b: a / b, 94, 5), (abi.OP_MODULUS, fmod_exact, 107, 5)]
    out = []
    for op, fn, line, nan in ops:
        for k, (a, b) in enumerate(pairs):
            out.append(("TestRealOperators.java:%d" % (line + k), call(op, abi.REAL, real(a), real(b)), val(ieee(fn(r32(a), r32(b)), real=True))))
        out.append(("TestRealOperators.java:%d" % (line + nan), call(op, abi.REAL, real(NAN), real(1.23)), val(NAN)))
        out.append(("TestRealOperators.java:%d" % (line + nan + 1), call(op, abi.REAL, real(1.23), real(NAN)), val(NAN)))
    return out


def double_kats():
    """TT/TestDoubleOperators.java:66-129"""
    a, b = 37.7, 17.1
    out = []
    ops = [(abi.OP_ADD, lambda x, y: x + y, 66), (abi.OP_SUBTRACT, lambda x, y: x - y, 78), (abi.OP_MULTIPLY, lambda x, y: x * y, 90),
           (abi.OP_DIVIDE, lambda x, y: x / y, 102), (abi.OP_MODULUS, fmod_exact, 114)]
    for op, fn, line in ops:
        for k, (x, y) in enumerate([(a, a), (a, b), (b, a), (b, b)]):
            out.append(("TestDoubleOperators.java:%d" % (line + k), call(op, abi.DOUBLE, dbl(x), dbl(y)), val(ieee(fn(F(x), F(y))))))
        out.append(("TestDoubleOperators.java:%d" % (line + 4), call(op, abi.DOUBLE, dbl(NAN), dbl(a)), val(NAN)))
        out.append(("TestDoubleOperators.java:%d" % (line + 5), call(op, abi.DOUBLE, dbl(a), dbl(NAN)), val(NAN)))
        out.append(("TestDoubleOperators.java:%d" % (line + 6), call(op, abi.DOUBLE, dbl(NAN), dbl(NAN)), val(NAN)))
    out.append(("TestDoubleOperators.java:126", -dbl(a), val(-37.7)))
    out.append(("TestDoubleOperators.java:128", -dbl(NAN), val(NAN)))
    for line, e, want in [(139, dbl(NAN).eq(dbl(a)), False), (141, dbl(NAN).eq(dbl(NAN)), False), (151, dbl(NAN).ne(dbl(a)), True),
                          (153, dbl(NAN).ne(dbl(NAN)), True), (163, dbl(NAN) < dbl(a), False), (164, dbl(a) < dbl(NAN), False),
                          (177, dbl(NAN) <= dbl(NAN), False), (188, dbl(a) > dbl(NAN), False), (201, dbl(NAN) >= dbl(NAN), False),
                          (219, dbl(NAN).between(dbl(b), dbl(a)), False), (220, dbl(b).between(dbl(NAN), dbl(NAN)), False),
                          (222, dbl(b).between(dbl(b), dbl(NAN)), False), (223, dbl(NAN).between(dbl(NAN), dbl(NAN)), False)]:
        out.append(("TestDoubleOperators.java:%d" % line, e, val(want)))
    out.append(("TestDoubleOperators.java:269", dbl(NAN).cast(abi.REAL), val(NAN)))
    return out


MAX64, MIN64, MAX32, MIN32 = M.I64_MAX, M.I64_MIN, M.I32_MAX, M.I32_MIN
KATS = [
    # TT/TestBigintOperators.java
    ("TestBigintOperators.java:62", big(37) + big(100000000037), val(100000000074)),
    ("TestBigintOperators.java:65", big(100000000017) + big(100000000017), val(200000000034)),
    ("TestBigintOperators.java:72", big(37) - big(100000000017), val(-99999999980)),
    ("TestBigintOperators.java:80", big(100000000037) * big(37), val(3700000001369)),
    ("TestBigintOperators.java:83", big(100000000017) * big(10000017), val(1000001700170000289)),
    ("TestBigintOperators.java:89", big(100000000037) / big(37), val(2702702703)),
    ("TestBigintOperators.java:90", big(37) / big(100000000017), val(0)),
    ("TestBigintOperators.java:98", big(100000000037) % big(37), val(26)),
    ("TestBigintOperators.java:99", big(37) % big(100000000017), val(37)),
    ("TestBigintOperators.java:100", big(100000000017) % big(37), val(6)),
    ("TestBigintOperators.java:107", -big(100000000037), val(-100000000037)),
    ("TestBigintOperators.java:114", big(100000000037).eq(big(100000000037)), val(True)),
    ("TestBigintOperators.java:115", big(37).eq(big(100000000017)), val(False)),
    ("TestBigintOperators.java:199", big(100000000017).cast(abi.DOUBLE), val(100000000017.0)),
    ("TestBigintOperators.java:206", big(-100000000017).cast(abi.REAL), val(-99999997952.0)),   # the float nearest -100000000017
    ("TestBigintOperators.java:238", big(MAX64) + big(1), OVERFLOW),
    ("TestBigintOperators.java:244", big(MIN64) - big(1), OVERFLOW),
    ("TestBigintOperators.java:250", big(MAX64) * big(2), OVERFLOW),
    ("TestBigintOperators.java:251", big(MIN64) * big(-1), OVERFLOW),
    ("TestBigintOperators.java:257", big(MIN64) / big(-1), OVERFLOW),
    ("TestBigintOperators.java:272", -big(MIN64), OVERFLOW),
    # TT/TestIntegerOperators.java
    ("TestIntegerOperators.java:62", i32(37) + i32(17), val(54)),
    ("TestIntegerOperators.java:65", i32(MAX32) + i32(1), OVERFLOW),
    ("TestIntegerOperators.java:73", i32(17) - i32(37), val(-20)),
    ("TestIntegerOperators.java:75", i32(MIN32) - i32(1), OVERFLOW),
    ("TestIntegerOperators.java:82", i32(37) * i32(17), val(629)),
    ("TestIntegerOperators.java:85", i32(MAX32) * i32(2), OVERFLOW),
    ("TestIntegerOperators.java:92", i32(37) / i32(17), val(2)),
    ("TestIntegerOperators.java:93", i32(17) / i32(37), val(0)),
    ("TestIntegerOperators.java:95", i32(17) / i32(0), DIV0),
    ("TestIntegerOperators.java:102", i32(37) % i32(17), val(3)),
    ("TestIntegerOperators.java:105", i32(17) % i32(0), DIV0),
    ("TestIntegerOperators.java:111", -i32(37), val(-37)),
    ("TestIntegerOperators.java:113", -i32(MAX32), val(MIN32 + 1)),
    ("TestIntegerOperators.java:114", -i32(MIN32), OVERFLOW),
    ("TestIntegerOperators.java:121", i32(37).eq(i32(17)), val(False)),
    ("TestIntegerOperators.java:130", i32(37).ne(i32(17)), val(True)),
    ("TestIntegerOperators.java:140", i32(17) < i32(37), val(True)),
    ("TestIntegerOperators.java:147", i32(37) <= i32(37), val(True)),
    ("TestIntegerOperators.java:157", i32(37) > i32(17), val(True)),
    ("TestIntegerOperators.java:167", i32(17) >= i32(37), val(False)),
    ("TestIntegerOperators.java:175", i32(37).between(i32(37), i32(17)), val(False)),
    ("TestIntegerOperators.java:177", i32(37).between(i32(17), i32(37)), val(True)),
    ("TestIntegerOperators.java:180", i32(17).between(i32(37), i32(37)), val(False)),
    ("TestIntegerOperators.java:190", i32(37).cast(abi.BIGINT), val(37)),
    ("TestIntegerOperators.java:218", i32(37).cast(abi.DOUBLE), val(37.0)),
    ("TestIntegerOperators.java:226", i32(MIN32).cast(abi.REAL), val(-2147483648.0)),
    ("TestIntegerOperators.java:227", i32(0).cast(abi.REAL), val(0.0)),
    # by hand from TM/type/IntegerOperators.java:81-101 (the reference's tests do not hold these): a plain long division, no range check
    ("IntegerOperators.java:81-89 MIN / -1", i32(MIN32) / i32(-1), val(2147483648)),
    ("IntegerOperators.java:93-101 MIN % -1", i32(MIN32) % i32(-1), val(0)),
    ("IntegerOperators.java:81-89 MIN / 1", i32(MIN32) / i32(1), val(MIN32)),
    ("IntegerOperators.java:81-89 -7 / 2 truncates", i32(-7) / i32(2), val(-3)),
    ("IntegerOperators.java:93-101 -7 % 2 keeps the dividend's sign", i32(-7) % i32(2), val(-1)),
    # TT/TestRealOperators.java
    ("TestRealOperators.java:60", real(-0.0) + real(0.0), val(0.0)),
    ("TestRealOperators.java:72", real(-0.0) - real(0.0), val(-0.0)),
    ("TestRealOperators.java:84", real(-0.0) * real(0.0), val(-0.0)),
    ("TestRealOperators.java:85", real(-17.71) * real(-1.0), val(float(np.float32(17.71)))),
    ("TestRealOperators.java:97", real(-0.0) / real(0.0), val(NAN)),
    ("TestRealOperators.java:110", real(-0.0) % real(0.0), val(NAN)),
    ("TestRealOperators.java:123", -real(NAN), val(NAN)),
    ("TestRealOperators.java:135", real(NAN).eq(real(1.23)), val(False)),
    ("TestRealOperators.java:269", real(754.1985).cast(abi.DOUBLE), val(float(np.float32(754.1985)))),
    ("TestRealOperators.java:272", real(-0.0).cast(abi.DOUBLE), val(-0.0)),
    ("TestRealOperators.java:273", real(754.1985).cast(abi.DOUBLE).cast(abi.REAL), val(float(np.float32(754.1985)))),
    ("TestRealOperators.java:274", real(NAN).cast(abi.DOUBLE), val(NAN)),
] + real_kats() + double_kats()


def same(t, got, want):
    if got[0] != want[0]:
        return False
    if got[0] == "error":
        return got[1] == want[1]
    return M.bits(t, got[1] if not isinstance(got[1], np.floating) else float(got[1])) == M.bits(t, want[1])


@pytest.mark.parametrize("source,expr,want", KATS, ids=[k[0] for k in KATS])
def test_model_reproduces_the_reference_answers(source, expr, want):
    got = M.outcome(expr, ())
    assert same(expr.type, got, want), (source, got, want)


def test_block_write_narrows_integer():
    """IntegerOperators.java:81-89 leaves 2147483648; the INTEGER block holds (int) of it"""
    assert M.write(abi.INTEGER, M.evaluate(i32(MIN32) / i32(-1), ())) == MIN32


def test_integer_conversions_round_once():
    """Java (float) long and (double) long round once; numpy.float32(int) goes through a double and is not used by the model where that
    differs.  Expected values by hand: the neighbours of n in the format and the distance to each."""
    assert float(M.long_to_float(2 ** 24 + 1)) == 2.0 ** 24                       # tie between 2^24 and 2^24 + 2: even
    assert float(M.long_to_float(2 ** 24 + 3)) == 2.0 ** 24 + 4                   # tie between +2 and +4: even mantissa
    assert M.long_to_double(2 ** 53 + 1) == 2.0 ** 53
    assert M.long_to_double(2 ** 53 + 3) == 2.0 ** 53 + 4
    assert M.long_to_double(2 ** 63 - 1) == 2.0 ** 63 and float(M.long_to_float(2 ** 63 - 1)) == 2.0 ** 63
    assert M.long_to_double(-2 ** 63) == -2.0 ** 63
    n = 2 ** 60 + 2 ** 36 + 1                                                       # just above the midpoint of 2^60 and 2^60 + 2^37
    assert float(M.long_to_float(n)) == 2.0 ** 60 + 2.0 ** 37
    assert float(np.float32(float(n))) == 2.0 ** 60                                 # what two roundings give: why the model rounds by hand


def test_page_level_order_and_laziness():
    from presto_amd.expr import field
    a, b = field(0, abi.BIGINT), field(1, abi.BIGINT)
    rows = [(1, 1), (2, 0), (3, 1), (M.I64_MAX, 1)]
    # a projection error on a row the filter rejected is not raised
    assert M.page(b.ne(big(0)), [a / b], rows[:3]) == [(1,), (3,)]
    with pytest.raises(M.ModelError) as e:
        M.page(None, [a / b], rows)
    assert e.value.status == M.DIVISION_BY_ZERO
    # the filter runs over every row before any projection: its error on the last row wins over the projection's on the second
    with pytest.raises(M.ModelError) as e:
        M.page((a + big(1)) > big(0), [a / b], rows)
    assert e.value.status == M.OUT_OF_RANGE
    # projections in turn: the first projection's error on a late row wins over the second's on an early row
    with pytest.raises(M.ModelError) as e:
        M.page(None, [a + big(1), a / b], rows)
    assert e.value.status == M.OUT_OF_RANGE


# ---- coverage, on the model alone ----------------------------------------------------------------------------------------------------------
MODELLED = [c for c in M.CELLS if c.modelled]


@pytest.mark.parametrize("cell", MODELLED, ids=[c.name for c in MODELLED])
def test_cell_coverage(cell):
    values, errors = M.split_rows(cell)
    statuses = {s for _, s in errors}
    assert statuses == set(cell.raises), (cell.name, statuses)            # one row at least per status the reference can raise, and no other
    if cell.kind in ("arith", "compare", "cast"):
        # (BOOLEAN's operand list is its whole domain: a unary BOOLEAN cell has three rows, all of which must then be values)
        need = 8 if set(cell.columns) != {"BOOLEAN"} else min(8, 3 ** len(cell.columns))
        assert len(values) >= need, (cell.name, len(values))
        assert any(v is None for _, v in values) and any(v is not None for _, v in values)


def test_cells_are_unique_and_every_operator_is_listed():
    assert len({c.name for c in M.CELLS}) == len(M.CELLS)
    for label, _ in M.ARITH_OPS:
        for name in ("BIGINT", "INTEGER", "DATE", "DOUBLE", "REAL", "DECIMAL"):
            assert "%s:%s" % (label, name) in M.CELL
    for label, _ in M.COMPARE_OPS:
        for name in M.ALL_TYPES:
            assert "%s:%s" % (label, name) in M.CELL
    for form in ("and:BOOLEAN", "or:BOOLEAN", "not:BOOLEAN"):
        assert form in M.CELL
    for form in ("is_null", "between", "in", "coalesce", "if"):
        for name in M.ALL_TYPES:
            assert "%s:%s" % (form, name) in M.CELL


# ---- the C oracle agrees with the model on every cell ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", MODELLED, ids=[c.name for c in MODELLED])
def test_oracle_agrees_with_the_model(oracle, cell):
    values, errors = M.split_rows(cell)
    rows = [r for r, _ in values]
    out = oracle.filter_project(M.page_of(cell.columns, rows), None, [cell.expr])
    got = [r[0] for r in out.to_rows()]
    want = [v for _, v in values]
    assert len(got) == len(want)
    wrong = [(r, g, w) for r, g, w in zip(rows, got, want) if M.bits(cell.out_type, g) != M.bits(cell.out_type, w)]
    assert not wrong, (cell.name, len(wrong), wrong[:5])
    benign = [r for r in rows if all(v is not None for v in r)][:3]
    for r, status in errors:                                                   # each raising row alone among benign rows
        with pytest.raises(oracle.OracleError) as e:
            oracle.filter_project(M.page_of(cell.columns, benign[:2] + [r] + benign[2:]), None, [cell.expr])
        assert e.value.status == status, (cell.name, r, e.value.status, status)
