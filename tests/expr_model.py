"""An independent statement of the expression semantics the device code generator (csrc/exprgen.cpp) and the C oracle
(oracle/presto_oracle.c) both restate: an interpreter over presto_amd.expr.RowExpression trees in exact Python arithmetic, written from
the reference's *Operators.java and sql/gen/*CodeGenerator.java.  Neither C side was consulted; where the three disagree, one of the C
sides is wrong (or the disagreement is a documented divergence of DESIGN.md section 5).

Citations: TM = core/trino-main/src/main/java/io/trino, SPI = core/trino-spi/src/main/java/io/trino/spi.

Values, one row at a time
  BIGINT / INTEGER / DATE / DECIMAL   Python int (a DECIMAL is its unscaled value)
  DOUBLE                              Python float
  REAL                                numpy.float32 at every step
  BOOLEAN                             bool
  VARCHAR                             bytes
  NULL                                None
An evaluation returns a value or raises ModelError(status) with the status of the C ABI.

Rules
  BIGINT arithmetic    Math.*Exact, NUMERIC_VALUE_OUT_OF_RANGE on overflow (TM/type/BigintOperators.java:47-79, :110-118); divide has an
                       explicit MIN / -1 check before the division (:83-94); modulus has none, MIN % -1 = 0 (:98-106); a zero divisor is
                       DIVISION_BY_ZERO; both truncate toward zero (Java `/`, `%`).
  INTEGER arithmetic   add / subtract / multiply / negate are Math.*Exact on the operands narrowed to int (TM/type/IntegerOperators.java
                       :45-77, :105-113); divide and modulus are plain long operations with no range check (:81-101): MIN / -1 is
                       2147483648, carried on as a long.  DATE follows the INTEGER rules (the device accepts DATE arithmetic as such).
  INTEGER comparisons  EQUAL compares the longs (SPI/type/AbstractIntType.java:135-139); LESS_THAN / LESS_THAN_OR_EQUAL compare the
                       operands narrowed to int (:159-169); the other three are derived from these (NOT EQUAL, swapped operands).
  DOUBLE               Java double arithmetic, % = fmod (TM/type/DoubleOperators.java:61-99).
  REAL                 Java float arithmetic, % = fmodf (TM/type/RealOperators.java:57-95).
  fp comparisons       Java primitive comparisons (SPI/type/DoubleType.java:157-210, RealType.java:101-158): NaN is unequal to
                       everything and unordered, -0.0 == 0.0.
  other comparisons    longs (AbstractLongType.java:132-166, ShortDecimalType.java:121-155), BOOLEAN false < true (BooleanType.java
                       :145-173), VARCHAR by unsigned bytes with a proper prefix first (VarcharType.java:229-233, Slice.compareTo).
  casts                Java primitive conversions: long -> double / float round once to nearest even (BigintOperators.java:186-196,
                       IntegerOperators.java:155-165), float -> double is exact (RealOperators.java:166), double -> float rounds once
                       and overflows to +-inf (DoubleOperators.java:167), BIGINT -> INTEGER is toIntExact (BigintOperators.java:129-137),
                       INTEGER -> BIGINT the value (IntegerOperators.java:117-120).
  short DECIMAL        add / subtract rescale to the larger scale and add the longs (TM/type/DecimalOperators.java:103, :203), multiply
                       multiplies them (:276), negate (:642); the derived result precision cannot overflow.  Casts: integer -> decimal is
                       multiplyExact(value, 10^scale) with the 10^precision bound (TM/type/DecimalCasts.java:208-220, :266-278), decimal ->
                       decimal rescales, a division rounding half away from zero, then the bound (SPI/type/DecimalConversions.java
                       :173-203).  The reference raises INVALID_CAST_ARGUMENT; the C ABI has no such status and reports
                       NUMERIC_VALUE_OUT_OF_RANGE.
  calls                arguments are evaluated left to right; a NULL argument makes the result NULL and the arguments after it are not
                       evaluated (TM/sql/gen/BytecodeUtils.java:300-304).
  AND / OR             left to right; a deciding operand hides the operands after it, a NULL one does not (AndCodeGenerator.java:44-105,
                       OrCodeGenerator.java:44-104).
  IF                   a NULL condition takes the else branch; the untaken branch is not evaluated (IfCodeGenerator.java:47-62).
  COALESCE             arguments after the first non-NULL one are not evaluated (CoalesceCodeGenerator.java:46-75).
  BETWEEN              the value is evaluated once; a NULL value is the result; else AND(min <= value, value <= max)
                       (BetweenCodeGenerator.java:59-82).
  IN                   a NULL value gives NULL; candidates are tested in order until one matches; no match with a NULL candidate gives
                       NULL (InCodeGenerator.java:256-283, :290-360).
  page                 the filter is evaluated for every row, then each projection in turn over the selected rows; the page fails with
                       the first error in that order (TM/operator/project/PageProcessor.java, TM/sql/gen/PageFunctionCompiler.java:459-544).
  block write          INTEGER / DATE are narrowed to 32 bits (SPI/type/AbstractIntType.java writeLong: (int) value).

LONG_DECIMAL arithmetic and casts are pinned against the reference's own values by tests/test_gpu_decimal.py and
tests/test_oracle_decimal.py and are not restated; its comparisons, IS NULL, IF, COALESCE, BETWEEN and IN are (plain integer compares).
"""
import collections
import itertools
import math
import struct

import numpy as np

from presto_amd import abi
from presto_amd.expr import call, coalesce, decimal_result_type, field, if_, not_, special

OUT_OF_RANGE = abi.ERR_NUMERIC_VALUE_OUT_OF_RANGE
DIVISION_BY_ZERO = abi.ERR_DIVISION_BY_ZERO
INVALID_CAST_ARGUMENT = abi.ERR_NUMERIC_VALUE_OUT_OF_RANGE   # the ABI's status for the reference's INVALID_CAST_ARGUMENT

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1


class ModelError(Exception):
    def __init__(self, status):
        super().__init__(abi.STATUS_NAMES.get(status, status))
        self.status = status


# ---- primitives ---------------------------------------------------------------------------------------------------------------------------
def to_int(v):
    """Java (int) value: the low 32 bits, signed."""
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >> 31 else v


def java_div(a, b):
    """Java long division: truncates toward zero (Python's // floors)."""
    q = abs(a) // abs(b)
    return -q if (a < 0) != (b < 0) else q


def java_rem(a, b):
    """Java long remainder: the sign of the dividend."""
    r = abs(a) % abs(b)
    return -r if a < 0 else r


def exact(v, lo, hi):
    if v < lo or v > hi:
        raise ModelError(OUT_OF_RANGE)
    return v


def round_int(n, mantissa_bits):
    """The integer nearest to n that has at most mantissa_bits significant bits, ties to even: one rounding, as Java's (double) long and
    (float) long.  The result converts to the floating type exactly."""
    m = abs(n)
    shift = m.bit_length() - mantissa_bits
    if shift <= 0:
        return n
    q, rem = m >> shift, m & ((1 << shift) - 1)
    half = 1 << (shift - 1)
    if rem > half or (rem == half and (q & 1)):
        q += 1
    m = q << shift
    return -m if n < 0 else m


def long_to_double(n):
    return float(round_int(n, 53))


def long_to_float(n):
    return np.float32(float(round_int(n, 24)))   # exact in a double, then exact in a float: numpy.float32(int) alone goes through a double


def is_fp(t):
    return t in (abi.DOUBLE, abi.REAL)


def is_int(t):
    return t in (abi.BIGINT, abi.INTEGER, abi.DATE)


def is_decimal(t):
    return t in (abi.DECIMAL, abi.LONG_DECIMAL)


def scale_of(t):
    return t.scale if isinstance(t, abi.DecimalType) else 0


# ---- operators ----------------------------------------------------------------------------------------------------------------------------
def arith(op, t, a, b=None):
    if t == abi.BIGINT:
        if op == abi.OP_ADD: return exact(a + b, I64_MIN, I64_MAX)
        if op == abi.OP_SUBTRACT: return exact(a - b, I64_MIN, I64_MAX)
        if op == abi.OP_MULTIPLY: return exact(a * b, I64_MIN, I64_MAX)
        if op == abi.OP_NEGATE: return exact(-a, I64_MIN, I64_MAX)
        if op == abi.OP_DIVIDE:
            if a == I64_MIN and b == -1:      # checked before the division, so also before the zero check -- but b is -1 here
                raise ModelError(OUT_OF_RANGE)
            if b == 0:
                raise ModelError(DIVISION_BY_ZERO)
            return java_div(a, b)
        if op == abi.OP_MODULUS:
            if b == 0:
                raise ModelError(DIVISION_BY_ZERO)
            return java_rem(a, b)
    if t in (abi.INTEGER, abi.DATE):
        if op == abi.OP_ADD: return exact(to_int(a) + to_int(b), I32_MIN, I32_MAX)
        if op == abi.OP_SUBTRACT: return exact(to_int(a) - to_int(b), I32_MIN, I32_MAX)
        if op == abi.OP_MULTIPLY: return exact(to_int(a) * to_int(b), I32_MIN, I32_MAX)
        if op == abi.OP_NEGATE: return exact(-to_int(a), I32_MIN, I32_MAX)
        if op in (abi.OP_DIVIDE, abi.OP_MODULUS):   # plain long operations: no range check, MIN / -1 = 2147483648 is carried on
            if b == 0:
                raise ModelError(DIVISION_BY_ZERO)
            return java_div(a, b) if op == abi.OP_DIVIDE else java_rem(a, b)
    if t == abi.DOUBLE:
        return float(fp_arith(op, np.float64(a), None if b is None else np.float64(b)))
    if t == abi.REAL:
        return np.float32(fp_arith(op, np.float32(a), None if b is None else np.float32(b)))
    if t == abi.DECIMAL:
        if op == abi.OP_NEGATE: return -a
        if op == abi.OP_MULTIPLY: return a * b
        if op in (abi.OP_ADD, abi.OP_SUBTRACT):
            return a + b if op == abi.OP_ADD else a - b    # (the operands arrive rescaled: see evaluate)
    raise NotImplementedError((op, t))


def fp_arith(op, a, b):
    with np.errstate(all="ignore"):
        if op == abi.OP_ADD: return a + b
        if op == abi.OP_SUBTRACT: return a - b
        if op == abi.OP_MULTIPLY: return a * b
        if op == abi.OP_DIVIDE: return a / b
        if op == abi.OP_MODULUS:
            if isinstance(a, np.float32):
                return np.fmod(a, b)
            try:
                return math.fmod(a, b)
            except ValueError:           # Python raises where IEEE fmod (and Java's %) gives NaN: an infinite dividend, a zero divisor
                return float("nan")
        if op == abi.OP_NEGATE: return -a
    raise NotImplementedError(op)


def compare(op, t, a, b):
    if t in (abi.INTEGER, abi.DATE):
        eq, lt, le = a == b, to_int(a) < to_int(b), to_int(a) <= to_int(b)
        gt, ge = to_int(b) < to_int(a), to_int(b) <= to_int(a)
    elif is_fp(t):
        a, b = float(a), float(b)    # a float widens exactly: the comparison of the widened values is the float comparison
        eq, lt, le, gt, ge = a == b, a < b, a <= b, b < a, b <= a
    elif t == abi.BOOLEAN:
        eq, lt, le, gt, ge = a == b, (not a) and b, (not a) or b, (not b) and a, (not b) or a
    else:                            # longs, unscaled decimals; bytes compare as unsigned bytes with a proper prefix first
        eq, lt, le, gt, ge = a == b, a < b, a <= b, b < a, b <= a
    return {abi.OP_EQUAL: eq, abi.OP_NOT_EQUAL: not eq, abi.OP_LESS_THAN: lt, abi.OP_LESS_THAN_OR_EQUAL: le,
            abi.OP_GREATER_THAN: gt, abi.OP_GREATER_THAN_OR_EQUAL: ge}[op]


def cast(src, dst, v):
    if is_decimal(dst) and (is_int(src) or is_decimal(src)):
        ss, ds = scale_of(src), scale_of(dst)
        if ds >= ss:
            r = v * 10 ** (ds - ss)
            if is_int(src) and not I64_MIN <= r <= I64_MAX and dst == abi.DECIMAL:   # multiplyExact
                raise ModelError(INVALID_CAST_ARGUMENT)
        else:
            f = 10 ** (ss - ds)
            r = java_div(v, f)
            rem = java_rem(v, f)
            if v >= 0 and 2 * rem >= f:
                r += 1
            elif v < 0 and 2 * rem <= -f:
                r -= 1
        if abs(r) >= 10 ** dst.precision:
            raise ModelError(INVALID_CAST_ARGUMENT)
        return r
    if is_int(src):
        if dst == abi.DOUBLE: return long_to_double(v)
        if dst == abi.REAL: return long_to_float(v)
        if dst == abi.BIGINT: return v
        if dst == abi.INTEGER and src == abi.BIGINT:
            return exact(v, I32_MIN, I32_MAX)
    if src == abi.REAL and dst == abi.DOUBLE:
        return float(v)
    if src == abi.DOUBLE and dst == abi.REAL:
        with np.errstate(all="ignore"):
            return np.float32(v)
    if src == dst and scale_of(src) == scale_of(dst):
        return v
    raise NotImplementedError((src, dst))


# ---- the interpreter ----------------------------------------------------------------------------------------------------------------------
def evaluate(e, row):
    """e over one row (a sequence of channel values) -> value | None, or raises ModelError."""
    if e.kind == abi.EXPR_INPUT_REF:
        return row[e.channel]
    if e.kind == abi.EXPR_CONSTANT:
        if e.is_null:
            return None
        return np.float32(e.value) if e.type == abi.REAL else e.value
    if e.kind == abi.EXPR_CALL:
        values = []
        for a in e.args:                 # left to right; a NULL argument ends the call (BytecodeUtils.java:300-304)
            v = evaluate(a, row)
            if v is None:
                return None
            values.append(v)
        t0 = e.args[0].type
        if abi.OP_EQUAL <= e.op <= abi.OP_GREATER_THAN_OR_EQUAL:
            return compare(e.op, t0, values[0], values[1])
        if e.op == abi.OP_NOT:
            return not values[0]
        if e.op == abi.OP_CAST:
            return cast(t0, e.type, values[0])
        if e.type == abi.DECIMAL and e.op in (abi.OP_ADD, abi.OP_SUBTRACT):
            s = scale_of(e.type)
            values = [v * 10 ** (s - scale_of(a.type)) for v, a in zip(values, e.args)]
        return arith(e.op, e.type, *values)
    form = e.op
    if form in (abi.FORM_AND, abi.FORM_OR):
        deciding = form == abi.FORM_OR
        saw_null = False
        for a in e.args:
            v = evaluate(a, row)
            if v is None:
                saw_null = True
            elif bool(v) == deciding:
                return deciding
        return None if saw_null else not deciding
    if form == abi.FORM_IS_NULL:
        return evaluate(e.args[0], row) is None
    if form == abi.FORM_IF:
        c = evaluate(e.args[0], row)
        return evaluate(e.args[1] if c else e.args[2], row)
    if form == abi.FORM_COALESCE:
        for a in e.args:
            v = evaluate(a, row)
            if v is not None:
                return v
        return None
    if form == abi.FORM_BETWEEN:
        t = e.args[0].type
        v = evaluate(e.args[0], row)
        if v is None:
            return None
        lo = evaluate(e.args[1], row)
        c1 = None if lo is None else compare(abi.OP_LESS_THAN_OR_EQUAL, t, lo, v)
        if c1 is False:
            return False
        hi = evaluate(e.args[2], row)
        c2 = None if hi is None else compare(abi.OP_LESS_THAN_OR_EQUAL, t, v, hi)
        if c2 is False:
            return False
        return None if c1 is None or c2 is None else True
    if form == abi.FORM_IN:
        t = e.args[0].type
        v = evaluate(e.args[0], row)
        if v is None:
            return None
        saw_null = False
        for a in e.args[1:]:
            c = evaluate(a, row)
            if c is None:
                saw_null = True
            elif compare(abi.OP_EQUAL, t, v, c):
                return True
        return None if saw_null else False
    raise NotImplementedError(form)


def outcome(e, row):
    """('value', v) or ('error', status)"""
    try:
        return "value", evaluate(e, row)
    except ModelError as err:
        return "error", err.status


def write(t, v):
    """The value as the type's block stores it (and as Page.to_rows gives it back)."""
    if v is None:
        return None
    if t in (abi.INTEGER, abi.DATE):
        return to_int(v)
    if t == abi.REAL:
        return float(v)
    if t == abi.BOOLEAN:
        return bool(v)
    return v


def page(filter_expr, projections, rows):
    """PageProcessor over one page: the output rows, or raises ModelError with the first error in the reference's evaluation order --
    the filter over every row, then each projection in turn over the selected rows."""
    selected = [r for r in rows if filter_expr is None or evaluate(filter_expr, r) is True]
    columns = [[write(p.type, evaluate(p, r)) for r in selected] for p in projections]
    return [tuple(c[i] for c in columns) for i in range(len(selected))]


def bits(t, v):
    """A written value as a bit pattern, NaN as a class (a NaN's payload and sign are not specified by Java arithmetic)."""
    if isinstance(v, float):
        if v != v:
            return "nan"
        return struct.pack("<f" if t == abi.REAL else "<d", v)
    return v


def row_bits(types, row):
    return tuple(bits(t, v) for t, v in zip(types, row))


# ---- operand edges ------------------------------------------------------------------------------------------------------------------------
def f32(v):
    return np.float32(v)


D82 = abi.decimal(8, 2)        # the short DECIMAL of the cells: sums are DECIMAL(9, 2), products DECIMAL(16, 4), all short
LD = abi.decimal(38, 2)
TYPES = {"BIGINT": abi.BIGINT, "INTEGER": abi.INTEGER, "DATE": abi.DATE, "DOUBLE": abi.DOUBLE, "REAL": abi.REAL, "BOOLEAN": abi.BOOLEAN,
         "VARCHAR": abi.VARCHAR, "DECIMAL": D82, "LONG_DECIMAL": LD}

_INT32_EDGES = [0, 1, -1, 2, -2, 3, -3, I32_MIN, I32_MIN + 1, I32_MAX, I32_MAX - 1, 46341, -46341, 46340, -46340, 0x01234567, -0x01234567, 1 << 16]
EDGES = {
    "BIGINT": [0, 1, -1, 2, -2, 3, -3, I64_MIN, I64_MIN + 1, I64_MAX, I64_MAX - 1, 2 ** 31, -2 ** 31, 2 ** 31 + 1, -(2 ** 31 + 1), 2 ** 31 - 1,
               -(2 ** 31 - 1), 46341, -46341, 3037000500, -3037000500, 3037000499, -3037000499],
    "INTEGER": _INT32_EDGES,
    "DATE": _INT32_EDGES + [9000, 19000, -719162],
    "DOUBLE": [0.0, -0.0, float("nan"), float("inf"), float("-inf"), 5e-324, -5e-324, 2.2250738585072014e-308, -2.2250738585072014e-308,
               1.7976931348623157e308, -1.7976931348623157e308, 2.0 ** 53, 2.0 ** 53 + 2, 0.1, 1 / 3, -7.5, 2.5, 1.5, -1.5, 1e-30, 3.4028235677973366e38,
               3.4028234663852886e38, 1e-46, 7e-46, 16777217.0, struct.unpack("<d", struct.pack("<Q", 0x0123456789ABCDEF))[0]],
    "REAL": [f32(v) for v in (0.0, -0.0, float("nan"), float("inf"), float("-inf"), 1e-45, -1e-45, 1.17549435e-38, -1.17549435e-38, 3.4028235e38,
                              -3.4028235e38, 16777216.0, 16777218.0, 0.1, 1 / 3, -7.5, 2.5, 1.5, -1.5, 1e-30, 3e-39)],
    "BOOLEAN": [True, False],
    "VARCHAR": [b"", b"a", b"ab", b"abcdefg", b"abcdefgh", b"abcdefghi", b"abcdefgh\x00", b"abcdefghj", b"\xff\xfe", b"zz" * 10, b"\x00", b"\x7f", b"\x80"],
    "DECIMAL": [0, 1, -1, 2, -2, 3, -3, 10 ** 8 - 1, -(10 ** 8 - 1), 12345, -12345, 12344, -12344, 5, -5, 4, -4, 99999949, 99999950, -99999950, 10 ** 6, -10 ** 6],
    "LONG_DECIMAL": [0, 7, -7, 10 ** 38 - 1, -(10 ** 38 - 1), 1 << 64, -(1 << 64), (1 << 64) + 1, (1 << 64) - 1, 1 << 63, -(1 << 63)],
}
# what only a conversion needs, on top of EDGES: the rounding boundaries of the floating formats
CAST_EDGES = {
    "BIGINT": [2 ** 24 + 1, 2 ** 24 + 3, 2 ** 53 + 1, -(2 ** 53 + 1), 2 ** 53 + 3,
               2 ** 60 + 2 ** 36 + 1,   # rounds up to 2^60 + 2^37 as a float in one step; through a double first it would tie to 2^60
               0x0123456789ABCDEF, -0x0123456789ABCDEF, 1 << 32, -(1 << 32), 10 ** 6 - 1, 10 ** 6, -10 ** 6],
    "INTEGER": [2 ** 24 + 1, -(2 ** 24 + 1), 2 ** 24 + 3, 10 ** 6 - 1, 10 ** 6, -10 ** 6],
}
# the three-operand forms take a cross product of three lists: a subset that keeps every class (zero, sign, extremes, NaN, prefix)
FORM_EDGES = {
    "BIGINT": [0, 1, -1, I64_MIN, I64_MAX, 2 ** 31],
    "INTEGER": [0, 1, -1, I32_MIN, I32_MAX, 46341],
    "DATE": [0, 1, -1, I32_MIN, I32_MAX, 9000],
    "DOUBLE": [0.0, -0.0, float("nan"), float("inf"), float("-inf"), 5e-324, 1.5],
    "REAL": [f32(v) for v in (0.0, -0.0, float("nan"), float("inf"), float("-inf"), 1e-45, 1.5)],
    "BOOLEAN": [True, False],
    "VARCHAR": [b"", b"abcdefg", b"abcdefgh", b"abcdefghi", b"abcdefgh\x00", b"\xff\xfe"],
    "DECIMAL": [0, 1, -1, 10 ** 8 - 1, -(10 ** 8 - 1), 12345],
    "LONG_DECIMAL": [0, 7, -7, 10 ** 38 - 1, -(10 ** 38 - 1), (1 << 64) + 1],
}


def operands(name, small=False, conversion=False):
    """The operand list of a type: its edges (and, for a conversion, the rounding boundaries), then NULL."""
    return list((FORM_EDGES if small else EDGES)[name]) + (CAST_EDGES.get(name, []) if conversion else []) + [None]


# ---- cells --------------------------------------------------------------------------------------------------------------------------------
# A cell is one (operator or form, operand types) pair the ABI can express.  `columns` names the type of each input channel; `expr` takes
# every operand from a channel (never a constant: one compiled kernel then serves every page of the cell); `group` names the cells that
# can share one operator, each over channels of its own (rebase) -- the arithmetic of a type, its comparisons, the casts from one source,
# the special forms of a type; `raises` is the set of statuses the reference can raise from the cell; `modelled` is False where the reference defines no such operator or this module restates none: such a cell must
# be refused by the device.
Cell = collections.namedtuple("Cell", "name kind group columns expr out_type small raises modelled")

ARITH_OPS = [("add", abi.OP_ADD), ("subtract", abi.OP_SUBTRACT), ("multiply", abi.OP_MULTIPLY), ("divide", abi.OP_DIVIDE), ("modulus", abi.OP_MODULUS),
             ("negate", abi.OP_NEGATE)]
COMPARE_OPS = [("eq", abi.OP_EQUAL), ("ne", abi.OP_NOT_EQUAL), ("lt", abi.OP_LESS_THAN), ("le", abi.OP_LESS_THAN_OR_EQUAL), ("gt", abi.OP_GREATER_THAN),
               ("ge", abi.OP_GREATER_THAN_OR_EQUAL)]
ALL_TYPES = ["BIGINT", "INTEGER", "DATE", "DOUBLE", "REAL", "BOOLEAN", "VARCHAR", "DECIMAL", "LONG_DECIMAL"]


def _arith_raises(op, name):
    if name in ("BIGINT", "INTEGER", "DATE"):
        if op == abi.OP_MODULUS or (op == abi.OP_DIVIDE and name != "BIGINT"):
            return {DIVISION_BY_ZERO}
        if op == abi.OP_DIVIDE:
            return {DIVISION_BY_ZERO, OUT_OF_RANGE}
        return {OUT_OF_RANGE}
    return set()


def _build_cells():
    cells = []

    def add(name, kind, columns, expr, small=False, raises=(), modelled=True, group=None):
        cells.append(Cell(name, kind, group or name, tuple(columns), expr, expr.type, small, frozenset(raises), modelled))

    def fields(*names):
        return [field(i, TYPES[n]) for i, n in enumerate(names)]

    # arithmetic: same-typed operands; LONG_DECIMAL arithmetic is pinned elsewhere (module docstring)
    for name in ["BIGINT", "INTEGER", "DATE", "DOUBLE", "REAL", "DECIMAL", "BOOLEAN", "VARCHAR"]:
        t = TYPES[name]
        for label, op in ARITH_OPS:
            modelled = name not in ("BOOLEAN", "VARCHAR") and not (name == "DECIMAL" and op in (abi.OP_DIVIDE, abi.OP_MODULUS))
            if op == abi.OP_NEGATE:
                a, = fields(name)
                add("%s:%s" % (label, name), "arith", [name], call(op, t, a), raises=_arith_raises(op, name), modelled=modelled, group="arith:" + name)
                continue
            a, b = fields(name, name)
            rt = decimal_result_type(op, t, t) if name == "DECIMAL" and modelled else t
            add("%s:%s" % (label, name), "arith", [name, name], call(op, rt, a, b), raises=_arith_raises(op, name), modelled=modelled, group="arith:" + name)
    # mixed operands need an explicit CAST: the planner never emits them, the ABI can express them
    for left, right in [("BIGINT", "DOUBLE"), ("DOUBLE", "BIGINT"), ("REAL", "DOUBLE"), ("DECIMAL", "BIGINT")]:
        for label, op in ARITH_OPS[:5]:
            a, b = fields(left, right)
            add("%s:%s,%s" % (label, left, right), "arith", [left, right], call(op, TYPES[left], a, b), modelled=False)
    # comparisons
    for name in ALL_TYPES:
        a, b = fields(name, name)
        for label, op in COMPARE_OPS:
            add("%s:%s" % (label, name), "compare", [name, name], call(op, abi.BOOLEAN, a, b), group="compare:" + name)
    for left, right in [("BIGINT", "DOUBLE"), ("REAL", "DOUBLE"), ("VARCHAR", "BIGINT")]:
        a, b = fields(left, right)
        add("eq:%s,%s" % (left, right), "compare", [left, right], call(abi.OP_EQUAL, abi.BOOLEAN, a, b), modelled=False)
    add("not:BOOLEAN", "not", ["BOOLEAN"], not_(field(0, abi.BOOLEAN)), group="form:BOOLEAN")
    # casts, source -> target
    D61, D124 = abi.decimal(6, 1), abi.decimal(12, 4)
    casts = {
        "BIGINT": [("BIGINT", abi.BIGINT, ()), ("DOUBLE", abi.DOUBLE, ()), ("REAL", abi.REAL, ()), ("INTEGER", abi.INTEGER, {OUT_OF_RANGE}),
                   ("DECIMAL(8,2)", D82, {INVALID_CAST_ARGUMENT})],
        "INTEGER": [("BIGINT", abi.BIGINT, ()), ("DOUBLE", abi.DOUBLE, ()), ("REAL", abi.REAL, ()), ("INTEGER", abi.INTEGER, ()),
                    ("DECIMAL(8,2)", D82, {INVALID_CAST_ARGUMENT})],
        "DATE": [("BIGINT", abi.BIGINT, ()), ("DOUBLE", abi.DOUBLE, ()), ("DATE", abi.DATE, ())],
        "DOUBLE": [("REAL", abi.REAL, ()), ("DOUBLE", abi.DOUBLE, ())],
        "REAL": [("DOUBLE", abi.DOUBLE, ()), ("REAL", abi.REAL, ())],
        "DECIMAL": [("DECIMAL(8,2)", D82, ()), ("DECIMAL(12,4)", D124, ()), ("DECIMAL(6,1)", D61, {INVALID_CAST_ARGUMENT})],
        "BOOLEAN": [("BOOLEAN", abi.BOOLEAN, ())],
        "VARCHAR": [("VARCHAR", abi.VARCHAR, ())],
    }
    for src, targets in casts.items():
        for label, t, raises in targets:
            a, = fields(src)
            add("cast:%s->%s" % (src, label), "cast", [src], a.cast(t), raises=raises, group="cast:" + src)
    # casts the reference has and this module does not restate (the device must refuse them), and casts it does not have
    for src, label, t in [("DOUBLE", "BIGINT", abi.BIGINT), ("DOUBLE", "INTEGER", abi.INTEGER), ("REAL", "BIGINT", abi.BIGINT), ("BIGINT", "BOOLEAN", abi.BOOLEAN),
                          ("BIGINT", "VARCHAR", abi.VARCHAR), ("BOOLEAN", "BIGINT", abi.BIGINT), ("VARCHAR", "BIGINT", abi.BIGINT), ("INTEGER", "DATE", abi.DATE),
                          ("DATE", "INTEGER", abi.INTEGER), ("DOUBLE", "DECIMAL(8,2)", D82), ("DECIMAL", "DOUBLE", abi.DOUBLE), ("DECIMAL", "BIGINT", abi.BIGINT)]:
        a, = fields(src)
        add("cast:%s->%s" % (src, label), "cast", [src], a.cast(t), modelled=False)
    # the seven special forms
    a, b = fields("BOOLEAN", "BOOLEAN")
    add("and:BOOLEAN", "form", ["BOOLEAN", "BOOLEAN"], special(abi.FORM_AND, abi.BOOLEAN, a, b), group="form:BOOLEAN")
    add("or:BOOLEAN", "form", ["BOOLEAN", "BOOLEAN"], special(abi.FORM_OR, abi.BOOLEAN, a, b), group="form:BOOLEAN")
    for name in ALL_TYPES:
        t = TYPES[name]
        a, = fields(name)
        g = "form:" + name
        add("is_null:%s" % name, "form", [name], a.is_null_(), group=g)
        a, b, c = fields(name, name, name)
        add("between:%s" % name, "form", [name] * 3, a.between(b, c), small=True, group=g)
        add("in:%s" % name, "form", [name] * 3, a.isin(b, c), small=True, group=g)
        a, b = fields(name, name)
        add("coalesce:%s" % name, "form", [name] * 2, coalesce(a, b), small=True, group=g)
        add("if:%s" % name, "form", ["BOOLEAN", name, name], if_(field(0, abi.BOOLEAN), field(1, t), field(2, t)), small=True, group=g)
    return cells


CELLS = _build_cells()
CELL = {c.name: c for c in CELLS}
assert len(CELL) == len(CELLS)
GROUPS = collections.OrderedDict()
for _c in CELLS:
    GROUPS.setdefault(_c.group, []).append(_c)


def cell_rows(cell):
    """The cell's operand rows: the cross product of the operand lists of its channels, NULL included."""
    return [tuple(r) for r in itertools.product(*[operands(n, cell.small, cell.kind == "cast") for n in cell.columns])]


def rebase(e, offset):
    """e with every input channel moved up by `offset`: the same expression over channels of its own inside a wider page"""
    from presto_amd.expr import RowExpression
    return RowExpression(e.kind, e.type, e.op, [rebase(a, offset) for a in e.args], e.channel + offset if e.kind == abi.EXPR_INPUT_REF else e.channel,
                         e.value, e.is_null)


def block_of(name, values):
    from presto_amd.page import Block
    nulls = [v is None for v in values]
    if name == "VARCHAR":
        return Block.varchar(values)
    if name == "LONG_DECIMAL":
        return Block.long_decimal(values)
    if name == "BOOLEAN":
        return Block.boolean([bool(v) for v in values], nulls)
    return Block.flat(TYPES[name], [0 if v is None else v for v in values], nulls)


def always_nullable(block):
    """the block with a valueIsNull array even when no position is NULL: kernels are generated per column-layout signature, and the pages
    of one cell should all have the same"""
    if block.nulls is None:
        block.nulls = np.zeros(block.position_count, dtype=np.uint8)
    return block


def page_of(columns, rows, nullable=False):
    """rows of operand values -> a host Page with one channel per name in `columns`"""
    from presto_amd.page import Page
    blocks = [block_of(n, [r[i] for r in rows]) for i, n in enumerate(columns)]
    return Page([always_nullable(b) for b in blocks] if nullable else blocks, len(rows))


def input_types(columns):
    return [TYPES[n] for n in columns]


def split_rows(cell, rows=None):
    """(value rows with their written values, raising rows with their status)"""
    values, errors = [], []
    for r in cell_rows(cell) if rows is None else rows:
        kind, v = outcome(cell.expr, r)
        if kind == "value":
            values.append((r, write(cell.out_type, v)))
        else:
            errors.append((r, v))
    return values, errors
