"""An independent statement of the six aggregates (count(*), count, sum, avg, min, max) the fused aggregation kernels, the host assembly
behind them (csrc/op_fused_output.cpp, csrc/decimal_host.hpp) and the C oracle (oracle/presto_oracle.c) all restate: plain Python over
one group's value list, written from the reference's aggregation functions.  Neither C side was consulted; where the three disagree, one
of the C sides is wrong or the disagreement is a row of DIVERGENCES.

Citations: AGG = core/trino-main/src/main/java/io/trino/operator/aggregation, TM = core/trino-main/src/main/java/io/trino,
SPI = core/trino-spi/src/main/java/io/trino/spi.

Values of one group, in row order (None = NULL): Python int for BIGINT / INTEGER / DATE and for a DECIMAL's unscaled value, float for
DOUBLE, numpy.float32 for REAL, bool for BOOLEAN, bytes for VARCHAR.

Rules
  mask, NULL        a row counts when its mask is true (NULL mask = false, TM/sql/gen/CompilerOperations.java:65-74), then, for every
                    aggregate but count(*), when its value is not NULL (AGG/AccumulatorCompiler.java:490-569).  A group none of whose
                    rows counts has count 0 and NULL everywhere else.
  count(*) / count  AGG/CountAggregation.java:33-55, AGG/CountColumn.java:124-142: BIGINT.
  sum(BIGINT)       Math.addExact in row order (AGG/LongSumAggregation.java:34-64 through TM/type/BigintOperators.java:47-55): BIGINT.
  sum(INTEGER)      the reference has none: its analyzer casts to BIGINT first and LongSumAggregation adds.  This project's ABI keeps an
                    INTEGER result column, so the model is sum(CAST(x AS BIGINT)) followed by the column's range: a total outside int32
                    is NUMERIC_VALUE_OUT_OF_RANGE (`agg-integer-sum-column`).
  sum(DOUBLE)       a double running sum from +0.0 in row order (AGG/DoubleSumAggregation.java:33-63): DOUBLE.
  sum(REAL)         the same over the widened floats; the result is (float) sum (AGG/RealSumAggregation.java:35-67): REAL.
  avg(BIGINT / INTEGER / DOUBLE)   a double running sum of (double) value, divided by (double) count (AGG/AverageAggregations.java:34-80).
  avg(REAL)         double sum of the widened floats; (float) (sum / count) (AGG/RealAverageAggregation.java:132-157): REAL.
  sum(DECIMAL(p, s))   a sign-magnitude sum of 127 bits with an overflow counter: adding two values of one sign wraps the magnitude at
                    2^127 and counts +1 / -1, adding values of different signs is exact (SPI/type/UnscaledDecimal128Arithmetic.java
                    :354-379, :416-432); the output fails when the counter is not zero or the magnitude reached 10^38
                    (AGG/DecimalSumAggregation.java:141-190): DECIMAL(38, s).
  avg(DECIMAL(p, s))   the same state and a row counter; the output puts overflow * 2^127 back and divides by the count, ROUND_HALF_UP at
                    the type's scale, i.e. half away from zero on the magnitude (AGG/DecimalAverageAggregation.java:153-227), and writes
                    the input's type, which fails beyond its storage (longValueExact / 10^38).  The overflow term is added as a BigDecimal
                    of scale 0 (:224), right only for scale 0 (stated here as the reference computes it): CASES holds overflowing
                    averages for scale 0 alone.
  min / max         the first value is taken as is, a later one when the type's COMPARISON operator says smaller / larger
                    (AGG/AbstractMinMaxAggregationFunction.java:274-330): Double.compare order for DOUBLE and REAL (-0.0 < +0.0, one NaN
                    above +inf: SPI/type/DoubleType.java:194-198, RealType.java), longs for the integer types and short DECIMAL, the
                    signed 128-bit value for long DECIMAL, false < true (SPI/type/BooleanType.java:145-173), unsigned bytes with a
                    proper prefix first for VARCHAR (SPI/type/VarcharType.java:229-233).
  PARTIAL           the flat intermediate row of include/presto_amd.h: [count] for count / count(*), [count, sum] for sum / avg (sum:
                    BIGINT, DOUBLE, or DECIMAL(38, s)), [count, value] for min / max.

The reference adds in row order; the device adds in lane / wave / workgroup / replica order.  order_free() says for which inputs every
order of addition gives one answer; only those are compared exactly, everything else is an `either` row of DIVERGENCES.
"""
import collections
import fractions
import functools
import math
import struct

import numpy as np

from presto_amd import abi

OUT_OF_RANGE = abi.ERR_NUMERIC_VALUE_OUT_OF_RANGE
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1
TEN38 = 10 ** 38
DBL_MAX = fractions.Fraction(1.7976931348623157e308)
FNS = {"count_star": abi.AGG_COUNT_STAR, "count": abi.AGG_COUNT, "sum": abi.AGG_SUM, "avg": abi.AGG_AVG, "min": abi.AGG_MIN, "max": abi.AGG_MAX}
FN_NAMES = {v: k for k, v in FNS.items()}

# outcome: ("value", v) | ("null",) | ("error", status) | ("either", v, status); row_order: what the reference's row order gives (never
# "either"); type: the result's type; intermediate: the flat PARTIAL row (count,) or (count, value), or ("error", status)
Result = collections.namedtuple("Result", "outcome type row_order intermediate")


def is_decimal(t):
    return t in (abi.DECIMAL, abi.LONG_DECIMAL)


def is_fp(t):
    return t in (abi.DOUBLE, abi.REAL)


def is_int(t):
    return t in (abi.BIGINT, abi.INTEGER, abi.DATE)


def scale_of(t):
    return t.scale if isinstance(t, abi.DecimalType) else 0


def result_type(fn, t):
    if fn in (abi.AGG_COUNT, abi.AGG_COUNT_STAR):
        return abi.BIGINT
    if fn == abi.AGG_SUM:
        return abi.decimal(38, scale_of(t)) if is_decimal(t) else t
    if fn == abi.AGG_AVG:
        return t if (is_decimal(t) or t == abi.REAL) else abi.DOUBLE
    return t


def counted(fn, values, mask=None):
    """the values of the rows an aggregate sees: mask first, then NULL (count(*) keeps NULLs)"""
    rows = [v for i, v in enumerate(values) if mask is None or mask[i] is True]
    return rows if fn == abi.AGG_COUNT_STAR else [v for v in rows if v is not None]


# ---- comparison (min / max) -----------------------------------------------------------------------------------------------------------------
def double_to_long_bits(v):
    """Double.doubleToLongBits as a signed long: every NaN is 0x7ff8000000000000"""
    if v != v:
        return 0x7FF8000000000000
    b = struct.unpack("<q", struct.pack("<d", float(v)))[0]
    return b


def compare(t, a, b):
    if is_fp(t):     # Double.compare: <, >, then the order of doubleToLongBits
        a, b = float(a), float(b)
        if a < b:
            return -1
        if a > b:
            return 1
        x, y = double_to_long_bits(a), double_to_long_bits(b)
        return (x > y) - (x < y)
    if t == abi.VARCHAR:   # bytes compares unsigned, a proper prefix first
        return (a > b) - (a < b)
    return (a > b) - (a < b)


def min_max(fn, t, vs):
    best = vs[0]
    for v in vs[1:]:
        c = compare(t, v, best)
        if (c < 0) if fn == abi.AGG_MIN else (c > 0):
            best = v
    return best


# ---- floating sums ---------------------------------------------------------------------------------------------------------------------------
def widen(t, v):
    """the double an fp aggregate adds: (double) long for the integer types (one rounding to nearest even), the float widened exactly"""
    return float(v)      # Python's int -> float rounds to nearest even once, as the JLS's long -> double; float32 -> float is exact


def double_sum(ds):
    s = 0.0              # the state starts at +0.0
    for d in ds:
        s = s + d
    return s


def to_float(d):
    """Java (float) double: one rounding to nearest even, overflow to the infinities"""
    with np.errstate(over="ignore"):
        return np.float32(d)


def exact_class(ds):
    """all values integer multiples of one power of two q with sum |v| / q < 2^53: every partial sum of every subset is a multiple of q
    below q * 2^53, so it is a double and no addition rounds"""
    fs = [fractions.Fraction(d) for d in ds if d != 0]
    if not fs:
        return True
    q = None
    for f in fs:      # the largest power of two that divides f: 2^(tz(numerator)) / denominator (a double's denominator is a power of two)
        n, tz = abs(f.numerator), 0
        while n % 2 == 0:
            n //= 2
            tz += 1
        e = fractions.Fraction(2 ** tz, f.denominator)
        q = e if q is None or e < q else q
    total = sum(abs(f) for f in fs)
    return total / q < 2 ** 53 and total <= DBL_MAX


def fp_class(ds):
    """'exact' | 'special' (an infinity or NaN decides) | 'overflow' | None (the answer depends on the order of addition)"""
    if any(d != d for d in ds):
        return "special"
    infs = [d for d in ds if math.isinf(d)]
    finite = [fractions.Fraction(d) for d in ds if not math.isinf(d)]
    if infs:
        # finite partial sums stay finite when sum |v| <= the largest double; inf + finite = inf, inf + -inf = NaN in every order
        return "special" if sum(abs(f) for f in finite) <= DBL_MAX else None
    if exact_class(ds):
        return "exact"
    if finite and (all(f > 0 for f in finite) or all(f < 0 for f in finite)):
        # one sign: partial sums only grow in magnitude, and an infinity stays.  Each addition loses at most 2^-53 of its result, so a
        # finite end result would be at least total * (1 - n * 2^-52); when that is still >= 2^1024 every order ends in the infinity
        total = abs(sum(finite))
        if total * (1 - fractions.Fraction(len(finite), 2 ** 52)) >= 2 ** 1024:
            return "overflow"
    return None


# ---- exact sums ------------------------------------------------------------------------------------------------------------------------------
def signed_class(vs, fits):
    """'value' (the positives alone and the negatives alone fit: no order overflows) | 'error' (one sign, the total does not fit: every
    order fails) | 'either'"""
    pos, neg = sum(v for v in vs if v > 0), sum(v for v in vs if v < 0)
    if fits(pos) and fits(neg):
        return "value"
    if (pos == 0 or neg == 0) and not fits(pos + neg):
        return "error"
    return "either"


def fits_i64(v):
    return I64_MIN <= v <= I64_MAX


def fits_dec38(v):
    return abs(v) < TEN38


def long_sum_row_order(vs):
    s = 0
    for v in vs:
        s += v
        if not fits_i64(s):          # Math.addExact
            return ("error", OUT_OF_RANGE)
    return ("value", s)


def decimal_state_row_order(vs):
    """-> (signed 127-bit sum, overflow counter) of UnscaledDecimal128Arithmetic.addWithOverflow in row order"""
    neg, mag, overflow = False, 0, 0          # unscaledDecimal(): +0
    for v in vs:
        vneg, vmag = v < 0, abs(v)
        if neg == vneg:                       # addUnsignedReturnOverflow: the magnitudes add, bit 127 goes to the counter
            mag += vmag
            if mag >> 127:
                mag &= (1 << 127) - 1
                overflow += -1 if neg else 1
        elif mag > vmag:                      # compareAbsolute, subtractUnsigned: exact
            mag -= vmag
        elif mag < vmag:
            neg, mag = vneg, vmag - mag
        else:
            neg, mag = False, 0               # setToZero
    return (-mag if neg else mag), overflow


def round_half_away(n, d):
    """n / d (d > 0) rounded half up on the magnitude: BigDecimal.divide(.., ROUND_HALF_UP)"""
    q, r = divmod(abs(n), d)
    if 2 * r >= d:
        q += 1
    return -q if n < 0 else q


def decimal_storage_fits(t, v):
    return I64_MIN <= v <= I64_MAX if t == abi.DECIMAL else abs(v) < TEN38


# ---- the entry points ------------------------------------------------------------------------------------------------------------------------
def order_free(fn, input_type, values):
    """values: the counted values (no NULLs).  True when every order of addition gives the same outcome."""
    if fn in (abi.AGG_COUNT, abi.AGG_COUNT_STAR, abi.AGG_MIN, abi.AGG_MAX) or not values:
        return True
    if is_decimal(input_type):
        return signed_class(values, fits_dec38) != "either"
    if fn == abi.AGG_SUM and is_int(input_type):
        return signed_class(values, fits_i64) != "either"
    return fp_class([widen(input_type, v) for v in values]) is not None


def aggregate(fn, input_type, values, mask=None, step="single"):
    """One group.  step: 'single' (also what PARTIAL -> FINAL gives in the reference, whose states carry everything) or 'partial'
    (only `intermediate` is of interest)."""
    fn = FNS.get(fn, fn)
    vs = counted(fn, values, mask)
    n = len(vs)
    rtype = result_type(fn, input_type)
    if fn in (abi.AGG_COUNT, abi.AGG_COUNT_STAR):
        return Result(("value", n), rtype, ("value", n), (n,))
    if n == 0:
        return Result(("null",), rtype, ("null",), (0, None) if fn in (abi.AGG_MIN, abi.AGG_MAX) else (0, 0.0 if _double_state(fn, input_type) else 0))
    if fn in (abi.AGG_MIN, abi.AGG_MAX):
        v = min_max(fn, input_type, vs)
        return Result(("value", v), rtype, ("value", v), (n, v))
    if is_decimal(input_type):
        return _decimal(fn, input_type, vs, rtype)
    if fn == abi.AGG_SUM and is_int(input_type):
        row = long_sum_row_order(vs)
        cls = signed_class(vs, fits_i64)
        total = sum(vs)
        inter = (n, total) if row[0] == "value" else row
        if input_type != abi.BIGINT:          # the 32-bit result column of this project's ABI
            assert cls == "value"             # (2^31 rows of one sign would be needed to leave int64)
            row = row if I32_MIN <= total <= I32_MAX else ("error", OUT_OF_RANGE)
            return Result(row, rtype, row, inter)
        if cls == "either":
            return Result(("either", total, OUT_OF_RANGE) if fits_i64(total) else ("error", OUT_OF_RANGE), rtype, row, inter)
        return Result(row, rtype, row, inter)
    # DOUBLE / REAL sums, every avg that is not DECIMAL
    s = double_sum([widen(input_type, v) for v in vs])
    if fn == abi.AGG_SUM:
        v = to_float(s) if input_type == abi.REAL else s
    else:
        a = s / float(n)
        v = to_float(a) if input_type == abi.REAL else a
    return Result(("value", v), rtype, ("value", v), (n, s))


def _double_state(fn, t):
    return not is_decimal(t) and (fn == abi.AGG_AVG or is_fp(t))


def _decimal(fn, t, vs, rtype):
    n = len(vs)
    s, overflow = decimal_state_row_order(vs)
    total = sum(vs)
    cls = signed_class(vs, fits_dec38)
    if fn == abi.AGG_SUM:
        row = ("error", OUT_OF_RANGE) if overflow != 0 or not fits_dec38(s) else ("value", s)
        exact = ("value", total) if fits_dec38(total) else ("error", OUT_OF_RANGE)
    else:
        # (:224 adds the overflow term as a BigDecimal of scale 0 to a sum of the type's scale: 10^scale times too much unless scale = 0)
        avg = round_half_away(s + overflow * 2 ** 127 * 10 ** scale_of(t), n)
        row = ("value", avg) if decimal_storage_fits(t, avg) else ("error", OUT_OF_RANGE)
        exact = row
    # the flat PARTIAL state is a DECIMAL(38, s): it holds the exact total or nothing
    inter = (n, total) if fits_dec38(total) else ("error", OUT_OF_RANGE)
    if cls == "either":
        out = ("either", exact[1], OUT_OF_RANGE) if exact[0] == "value" else exact
        return Result(out, rtype, row, inter)
    assert row == exact or fn == abi.AGG_AVG, (vs, row, exact)
    if fn == abi.AGG_AVG and cls == "error":
        # one sign and the total beyond 10^38: the reference's average still comes out (the overflow is put back); the device's limbs hold
        # it too, its flat PARTIAL state does not
        return Result(("either", exact[1], OUT_OF_RANGE) if exact[0] == "value" else exact, rtype, row, inter)
    return Result(row, rtype, row, inter)


# ---- bit patterns for comparison --------------------------------------------------------------------------------------------------------------
def bits(t, v):
    """a value as what a block stores: floats as bit patterns with every NaN as 'nan'"""
    if v is None:
        return None
    if t == abi.DOUBLE:
        return "nan" if v != v else struct.pack("<d", float(v))
    if t == abi.REAL:
        return "nan" if v != v else struct.pack("<f", float(v))
    if t == abi.BOOLEAN:
        return bool(v)
    return v


def outcome_bits(t, o):
    return (o[0], bits(t, o[1])) + tuple(o[2:]) if o[0] in ("value", "either") else o


# ---- pages -----------------------------------------------------------------------------------------------------------------------------------
def block_of(t, values, nullable=False):
    """a host block of type t (None = NULL); nullable: with a valueIsNull array even when no position is NULL (kernels are generated per
    column-layout signature)"""
    from presto_amd.page import Block
    nulls = np.asarray([v is None for v in values], dtype=np.uint8)
    if t == abi.VARCHAR:
        b = Block.varchar(values)
    elif t == abi.LONG_DECIMAL:
        b = Block.long_decimal(values)
    elif t == abi.BOOLEAN:
        b = Block.boolean([bool(v) for v in values], nulls)
    elif t == abi.DOUBLE:
        b = Block.double(np.asarray([0.0 if v is None else v for v in values], dtype=np.float64), nulls)
    elif t == abi.REAL:
        b = Block.real(np.asarray([0.0 if v is None else v for v in values], dtype=np.float32), nulls)
    else:
        b = Block.flat(int(t), [0 if v is None else v for v in values], nulls)
    if nullable and b.nulls is None:
        b.nulls = np.zeros(b.position_count, dtype=np.uint8)
    return b


# ---- the table -------------------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "name fn type values mask")
NAN = float("nan")
NAN_PAYLOAD = struct.unpack("<d", struct.pack("<Q", 0x7FF0000000000123))[0]     # a signalling NaN pattern with a payload
NAN_NEGATIVE = struct.unpack("<d", struct.pack("<Q", 0xFFF8000000000001))[0]
NAN_NEGATIVE_F32 = np.frombuffer(struct.pack("<I", 0xFFC00001), dtype=np.float32)[0]
INF = float("inf")
F32 = np.float32
D82, D122, D182, D274 = abi.decimal(8, 2), abi.decimal(12, 2), abi.decimal(18, 2), abi.decimal(27, 4)
D380, D3810 = abi.decimal(38, 0), abi.decimal(38, 10)
ALL = ("count_star", "count", "sum", "avg", "min", "max")
TYPE_LABEL = {abi.BIGINT: "BIGINT", abi.INTEGER: "INTEGER", abi.DATE: "DATE", abi.DOUBLE: "DOUBLE", abi.REAL: "REAL", abi.BOOLEAN: "BOOLEAN",
              abi.VARCHAR: "VARCHAR"}


def label(t):
    return ("D%d_%d" % (t.precision, t.scale)) if isinstance(t, abi.DecimalType) else TYPE_LABEL[t]


def _variants(name, fn, t, values):
    """the list as it is, with NULL rows interleaved, and under a mask that removes rows (the removed rows hold values that would change
    every aggregate: the largest and the smallest of the list, and for sums they would not cancel)"""
    out = [Case(name, fn, t, list(values), None)]
    if not values:
        return out
    nulled = [None]
    for v in values:
        nulled += [v, None]
    out.append(Case(name + "/nulls", fn, t, nulled, None))
    decoys = [max(values, key=_key(t)), min(values, key=_key(t))] if t != abi.BOOLEAN else [True, False]
    masked, mask = [], []
    for i, v in enumerate(values):
        masked += [decoys[i % 2], v]
        mask += [False if i % 2 else None, True]          # a NULL mask is false too
    masked.append(None)
    mask.append(True)
    out.append(Case(name + "/mask", fn, t, masked, mask))
    return out


def _key(t):
    return functools.cmp_to_key(lambda a, b: compare(t, a, b))


def _cases():
    out = []

    def add(tag, t, values, fns=ALL):
        for fn in fns:
            out.extend(_variants("%s:%s:%s" % (fn, label(t), tag), FNS[fn], t, values))

    B, I = abi.BIGINT, abi.INTEGER
    add("max", B, [I64_MAX])
    add("min", B, [I64_MIN])
    add("max_min", B, [I64_MAX, I64_MIN])
    exact_only = ("count", "sum", "min", "max")          # (their doubles are no exact-class input: no avg)
    add("fits", B, [2 ** 62, 2 ** 62 - 1, 1], exact_only)
    add("over", B, [2 ** 62, 2 ** 62], exact_only)
    add("under", B, [-2 ** 62, -2 ** 62, -1], exact_only)
    add("back", B, [I64_MAX, 1, -5], ("sum",))
    add("avg_max2", B, [I64_MAX, I64_MAX], ("avg", "count", "min", "max"))
    add("avg_2p53", B, [2 ** 53 + 1], ("avg",))
    add("ends", I, [I32_MAX, I32_MIN], ("count", "avg", "min", "max", "sum"))
    add("over", I, [I32_MAX, 1], ("sum", "avg"))
    add("under", I, [I32_MIN, -1], ("sum", "avg"))
    add("one_max", I, [I32_MAX])
    add("one_min", I, [I32_MIN])
    add("ends", abi.DATE, [I32_MAX, I32_MIN, 0], ("count", "min", "max"))
    add("both", abi.BOOLEAN, [True, False, True], ("count", "min", "max"))
    add("true", abi.BOOLEAN, [True], ("count", "min", "max"))
    add("false", abi.BOOLEAN, [False, False], ("count", "min", "max"))
    doubles = {
        "neg_zeros": [-0.0, -0.0, -0.0], "neg_pos_zero": [-0.0, 0.0], "pos_neg_zero": [0.0, -0.0],
        "nan": [NAN], "nan_among": [1.5, NAN, -2.25], "nan_first": [NAN, 3.0, -INF], "nan_middle": [INF, NAN, -1.0], "nan_last": [-7.0, INF, NAN],
        "both_inf": [INF, 1.0, -INF], "pos_inf": [1.0, INF, -3.5, INF], "neg_inf": [-INF, 2.0],
        "max_twice": [1.7976931348623157e308] * 2, "denormals": [5e-324] * 3,
        # [2^53, 1.0, -2^53] itself is no exact-class input (sum |v| = 2^54 + 1: the 1.0 is absorbed or not, by the order); the same shape
        # at the largest magnitude that is: q = 1, sum |v| = 2^53 - 1
        "cancel": [2.0 ** 52, 1.0, -(2.0 ** 52 - 2)],
        "two_nans": [NAN_PAYLOAD, NAN_NEGATIVE],
        "negative_nan_among": [1.5, NAN_NEGATIVE, -2.25],                              # a NaN with the sign bit set is the one NaN too
    }
    for tag, vs in doubles.items():
        add(tag, abi.DOUBLE, vs)
    reals = {
        "neg_zeros": [-0.0, -0.0], "neg_pos_zero": [-0.0, 0.0], "pos_neg_zero": [0.0, -0.0],
        "nan": [NAN], "nan_among": [1.5, NAN, -2.25], "nan_first": [NAN, 3.0, -INF], "nan_middle": [INF, NAN, -1.0], "nan_last": [-7.0, INF, NAN],
        "both_inf": [INF, 1.0, -INF], "pos_inf": [1.0, INF, -3.5],
        "max_twice": [3.4028235e38] * 2,           # the DOUBLE sum is finite, (float) of it +inf, the average finite
        "not_a_float": [16777217.0, 16777217.0],   # 2^24 + 1 rounds to 2^24 when the block is written
        "denormal": [1e-45] * 3,
        "cancel": [2.0 ** 23, 1.0, -(2.0 ** 23 - 2)],
        "negative_nan_among": [1.5, NAN_NEGATIVE_F32, -2.25],
    }
    for tag, vs in reals.items():
        add(tag, abi.REAL, [F32(v) for v in vs])
    for t in (D82, D122, D182, D274):
        top = 10 ** t.precision - 1
        add("top", t, [top])
        add("bottom", t, [-top])
        add("top_twice", t, [top, top])
        add("bottom_twice", t, [-top, -top, -top])
        add("cancel", t, [top, -top, 7, -7])
        limbs = [v for v in (-1, -2 ** 30, 2 ** 30 - 1, 2 ** 30, 2 ** 60, -2 ** 60, 2 ** 60 - 1) if abs(v) <= top]
        add("limb_edges", t, limbs)
        for v in limbs:
            add("limb_%s" % str(v).replace("-", "m"), t, [v], ("sum", "avg", "min"))
        add("half_up", t, [1, 2], ("avg",))
        add("half_down", t, [-1, -2], ("avg",))
        add("third_up", t, [1, 1, 2], ("avg",))
        add("third_down", t, [-1, -1, -2], ("avg",))
    for t in (D380, D3810):
        top = TEN38 - 1
        add("top", t, [top])
        add("bottom", t, [-top])
        add("words", t, [2 ** 64 - 1, 2 ** 64, 2 ** 64 + 1, -2 ** 64])
        for v in (2 ** 64 - 1, 2 ** 64, 2 ** 64 + 1, -2 ** 64):
            add("word_%s" % str(v).replace("-", "m"), t, [v], ("sum", "avg", "max"))
        add("over", t, [top, 1], ("sum",))
        add("under", t, [-top, -1], ("sum",))
        # -> 5 in the reference's row order and on the device; by order_free's rule an `either` row all the same (the positives alone
        # reach 10^38): test_gpu_agg_edges asserts exactly 5 in a SINGLE step, 5 or OUT_OF_RANGE where a PARTIAL state is cut
        add("cancel", t, [top, -top, 5], ("sum", "avg"))
        add("cancel_fits", t, [top - 5, -top, 5])
        add("back", t, [top, top, -top], ("sum",))
        add("half_up", t, [1, 2], ("avg",))
        add("half_down", t, [-1, -2], ("avg",))
    add("avg_top_twice", D380, [TEN38 - 1, TEN38 - 1], ("avg",))
    strings = [b"", b"\x00", b"a", b"ab", b"\xff\xfe", b"abcdefgh", b"abcdefgh\x00", b"abcdefghi", b"abcdefg", b"0123456789" * 4]
    add("all", abi.VARCHAR, strings, ("count", "min", "max"))
    add("short", abi.VARCHAR, [b"a", b"", b"\x00", b"ab", b"\xff\xfe", b"abcdefg"], ("count", "min", "max"))
    add("prefix8", abi.VARCHAR, [b"abcdefgh\x00", b"abcdefgh", b"abcdefghi"], ("count", "min", "max"))
    add("empty_only", abi.VARCHAR, [b""], ("count", "min", "max"))
    for t, one in ((B, 5), (I, -5), (abi.DOUBLE, -0.0), (abi.REAL, F32(2.5)), (D122, -1), (D380, 1), (abi.VARCHAR, b"x")):
        fns = ("count_star", "count", "min", "max") if t == abi.VARCHAR else ALL
        for fn in fns:
            out.append(Case("%s:%s:one_row" % (fn, label(t)), FNS[fn], t, [one], None))
            out.append(Case("%s:%s:only_nulls" % (fn, label(t)), FNS[fn], t, [None, None, None], None))
            out.append(Case("%s:%s:all_masked" % (fn, label(t)), FNS[fn], t, [one, one], [False, None]))
            out.append(Case("%s:%s:no_rows" % (fn, label(t)), FNS[fn], t, [], None))
    return out


CASES = _cases()
CASE = {c.name: c for c in CASES}
assert len(CASE) == len(CASES)

# What the device (and, for the first, this project's ABI as a whole) deliberately computes differently from the reference: the tag of the
# entry in DESIGN.md section 5 -> the names of the CASES rows it covers.  An `either` outcome may appear on these rows alone.
DIVERGENCES = {
    # (1) of DESIGN section 5: partial sums instead of the running sum
    "agg-bigint-sum-order": [n for n in CASE if n.startswith("sum:BIGINT:back")],
    # the DECIMAL twin: exact limb sums, failing only on the total; the flat PARTIAL state is a DECIMAL(38, s)
    "agg-decimal-sum-order": [n for n in CASE if n.startswith(("sum:D38_0:back", "sum:D38_10:back", "avg:D38_0:avg_top_twice", "sum:D38_0:cancel", "avg:D38_0:cancel",
                                                                "sum:D38_10:cancel", "avg:D38_10:cancel")) and ":cancel_fits" not in n],
    # sum(INTEGER) keeps an INTEGER column and fails beyond it
    "agg-integer-sum-column": [n for n in CASE if n.startswith(("sum:INTEGER:over", "sum:INTEGER:under"))],
}


def case_result(c, step="single"):
    return aggregate(c.fn, c.type, c.values, c.mask, step)


def compared(c):
    """rows whose outcome is one value, NULL or one status in every order of addition"""
    return case_result(c).outcome[0] != "either"
