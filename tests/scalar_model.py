"""LIKE, substr, length and year / month / day restated in plain Python, independently of the device's algorithms (not a test file).

The reference is the specification:
  core/trino-main/src/main/java/io/trino/type/LikeFunctions.java           likeVarchar :74-89, likePattern :198-241, escape :181-195 / :244-255
  core/trino-main/src/main/java/io/trino/operator/scalar/StringFunctions.java   length :98-101, substring :278-310 / :325-368
  core/trino-main/src/main/java/io/trino/operator/scalar/DateTimeFunctions.java dayFromDate :428, monthFromDate :477, yearFromDate :501

Values are Python str (code points), or None for NULL; a NULL argument gives NULL.  LIKE goes through `re` (DOTALL, fullmatch) -- the
device splits the pattern at `%` or walks it with one backtrack point; substr and length work on str code points -- the device steps
through UTF-8 lead bytes; the date fields come from datetime.date -- the device uses a closed-form civil-from-days.
"""
import datetime
import re

INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
BAD_ESCAPE = "Escape character must be followed by '%', '_' or the escape character itself"
BAD_ESCAPE_STRING = "Escape string must be a single character"


class InvalidArgument(Exception):
    """INVALID_FUNCTION_ARGUMENT when the pattern is compiled"""


class ReferenceFails(Exception):
    """the reference itself fails on this input with an internal error (no SQL result)"""


def like_regex(pattern, escape=None):
    """likePattern :198-241 (escape :244-255): the pattern as a Python regular expression.  The reference iterates UTF-16 chars and the
    escape is one char; patterns here hold an escape of the BMP only, where chars and code points coincide."""
    escaping = False
    if escape is not None:
        if escape != "":                       # an empty escape string disables escaping
            if len(escape.encode("utf-16-le")) != 2:
                raise InvalidArgument(BAD_ESCAPE_STRING)
            escaping = True
    out = []
    escaped = False
    for c in pattern:
        if escaped and c not in ("%", "_") and not (escaping and c == escape):
            raise InvalidArgument(BAD_ESCAPE)
        if escaping and not escaped and c == escape:
            escaped = True
            continue
        if c == "%" and not escaped:
            out.append(".*")
        elif c == "_" and not escaped:
            out.append(".")
        else:
            out.append(re.escape(c))
        escaped = False
    if escaped:
        raise InvalidArgument(BAD_ESCAPE)
    return re.compile("".join(out), re.DOTALL)


def like(value, pattern, escape=None, has_escape=False):
    """value LIKE pattern [ESCAPE escape].  has_escape: the three-argument form (escape None is then the NULL constant)."""
    if pattern is None or (has_escape and escape is None):
        return None
    regex = like_regex(pattern, escape if has_escape else None)    # a bad pattern is an error whatever the value
    return None if value is None else regex.fullmatch(value) is not None


def length(value):
    return None if value is None else len(value)


def _saturate(v):
    return max(INT32_MIN, min(INT32_MAX, v))


def _wrap32(v):
    return ((v + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def substr(value, start, length=None, has_length=False):
    """substring :278-310 (two arguments) and :325-368 (three): code points, 1-based.  Raises ReferenceFails where the reference's own
    code fails: the int addition of :360 wraps for a negative start and a length near 2^31, offsetOfCodePoint then answers -1 and
    Slice.slice is asked for a negative length."""
    if value is None or start is None or (has_length and length is None):
        return None
    if start == 0 or value == "" or (has_length and length <= 0):
        return ""
    start_cp = _saturate(start)
    length_cp = _saturate(length) if has_length else None
    if start_cp > 0:
        if start_cp - 1 >= len(value):          # offsetOfCodePoint < 0
            return ""
        return value[start_cp - 1:] if not has_length else value[start_cp - 1:start_cp - 1 + length_cp]
    cps = len(value)
    start_cp += cps
    if start_cp < 0:
        return ""
    if not has_length:
        return value[start_cp:]
    if _wrap32(start_cp + length_cp) < cps:      # :360, a Java int addition
        if start_cp + length_cp >= cps:          # wrapped: offsetOfCodePoint(utf8, indexStart, lengthCodePoints) = -1, slice(indexStart, -1 - indexStart)
            raise ReferenceFails("substring: negative slice length")
        return value[start_cp:start_cp + length_cp]
    return value[start_cp:]


_CYCLE_DAYS = 146097                              # days of 400 Gregorian years
_EPOCH_ORDINAL = datetime.date(1970, 1, 1).toordinal()
_MIN_ORDINAL, _MAX_ORDINAL = datetime.date.min.toordinal(), datetime.date.max.toordinal()


def civil(days):
    """(year, month, day) of the DATE `days` since 1970-01-01: proleptic Gregorian, astronomical year numbering (ISOChronology in UTC).
    datetime.date inside years 1..9999; outside, whole 400-year cycles are shifted in first (the calendar repeats every 146097 days)."""
    if days is None:
        return None
    ordinal = days + _EPOCH_ORDINAL
    cycles = 0
    if ordinal < _MIN_ORDINAL:
        cycles = -((_MIN_ORDINAL - ordinal + _CYCLE_DAYS - 1) // _CYCLE_DAYS)
    elif ordinal > _MAX_ORDINAL:
        cycles = (ordinal - _MAX_ORDINAL + _CYCLE_DAYS - 1) // _CYCLE_DAYS
    d = datetime.date.fromordinal(ordinal - cycles * _CYCLE_DAYS)
    return d.year + 400 * cycles, d.month, d.day


def year(days): return None if days is None else civil(days)[0]
def month(days): return None if days is None else civil(days)[1]
def day(days): return None if days is None else civil(days)[2]
