"""tests/scalar_model.py pinned by the reference's own known answers (paths under core/trino-main/src/test/java/io/trino):
sql/TestLikeFunctions.java, operator/scalar/TestStringFunctions.java, operator/scalar/TestDateTimeFunctions.java.  The char(x)
variants and the invalid-UTF-8 value (TestLikeFunctions.java:116-123) are not on the device path and are left out."""
import datetime

import pytest

from tests import scalar_model as S

# (value, pattern, escape or None, expected) -- TestLikeFunctions.java, line of the assertion
LIKE_CASES = [
    ("foobar", "f%b__", None, True),                  # :54
    ("foob", "f%b__", None, False),                   # :57
    ("foob", "f%b", None, True),                      # :58
    ("ala  ", "ala  ", None, True),                   # :80
    ("ala", "ala  ", None, False),                    # :81
    ("foo\nbar", "%o\nbar", None, True),              # :92
    ("foo\nbar", "%b%", None, True),                  # :99
    ("foo\nbar", "f%b%", None, True),                 # :106
    ("foo", "%名誉%", "\\", False),           # :112-113
    ("\\abc\\/\\\\", "\\abc\\/\\\\", None, True),     # :128-129 backslashes have no special meaning
    ("\\abc%", "\\\\abc\\%", "\\", True),             # :135-136
    ("x%_abcx", "xxx%x_abcxx", "x", True),            # :142-143
]


@pytest.mark.parametrize("value,pattern,escape,expected", LIKE_CASES)
def test_like_known_answers(value, pattern, escape, expected):
    assert S.like(value, pattern, escape, has_escape=escape is not None) is expected


@pytest.mark.parametrize("pattern", ["#", "abc#abc", "abc#"])     # TestLikeFunctions.java:149-157
def test_invalid_escape_is_an_error(pattern):
    with pytest.raises(S.InvalidArgument, match="Escape character must be followed by"):
        S.like("abc", pattern, "#", has_escape=True)
    with pytest.raises(S.InvalidArgument):
        S.like(None, pattern, "#", has_escape=True)       # the pattern is compiled whatever the value


def test_escape_string_rules():
    """LikeFunctions.java:244-255: empty = escaping disabled, one char, else an error; :187 a non-BMP escape is not one char"""
    assert S.like("a#b", "a#b", "", has_escape=True) is True
    assert S.like("a%b", "a#%b", "#", has_escape=True) is True and S.like("axb", "a#%b", "#", has_escape=True) is False
    for bad in ("##", "ab", "\U0001F600"):
        with pytest.raises(S.InvalidArgument, match="single character"):
            S.like("a", "a", bad, has_escape=True)
    assert S.like("a", None) is None and S.like(None, "a") is None and S.like("a", "a", None, has_escape=True) is None


def test_regex_characters_match_themselves():
    for c in "\\^$.*+?()[]{}|":
        assert S.like("a" + c + "b", "a" + c + "b") is True and S.like("axb", "a" + c + "b") is False


def test_underscore_is_one_code_point_line_feed_included():
    for c in ("a", "é", "名", "\U0001F600", "\n"):
        assert S.like(c, "_") is True and S.like(c + c, "_") is False and S.like(c + c, "__") is True


HOPE = "信念,爱,希望"
DESERET = "\U0001042Dend"
# (value, start, length or None, expected) -- TestStringFunctions.java
SUBSTR_CASES = [
    ("Quadratically", 5, None, "ratically"), ("Quadratically", 50, None, ""), ("Quadratically", -5, None, "cally"),       # :355-357
    ("Quadratically", -50, None, ""), ("Quadratically", 0, None, ""),                                                     # :358-359
    ("Quadratically", 5, 6, "ratica"), ("Quadratically", 5, 10, "ratically"), ("Quadratically", 5, 50, "ratically"),      # :361-363
    ("Quadratically", 50, 10, ""), ("Quadratically", -5, 4, "call"), ("Quadratically", -5, 40, "cally"),                  # :364-366
    ("Quadratically", -50, 4, ""), ("Quadratically", 0, 4, ""), ("Quadratically", 5, 0, ""),                              # :367-369
    (HOPE, 1, 1, "信"), (HOPE, 3, 5, ",爱,希望"), (HOPE, 4, None, "爱,希望"),                 # :381-383
    (HOPE, -2, None, "希望"), (DESERET, 1, 1, "\U0001042D"), (DESERET, 2, 3, "end"),                              # :384-386
]
LENGTH_CASES = [("", 0), ("hello", 5), ("Quadratically", 13), ("hello naïve world", 17), (DESERET, 4), (HOPE, 7)]   # :134-141


@pytest.mark.parametrize("value,start,length,expected", SUBSTR_CASES)
def test_substr_known_answers(value, start, length, expected):
    assert S.substr(value, start, length, has_length=length is not None) == expected


@pytest.mark.parametrize("value,expected", LENGTH_CASES)
def test_length_known_answers(value, expected):
    assert S.length(value) == expected


def test_substr_saturation_and_the_wrapping_addition():
    """StringFunctions.java:284 / :331-332 saturate; :360 is an int addition.  -2 + 3 code points = 1, + INT32_MAX wraps below the count:
    the reference then slices with a negative length and fails; one less than the wrap is the plain clipped case."""
    assert S.substr("abc", S.INT64_MAX) == "" and S.substr("abc", S.INT64_MIN) == ""
    assert S.substr("abc", 1, S.INT64_MAX, has_length=True) == "abc" and S.substr("abc", 2, S.INT64_MIN, has_length=True) == ""
    assert S.substr("abc", -3, S.INT64_MAX, has_length=True) == "abc"          # 0 + INT32_MAX does not wrap
    with pytest.raises(S.ReferenceFails):
        S.substr("abc", -2, S.INT64_MAX, has_length=True)
    assert S.substr("abc", -2, S.INT32_MAX - 1, has_length=True) == "bc"
    assert S.substr(None, 1) is None and S.substr("a", None) is None and S.substr("a", 1, None, has_length=True) is None


def days(y, m, d):
    return datetime.date(y, m, d).toordinal() - datetime.date(1970, 1, 1).toordinal()


def test_date_fields_known_answers():
    d = days(2001, 8, 22)        # TestDateTimeFunctions.java:99 DATE_LITERAL; :512 day, :519 month, :521 year
    assert (S.year(d), S.month(d), S.day(d)) == (2001, 8, 22)
    assert S.year(None) is None and S.month(None) is None and S.day(None) is None


def test_date_fields_outside_datetime_range():
    """year 0 exists (a leap year), negative days work, the INTEGER range of DATE is exact"""
    assert S.civil(0) == (1970, 1, 1) and S.civil(-1) == (1969, 12, 31)
    assert S.civil(59) == (1970, 3, 1) and S.civil(11016) == (2000, 2, 29) and S.civil(11017) == (2000, 3, 1)
    assert S.civil(-719162) == (1, 1, 1) and S.civil(-719163) == (0, 12, 31)
    assert S.civil(-719528) == (0, 1, 1) and S.civil(-719529) == (-1, 12, 31)
    assert S.civil(-719528 + 59) == (0, 2, 29)
    assert S.civil(S.INT32_MAX) == (5881580, 7, 11) and S.civil(S.INT32_MIN) == (-5877641, 6, 23)     # java.time.LocalDate.ofEpochDay
    assert S.civil(days(9999, 12, 31) + 1) == (10000, 1, 1)
