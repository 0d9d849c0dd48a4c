"""csrc/decimal_host.hpp -- the host half of sum / avg over DECIMAL -- against Python's exact integers, through a stand-alone program
(tests/cpp/test_decimal_host.cpp, built here with g++ -Wall -Werror).  The kernels hand over a group's sum as i64 sums of 30-bit limbs
(pa_dec_limb in csrc/kernels/pa_device.h, restated below); the GPU tests cannot reach the documented limit of 2^33 rows per group, so
limb words of the size they have after 2^33 rows of +-(10^p - 1) are checked here."""
import ctypes as C
import os
import subprocess
import tempfile

import pytest

from presto_amd import abi
from presto_amd.expr import field
from presto_amd.operators import fused_aggregation_desc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMB_BITS = 30
TEN38 = 10 ** 38
MASK64 = (1 << 64) - 1


def limbs_of(v, limbs):
    """pa_dec_limb: limb k is bits 30k .. 30k+29 of the two's complement value, the last limb everything above, signed"""
    out = []
    for k in range(limbs):
        s = v >> (LIMB_BITS * k)              # arithmetic shift
        out.append(s if k == limbs - 1 else s & ((1 << LIMB_BITS) - 1))
    return out


def limb_sums(values, limbs):
    sums = [0] * limbs
    for v, times in values:
        for k, w in enumerate(limbs_of(v, limbs)):
            sums[k] += w * times
    assert all(-2 ** 63 <= s < 2 ** 63 for s in sums), sums      # what an i64 accumulator word holds
    return sums


def round_half_away(n, d):
    q, r = divmod(abs(n), d)
    if 2 * r >= d:
        q += 1
    return -q if n < 0 else q


def words192(v):
    v &= (1 << 192) - 1
    return "%016x %016x %016x" % (v & MASK64, (v >> 64) & MASK64, v >> 128)


def fit(v, bound):
    if abs(v) >= bound:
        return "-"
    return "%s:%016x:%016x" % ("n" if v < 0 else "p", abs(v) >> 64, abs(v) & MASK64)


def stored(v):
    """LongDecimalType's 16 bytes: the low word of the magnitude, then the high word with the sign on top (no negative zero)"""
    if abs(v) >= TEN38:
        return "-"
    lo, hi = abs(v) & MASK64, (abs(v) >> 64) | ((1 << 63) if v < 0 else 0)
    return (lo.to_bytes(8, "little") + hi.to_bytes(8, "little")).hex()


def expected_line(sums, count):
    total = sum(s << (LIMB_BITS * k) for k, s in enumerate(sums))
    avg = round_half_away(total, count)
    return "total %s avg %s t63 %s t38 %s a63 %s a38 %s tbytes %s abytes %s" % (
        words192(total), words192(avg), fit(total, 2 ** 63), fit(total, TEN38), fit(avg, 2 ** 63), fit(avg, TEN38), stored(total), stored(avg))


@pytest.fixture(scope="module")
def program():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "test_decimal_host")
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "presto_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "test_decimal_host.cpp"), "-o", exe], check=True)

        def run(lines):
            out = subprocess.run([exe], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True).stdout.splitlines()
            assert len(out) == len(lines)
            return out
        yield run


def bits_needed(p):
    """bits of a two's complement integer that holds +-(10^p - 1)"""
    return (10 ** p - 1).bit_length() + 1


def test_limbs_hold_every_precision(program):
    out = program(["p %d" % p for p in range(1, 39)])
    for p, line in zip(range(1, 39), out):
        _, bits, _, limbs = line.split()
        bits, limbs = int(bits), int(limbs)
        assert bits >= bits_needed(p), (p, bits)
        assert limbs * LIMB_BITS >= bits_needed(p) or (p > 18 and limbs == 5), (p, limbs)     # 5 limbs: the top one takes what is left of 128 bits
        top = 10 ** p - 1
        # as the generator cuts them: short decimals into at most 64 bits, long ones into at most 128
        n = -(-min(64 if p <= 18 else 128, bits) // LIMB_BITS)
        for v in (top, -top, 0, -1):
            cut = limbs_of(v, n)
            assert sum(w << (LIMB_BITS * k) for k, w in enumerate(cut)) == v
            assert all(0 <= w < 2 ** LIMB_BITS for w in cut[:-1]) and -2 ** 63 <= cut[-1] < 2 ** 63
    assert [int(line.split()[3]) for line in (out[7], out[11], out[17], out[26], out[37])] == [1, 2, 3, 4, 5]   # p = 8, 12, 18, 27, 38


def cases():
    out = []
    rows33 = 2 ** 33
    for p, limbs in ((8, 1), (12, 2), (18, 3), (27, 4), (38, 5)):
        top = 10 ** p - 1
        for count in (1, 2, 3, rows33):
            for v in (top, -top):
                if abs(v * count) < 2 ** 160:
                    out.append((limb_sums([(v, count)], limbs), count))
        # exact halves of both signs, and just beside them
        out.append((limb_sums([(1, 1), (2, 1)], limbs), 2))
        out.append((limb_sums([(-1, 1), (-2, 1)], limbs), 2))
        out.append((limb_sums([(1, 2), (2, 1)], limbs), 3))
        out.append((limb_sums([(-1, 2), (-2, 1)], limbs), 3))
        out.append((limb_sums([(top, rows33 // 2), (top - 1, rows33 // 2)], limbs), rows33))        # remainder exactly half
        out.append((limb_sums([(-top, rows33 // 2), (-(top - 1), rows33 // 2)], limbs), rows33))
        out.append((limb_sums([(top, rows33 // 2 - 1), (top - 1, rows33 // 2 + 1)], limbs), rows33))  # just below half
        out.append((limb_sums([(top, 1), (-top, 1)], limbs), 2))
        out.append((limb_sums([(-1, rows33)], limbs), rows33))      # low limbs full, a negative top limb
        out.append((limb_sums([(-2 ** 30, 3), (2 ** 30 - 1, 3)], limbs), 6) if p > 9 else (limb_sums([(-1, 7)], limbs), 7))
    # limb words near +-2^63 (whatever rows would leave them there)
    for limbs in (1, 2, 3, 4, 5):
        for word in (2 ** 63 - 1, -2 ** 63, 2 ** 63 - 2, -2 ** 63 + 1):
            out.append(([word] * limbs, 2 ** 33))
            out.append(([0] * (limbs - 1) + [word], 1))
            out.append(([word] + [0] * (limbs - 1), 3))
    # totals of both signs at 10^38 - 1, 10^38 and -10^38, over the counts 1, 2, 3 and 2^33
    for total in (TEN38 - 1, TEN38, -TEN38, -(TEN38 - 1), TEN38 + 1, 2 ** 127, -2 ** 127, 2 ** 63, 2 ** 63 - 1, -2 ** 63, -2 ** 63 - 1):
        for count in (1, 2, 3, rows33):
            out.append((limbs_of(total, 5), count))
    return out


def test_totals_averages_bounds_and_bytes(program):
    cs = cases()
    got = program(["v %d %d %s" % (len(sums), count, " ".join(str(s) for s in sums)) for sums, count in cs])
    wrong = [(sums, count, g, expected_line(sums, count)) for (sums, count), g in zip(cs, got) if g != expected_line(sums, count)]
    assert not wrong, (len(wrong), wrong[:3])
    assert len(cs) > 150


@pytest.mark.parametrize("precision,limbs", [(8, 1), (12, 2), (18, 3), (27, 4), (38, 5)])
def test_generated_sum_cuts_as_many_limbs(precision, limbs):
    """the generator cuts a DECIMAL(p, s) sum into the limbs its precision needs (2^33 rows of +-(10^p - 1) must fit the i64 words): the
    generated source of every tier names limb 0 .. limbs - 1 and says which is the last"""
    from presto_amd._lib import lib
    t = abi.decimal(precision, 2)
    desc, keep = fused_aggregation_desc([abi.BIGINT, t], None, [field(0, abi.BIGINT), field(1, t)], [0], [(abi.AGG_SUM, 1, t), (abi.AGG_AVG, 1, t)])
    for variant in (1, 2, 3):      # few groups, HBM table, LDS table
        need = lib().pa_codegen_fused(C.byref(desc), variant, None, 0, None)
        assert need > 0, lib().pa_last_error().decode()
        buf = C.create_string_buffer(need)
        lib().pa_codegen_fused(C.byref(desc), variant, buf, need, None)
        src = buf.value.decode()
        for k in range(limbs):
            assert ", %d, %d)" % (k, limbs - 1) in src and "pa_dec_limb(" in src, (precision, variant, k)
        assert ", %d, %d)" % (limbs, limbs) not in src and ", %d, %d)" % (limbs - 1, limbs) not in src
