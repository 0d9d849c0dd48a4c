// pa_scalar.h -- device helpers of the scalar functions the expression generator knows beyond arithmetic (pa_call_op PA_OP_LIKE ..
// PA_OP_DAY, csrc/exprgen.cpp).  Embedded behind pa_device.h into the translation units whose row function calls one of them, and only
// into those (jit.cpp): every other generated kernel keeps its source, its key and its name.
#pragma once

// ---------------------------------------------------------------------------------------------
// LIKE / substr / length (LikeFunctions.java:74-89, :198-241; StringFunctions.java:98-101, :278-368).  Bytes are read one at
// a time, or eight at a time while eight are left (pa_str_eq, pa_str_find): no read leaves [a, a + alen).  UTF-8 is never validated:
// a code point is as long as its lead byte says (a continuation byte in lead position counts as one byte), clipped to the end.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ bool pa_str_prefix(const u8* a, i32 alen, const u8* lit, i32 n)
{
    return alen >= n && pa_str_eq(a, n, lit, n);
}
__device__ __forceinline__ bool pa_str_suffix(const u8* a, i32 alen, const u8* lit, i32 n)
{
    return alen >= n && pa_str_eq(a + (alen - n), n, lit, n);
}
// leftmost occurrence of lit[0, n), n >= 1, inside a[from, to): its index, or -1
__device__ inline i32 pa_str_find(const u8* a, i32 from, i32 to, const u8* lit, i32 n)
{
    const u8 first = lit[0];
    i32 i = from;
    // eight bytes at a time, all of them inside [from, to): the bytes equal to the literal's first one are the zero bytes of w ^ ones * first
    // (the lowest flagged byte is exact, a higher one may be a borrow's: every candidate is compared in full)
    const u64 ones = 0x0101010101010101ULL, highs = 0x8080808080808080ULL;
    for (; i + 8 <= to; i += 8) {
        const u64 x = pa_rd64(a + i) ^ (ones * first);
        for (u64 m = (x - ones) & ~x & highs; m; m &= m - 1) {
            const i32 at = i + (__builtin_ctzll(m) >> 3);
            if (at + n > to) break;
            i32 j = 0;
            while (j < n && a[at + j] == lit[j]) j++;
            if (j == n) return at;
        }
    }
    for (; i + n <= to; i++) {
        if (a[i] != first) continue;
        i32 j = 1;
        while (j < n && a[i + j] == lit[j]) j++;
        if (j == n) return i;
    }
    return -1;
}
__device__ __forceinline__ i32 pa_cp_len(u8 lead)
{
    return lead < 0xC0 ? 1 : (lead < 0xE0 ? 2 : (lead < 0xF0 ? 3 : 4));
}
// the byte index after the code point that starts at a[i], i < alen
__device__ __forceinline__ i32 pa_cp_next(const u8* a, i32 alen, i32 i)
{
    const i32 e = i + pa_cp_len(a[i]);
    return e < alen ? e : alen;
}
// SliceUtf8.countCodePoints: the bytes that are not 10xxxxxx
__device__ inline i32 pa_cp_count(const u8* a, i32 alen)
{
    i32 n = 0;
    for (i32 i = 0; i < alen; i++) n += (a[i] & 0xC0) != 0x80;
    return n;
}
// the byte index of code point `k` (0-based) counted from byte `from`; alen when the string ends first
__device__ inline i32 pa_cp_offset(const u8* a, i32 alen, i32 from, i32 k)
{
    i32 i = from;
    while (k > 0 && i < alen) {
        i = pa_cp_next(a, alen, i);
        k--;
    }
    return i;
}
// LIKE with `_`: pat is the unescaped pattern, 0xFF for `%` (runs collapsed) and 0xFE for `_`, every other byte itself (the generator
// refuses literals that hold 0xFE / 0xFF).  One pass with a single backtrack point, the last `%`: leftmost-first is exact for `%`.
#define PA_LIKE_ANY 0xFF
#define PA_LIKE_ONE 0xFE
__device__ inline bool pa_like_general(const u8* a, i32 alen, const u8* pat, i32 plen)
{
    i32 v = 0, p = 0, star_p = -1, star_v = 0;
    while (v < alen) {
        const u8 t = p < plen ? pat[p] : (u8)PA_LIKE_ANY;
        if (p < plen && t == PA_LIKE_ANY) {
            star_p = ++p;
            star_v = v;
        }
        else if (p < plen && t == PA_LIKE_ONE) {
            v = pa_cp_next(a, alen, v);
            p++;
        }
        else if (p < plen && t == a[v]) {
            v++;
            p++;
        }
        else {
            if (star_p < 0) return false;
            star_v = pa_cp_next(a, alen, star_v);   // the `%` takes one more code point
            v = star_v;
            p = star_p;
        }
    }
    while (p < plen && pat[p] == PA_LIKE_ANY) p++;
    return p == plen;
}
// substr(value, start[, length]): the byte range [*from, *from + result) of the value (StringFunctions.java:278-310, :325-368).
// start / length arrive saturated to int32 (Ints.saturatedCast); `has_length` false is the two-argument form.
__device__ inline i32 pa_substr(const u8* a, i32 alen, i64 start64, bool has_length, i64 length64, i32* from)
{
    *from = 0;
    if (start64 == 0 || alen == 0 || (has_length && length64 <= 0)) return 0;
    const i32 start = start64 > 2147483647LL ? 2147483647 : (start64 < -2147483648LL ? (i32)(-2147483647 - 1) : (i32)start64);
    const i32 length = length64 > 2147483647LL ? 2147483647 : (i32)length64;
    if (start > 0) {
        const i32 s = pa_cp_offset(a, alen, 0, start - 1);
        if (s >= alen) return 0;                                   // offsetOfCodePoint < 0: past the end
        const i32 e = has_length ? pa_cp_offset(a, alen, s, length) : alen;
        *from = s;
        return e - s;
    }
    const i32 cps = pa_cp_count(a, alen);
    const i32 sc = (i32)((u32)start + (u32)cps);                   // start < 0, cps >= 0: no overflow
    if (sc < 0) return 0;
    const i32 s = pa_cp_offset(a, alen, 0, sc);
    i32 e = alen;
    if (has_length) {
        // :360 `startCodePoint + lengthCodePoints < codePoints` is a Java int addition: it wraps.  Wrapped, the reference asks
        // offsetOfCodePoint for more code points than there are, gets -1 and fails in Slice.slice (negative length): the empty string
        // here (scalar-substr-wrapped-length)
        const i32 sum = (i32)((u32)sc + (u32)length);
        if (sum < cps) {
            if ((i64)sc + (i64)length != (i64)sum) return 0;
            e = pa_cp_offset(a, alen, s, length);
        }
    }
    *from = s;
    return e - s;
}
// DateTimeFunctions.java:428 / :477 / :501 (ISOChronology in UTC): proleptic Gregorian, year 0 exists; 64-bit throughout.
// field 0 = year, 1 = month, 2 = day
__device__ inline i64 pa_civil_from_days(i64 days, int field)
{
    const i64 z = days + 719468;
    const i64 era = (z >= 0 ? z : z - 146096) / 146097;
    const i64 doe = z - era * 146097;                                        // [0, 146096]
    const i64 yoe = (doe - doe / 1460 + doe / 36524 - doe / 146096) / 365;   // [0, 399]
    const i64 doy = doe - (365 * yoe + yoe / 4 - yoe / 100);                 // [0, 365], March 1st = 0
    const i64 mp = (5 * doy + 2) / 153;
    const i64 m = mp < 10 ? mp + 3 : mp - 9;
    if (field == 2) return doy - (153 * mp + 2) / 5 + 1;
    if (field == 1) return m;
    return yoe + era * 400 + (m <= 2 ? 1 : 0);
}
