"""Exact decimal -> fp32 oracle and hard-case corpora for the number parsers (host: core/json.cpp,
device: kernels/decode.hip).  Pure Python on fractions.Fraction: no float arithmetic decides a bit.

f32_bits(token)          correctly rounded (nearest, ties-to-even) fp32 bit pattern, None = infinity
midpoint_distance(token) relative distance of the exact value from the nearest fp32 rounding boundary
must_accept(token)       the device contract (decode.hip's header comment), not the kernel's code
near_midpoints / exact_ties / boundaries / forms / ordinary: seeded corpus generators (lists of tokens)
"""
import random
import re
from fractions import Fraction
from functools import lru_cache

import numpy as np

_NUM = re.compile(r"(-?)(0|[1-9][0-9]*)(?:\.([0-9]+))?(?:[eE]([+-]?[0-9]+))?\Z")

FLT_MAX = Fraction((1 << 24) - 1) * (1 << 104)
FLT_MIN = Fraction(1, 1 << 126)
OVERFLOW = Fraction((1 << 25) - 1) * (1 << 103)  # midpoint of FLT_MAX and 2^128: rounds to infinity
SUB_MAX = Fraction((1 << 23) - 1, 1 << 149)
SUB_MIN = Fraction(1, 1 << 149)


def well_formed(token: str) -> bool:
    return _NUM.match(token) is not None


@lru_cache(maxsize=None)
def scan(token: str):
    """(neg, mant, exp10, ndigits) with value = mant * 10^exp10; mant and ndigits as the parsers count
    them: leading zeros dropped, trailing zeros kept.  None for a malformed token."""
    m = _NUM.match(token)
    if m is None:
        return None
    sign, ip, fp, ex = m.groups()
    fp = fp or ""
    digits = (ip + fp).lstrip("0")
    return sign == "-", int(digits or "0"), int(ex or "0") - len(fp), len(digits)


def _magnitude(token: str):
    """|value| as a Fraction, or "inf" / "tiny" when it is far outside fp32 (keeps 10^99999 off the heap)."""
    neg, mant, exp10, nd = scan(token)
    if mant == 0:
        return Fraction(0)
    if exp10 + nd > 60:
        return "inf"  # >= 10^60 > 2^128
    if exp10 + nd < -60:
        return "tiny"  # < 10^-60 < 2^-151
    return Fraction(mant) * Fraction(10) ** exp10


def _floor_log2(x: Fraction) -> int:
    e = x.numerator.bit_length() - x.denominator.bit_length()
    if Fraction(2) ** e > x:
        e -= 1
    return e


def _round_half_even(q: Fraction) -> int:
    n = q.numerator // q.denominator
    r = q - n
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and n & 1):
        n += 1
    return n


@lru_cache(maxsize=None)
def f32_bits(token: str):
    s = scan(token)
    assert s is not None, token
    sign = 0x80000000 if s[0] else 0
    x = _magnitude(token)
    if x == "inf":
        return None
    if x == "tiny" or x == 0:
        return sign
    e = max(_floor_log2(x), -126)  # subnormals share the 2^-149 grid of the lowest binade
    n = _round_half_even(x / Fraction(2) ** (e - 23))
    bits = ((e + 127) << 23) + n - (1 << 23)  # n == 2^24 carries into the exponent; subnormal n < 2^23 -> exponent 0
    return None if bits >= 0x7F800000 else sign | bits


@lru_cache(maxsize=None)
def midpoint_distance(token: str) -> Fraction:
    x = _magnitude(token)
    if x == "inf" or x == "tiny" or x == 0:
        return Fraction(1)
    e = max(_floor_log2(x), -126)
    ulp = Fraction(2) ** (e - 23)
    k = (x / ulp).numerator // (x / ulp).denominator  # x in [k ulp, (k + 1) ulp)
    cands = [(k + Fraction(1, 2)) * ulp]
    if k > (1 << 23) or e == -126:
        cands.append((k - Fraction(1, 2)) * ulp)
    else:  # first interval of a binade: the boundary below lies in the binade below (half the spacing)
        cands.append(k * ulp - ulp / 4)
    return min(abs(x - c) for c in cands) / x


@lru_cache(maxsize=None)
def must_accept(token: str) -> bool:
    """The device must convert this token itself (status 0): see decode.hip's header.  The hazard
    window of the double path is at most 5 ulp(double) wide on top of at most 4 ulp of accumulated
    error, below 2^-48 relative; 2^-44 leaves slack and is still far tighter than random input gets."""
    s = scan(token)
    if s is None or len(token) > 64:
        return False
    neg, mant, exp10, nd = s
    if nd > 19 or not -66 <= exp10 <= 66:
        return False
    if mant == 0:
        return True
    x = _magnitude(token)
    if x in ("inf", "tiny"):
        return False
    eps = Fraction(1, 1 << 20)
    if not FLT_MIN * (1 + eps) <= x <= FLT_MAX * (1 - eps):
        return False
    if mant <= (1 << 24) and -10 <= exp10 <= 10:
        return True
    return midpoint_distance(token) >= Fraction(1, 1 << 44)


# ---- corpora ---------------------------------------------------------------------------------------

def _digits_of(x: Fraction, nd: int):
    """(D, k): D = floor(x / 10^k) has exactly nd digits."""
    k = len(str(x.numerator // x.denominator)) - nd if x >= 1 else -nd
    while True:
        D = (x / Fraction(10) ** k).numerator // (x / Fraction(10) ** k).denominator
        if D >= 10 ** nd:
            k += 1
        elif D < 10 ** (nd - 1):
            k -= 1
        else:
            return D, k


def _plain(D: int, k: int):
    """D * 10^k written without an exponent, or None above 64 bytes."""
    s = str(D)
    if k >= 0:
        t = s + "0" * k
    elif len(s) > -k:
        t = s[:k] + "." + s[k:]
    else:
        t = "0." + "0" * (-k - len(s)) + s
    return t if len(t) <= 64 else None


NEAR_ND = (9, 12, 16, 17, 18, 19)
NEAR_JITTER = (-3, -2, -1, 0, 1, 2, 3)


def near_midpoints(nd: int, jitter: int, n: int = 48, seed: int = 0, plain: bool = True):
    """Random fp32 midpoints (binary exponent in [-40, 40]) cut to nd significant digits, moved by
    `jitter` units in the last place; as <digits>e<exp> and, where it fits, as ddd.ddd."""
    rng = random.Random(1000 * nd + 10 * jitter + seed)
    out = []
    for _ in range(n):
        m = rng.randrange(1 << 23, 1 << 24)
        e = rng.randrange(-40, 41)
        mid = Fraction(2 * m + 1) * Fraction(2) ** (e - 24)
        D, k = _digits_of(mid, nd)
        D += jitter
        sign = "-" if rng.random() < 0.25 else ""
        out.append("%s%de%d" % (sign, D, k))
        p = _plain(D, k)
        if plain and p is not None:
            out.append(sign + p)
    return out


def off_midpoints(nd: int, n: int = 40, seed: int = 0):
    """fp32 midpoints written with nd >= 17 digits and moved away by 1.01, 2 and 16 times 2^-44
    relative: the closest tokens the device must still convert itself, on either side."""
    rng = random.Random(77 * nd + seed)
    out = []
    for i in range(n):
        m = rng.randrange(1 << 23, 1 << 24)
        e = rng.randrange(-40, 41)
        mid = Fraction(2 * m + 1) * Fraction(2) ** (e - 24)
        D, k = _digits_of(mid, nd)
        for c in (Fraction(101, 100), 2, 16):
            step = int(D * c / (1 << 44)) + 2
            for D2 in (D - step, D + step + 1):
                out.append("%s%de%d" % ("-" if i % 4 == 0 else "", D2, k))
                p = _plain(D2, k)
                if p is not None and i % 2:
                    out.append(p)
    return out


def long_forms(n: int = 40, seed: int = 0):
    """Tokens of 33 to 64 bytes with hard values: 17-19 digit neighbours of midpoints between 2^-110
    and 2^-50 written as 0.000...ddd, and the same digits behind a zero-padded exponent."""
    rng = random.Random(31 + seed)
    out = []
    for i in range(n):
        nd = (17, 18, 19)[i % 3]
        m = rng.randrange(1 << 23, 1 << 24)
        mid = Fraction(2 * m + 1) * Fraction(2) ** (rng.randrange(-110, -49) - 24)
        D, k = _digits_of(mid, nd)
        step = int(D * (1 + i % 5) / (1 << 44)) + 2
        for D2 in (D - step, D + step + 1, D + (i % 7) - 3):
            out.append(("-" if i % 4 == 0 else "") + _plain(D2, k))
            out.append(_pad_exp(str(D2), k, (33, 48, 63, 64)[i % 4]))
    return out


def fastpath_edge(n: int = 150, seed: int = 0):
    """Mantissas around the 2^24 bound of the single-rounding fp32 path, at every power of ten that
    path takes: above the bound float(mant) is itself rounded, so mant / 10^k rounds twice."""
    rng = random.Random(5 + seed)
    out = []
    for i in range(n):
        m = rng.randrange((1 << 24) + 1, 1 << 25) | 1 if i % 3 else rng.randrange(10 ** 7, 1 << 24)
        s = str(m)
        for k in (1, 3, 7, 8):
            out.append(s[:-k] + "." + s[-k:] if k < 8 else "0." + s)
        out.append(s)
        out.append("%se%d" % (s, rng.randrange(-10, 11)))
        out.append("-%s.%se%d" % (s[0], s[1:], rng.randrange(-3, 4)))
    return out


def exact_ties():
    """Decimal tokens that ARE fp32 midpoints (ties to even decides), each with a neighbour just above
    and just below it."""
    out = []
    for b in (24, 25, 26, 27, 30):
        step = 1 << (b - 23)
        for j in (0, 1, 2, 5):
            t = (1 << b) + step // 2 + j * step
            out += [str(t), "%d.0001" % t, "%d.9999" % (t - 1), "%d.%s1" % (t, "0" * (18 - len(str(t)))),
                    "%d.%s" % (t - 1, "9" * (19 - len(str(t - 1)))), "%de0" % t, "%d.0e0" % t, "%d0e-1" % t,
                    "%s.%se%d" % (str(t)[0], str(t)[1:], len(str(t)) - 1)]
    # ulp 1, 0.5, 0.25: x.5 / x.25 / x.125 forms
    for base, frac in ((1 << 23, "5"), ((1 << 23) + 1, "5"), ((1 << 24) - 1, "5"), (1 << 22, "25"), (1 << 22, "75"),
                       ((1 << 22) + 7, "25"), (1 << 21, "125"), ((1 << 21) + 2, "375"), (1, "000000059604644775390625"),
                       (3, "00000011920928955078125")):
        t = "%d.%s" % (base, frac)
        out += [t, t + "0001", t[:-1] + str(int(t[-1]) - 1) + "9999", "-" + t]
    return out


BOUNDARY_MANTS = ((1 << 24) - 1, 1 << 24, (1 << 24) + 1, (1 << 53) - 1, 1 << 53, (1 << 53) + 1, 10 ** 19 - 1)
BOUNDARY_EXPS = (-11, -10, 10, 11, -23, -22, 22, 23, -67, -66, 66, 67)


def boundaries():
    out = ["%de%d" % (m, e) for m in BOUNDARY_MANTS for e in BOUNDARY_EXPS]
    out += [str(m) for m in BOUNDARY_MANTS] + ["-%d.0" % m for m in BOUNDARY_MANTS]
    for v in (FLT_MAX, OVERFLOW, FLT_MIN, SUB_MAX, SUB_MIN, SUB_MIN / 2):
        for nd in (9, 17, 19):
            D, k = _digits_of(v, nd)
            for j in (-2, -1, 0, 1, 2):
                out.append("%de%d" % (D + j, k))
                out.append("-%s.%se%d" % (str(D + j)[0], str(D + j)[1:], k + nd - 1))
    # the exact integers around FLT_MAX and the overflow threshold (39 digits)
    for v in (FLT_MAX, OVERFLOW):
        n = v.numerator
        out += [str(n - 1), str(n), str(n + 1), "-%d" % n, "%d.5" % n, "%d.5" % (n - 1)]
    out += ["3.4028234663852886e38", "3.4028235677973366e38", "3.4028235677973367e38", "3.4028235677973365e38",
            "1.1754943508222875e-38", "1.1754942106924411e-38", "1.401298464324817e-45", "7.006492321624085e-46",
            "7.006492321624086e-46", "1e39", "-1e39", "1e-46", "-1e-46", "2e-45", "1e38", "1e-37"]
    return out


def _pad_exp(mant: str, e: int, length: int):
    """mant + 'e' + sign + zero-padded exponent, exactly `length` bytes."""
    sign = "-" if e < 0 else ""
    digits = length - len(mant) - 1 - len(sign)
    assert digits >= len(str(abs(e)))
    return "%se%s%0*d" % (mant, sign, digits, abs(e))


FORM_LENGTHS = (10, 11, 32, 33, 63, 64, 65)


def forms():
    out = ["1E5", "1e+5", "1e-05", "1e0005", "0e99999", "-0e-400", "-0", "-0.000", "0", "0.0", "0e0", "0E+0", "1", "-1",
           "9", "10", "1.0", "1.5E+3", "-2.5e-3", "12345678", "123456789", "0.12345678", "0.123456789", "16777216",
           "16777217", "99999999", "0.00000001"]
    for z in (20, 21, 26, 30, 31, 36, 37, 38, 44, 45, 50, 58):
        for d in ("1", "9", "125", "17014118346046923", "1234567890123456789"):
            out.append("0." + "0" * z + d)
    out += ["1234567890123456789" + "0" * z for z in (1, 2, 5, 19)]  # 19 digits, then zeros
    out += ["12345678901234567890", "99999999999999999999", "-18446744073709551616", "1234567890123456789.5",
            "0.12345678901234567890", "1.2345678901234567891e5"]  # 20 digits
    for n in FORM_LENGTHS:
        out.append(_pad_exp("1.5", 7, n))
        out.append(_pad_exp("-3.0000001192092896", -5, n) if n >= 32 else _pad_exp("-3", -5, n))
        if n <= 33:
            out.append(("0." + "0" * (n - 2 - 8) + "16777217") if n > 11 else "0.123456789012345"[:n])
            out.append("-" + "1234567.8901234567890123456789012345"[:n - 1])
        else:
            out.append("0." + "0" * 30 + "16777217" + "e" + "0" * (n - 43) + "25")
    return out


def ordinary(n: int = 400, seed: int = 0):
    """The formats of test_gpu_decode._texts(): what serializers emit for image-like data."""
    rng = np.random.default_rng(seed)
    u = rng.random(n)
    s = rng.standard_normal(n).astype(np.float32)
    out = ["%.4f" % x for x in u]
    out += ["%.7f" % x for x in (u * 6 - 3)]
    out += [repr(float(x)) for x in s]
    out += [repr(float(x)) for x in rng.random(n)]
    out += [str(int(x)) for x in rng.integers(-100000, 100000, n)]
    out += ["%.6e" % x for x in s * 10.0 ** rng.integers(-15, 15, n)]
    out += ["0", "-0", "0.0", "-0.000", "0e5"]
    out += ["%.17g" % x for x in rng.random(n) * 1e3]
    return out


MALFORMED = ["1.", ".5", "01", "abc", "", "[1]", '"1"', "1e", "+1", "--1", "nan", "1 2", "1e+-5", "1e-+5", "-", "-.5",
             "1.e5", "00", "-01"]


# Well formed but outside the device contract: the device must hand these to the host (status bit 1).
OUT_OF_CONTRACT = [
    "12345678901234567890", "1234567890123456789.5", "0.12345678901234567890", "1234567890123456789000",  # > 19 digits
    "1e67", "-1e-67", "1.5e68", "123e-69", "1e99999", "1e-99999",  # exp10 outside [-66, 66]
    "1e-40", "1.1754942e-38", "1e-45", "-7.006492321624085e-46",  # subnormal / underflow
    "3.5e38", "1e39", "-3.4028236e38", "340282356779733661637539395458142568448",  # overflow
    _pad_exp("1.5", 7, 65), _pad_exp("-2.5", -3, 66), _pad_exp("1", 0, 80), "0." + "0" * 30 + "16777217e" + "0" * 22 + "25",
    "1." + "0" * 70,  # longer than 64 bytes
]


# The edge of the device's hazard window.  Following decode.hip's documented steps in IEEE doubles
# (mantissa to double, then one exact power of ten <= 1e22 per step, r roundings in all), these tokens
# land r + 1 ulp(double) from a float midpoint (the last position inside the window) or r + 2 (the
# first one outside), below and above it, for r = 1, 2, 3.  Whichever way the device decides, an
# accepted value must be exact.
WINDOW_EDGE = [
    "283474928232038340e0", "283474928232038341e0", "283474928232038448e0", "283474928232038449e0",
    "38677599987171301e0", "38677599987171302e0", "38677599987171349e0", "38677599987171350e0",
    "15391181659651911e-20", "15391181659651912e-20", "15391181659651927e-20", "15391181659651928e-20",
    "15391181659651910e-20", "15388633608818046e-16", "15391181659651930e-20", "15391181659651931e-20",
    "14442687490401334e-24", "10259672343464190e-28", "14442687490401346e-24", "10259672343464207e-28",
    "14442687490401331e-24", "14442687490401332e-24", "14442687490401347e-24", "14442687490401348e-24",
]


# Tokens that once exposed a converter bug: name -> token.
REGRESSIONS = {
    # decode.hip converted a well-formed token of more than 64 bytes when it was not its chunk's last
    # token (only the chunk's last token met the 64-byte halo limit); the contract says status bit 1.
    "inner_token_65_bytes": _pad_exp("1.5", 7, 65),
    "inner_token_80_bytes": _pad_exp("-2.5", -3, 80),
}


# What the device must flag: malformed text and everything outside its contract.
DEVICE_REJECTS = MALFORMED + OUT_OF_CONTRACT + ["1,,2", "1,", "1" * 70, "1e-50", "3e39"] + list(REGRESSIONS.values())


def device_classes(corp):
    """(class of each distinct token, must-accept tokens, may-fall-back tokens) of corpora()."""
    cls = {}
    for name, toks in corp.items():
        for t in toks:
            cls.setdefault(t, name)
    return cls, [t for t in cls if must_accept(t)], [t for t in cls if not must_accept(t)]


def corpora():
    """name -> tokens (all well formed)."""
    c = {"near_nd%d" % nd: [t for j in NEAR_JITTER for t in near_midpoints(nd, j)] for nd in NEAR_ND}
    c["off_mid"] = [t for nd in (17, 18, 19) for t in off_midpoints(nd)]
    c["long_forms"] = long_forms()
    c["fastpath_edge"] = fastpath_edge()
    c["window_edge"] = WINDOW_EDGE + ["-" + t for t in WINDOW_EDGE]
    c["exact_ties"] = exact_ties()
    c["boundaries"] = boundaries()
    c["forms"] = forms()
    c["ordinary"] = ordinary()
    c["regressions"] = list(REGRESSIONS.values())
    return c
