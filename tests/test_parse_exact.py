"""Host number parsers (csrc/core/json.cpp) against the exact oracle of decimal_oracle.py.

The host has no fallback: every well-formed token must come back as the correctly rounded fp32, bit for
bit, subnormals included, whichever converter meets it.  Each corpus is therefore sent
  * in arrays long enough for the bulk path (token pairs inside a 64-byte block, single tokens across
    block edges), behind pads that move the block phase over all 64 positions,
  * in arrays of 1 to 3 tokens (the strict scanner, and the SWAR converter where 20 bytes follow),
  * and again with the SIMD token converters switched off (scalar parse_token).
"""
from fractions import Fraction

import numpy as np
import pytest

import decimal_oracle as O

CORPORA = O.corpora()
INF = 0x7F800000


def expected_bits(tok: str) -> int:
    b = O.f32_bits(tok)
    if b is None:  # the magnitude rounds to infinity: slow_float mirrors strtof, which returns +-inf
        return INF | (0x80000000 if tok.startswith("-") else 0)
    return b


def _parse(native, text: str, n: int, tail_first: bool = False):
    if tail_first:
        body = '{"input_data":[%s],"request_id":"a-request-id-of-some-length"}' % text
    else:
        body = '{"request_id":"r","input_data":[%s]}' % text
    _, out, cnt = native.parse_infer(body.encode(), n)
    assert cnt == n, (cnt, n, text[:80])
    return out.view(np.uint32)


def _pad(shift: int):
    """Tokens of 1-7 digits whose text, commas included, is `shift` bytes (shift 0 or >= 2)."""
    out = []
    while shift:
        k = shift if shift <= 8 else (8 if shift >= 10 else shift - 2)
        out.append("7" * (k - 1))
        shift -= k
    return out


def _is_simple(tok: str) -> bool:
    """Plain decimals short enough for the bulk path's converters (<= 17 bytes after the sign)."""
    return "e" not in tok and "E" not in tok and len(tok.lstrip("-")) <= 17


def _check(native, tokens, pads=(), tail_first=False):
    toks = list(pads) + list(tokens)
    got = _parse(native, ",".join(toks), len(toks), tail_first)
    return [(t, hex(int(g)), hex(expected_bits(t))) for t, g in zip(toks, got) if int(g) != expected_bits(t)]


def _bulk_runs(native, tokens, shifts):
    bad = []
    simple = [t for t in tokens if _is_simple(t)]
    # a token the bulk path declines ends the bulk path for the rest of its array, so the simple tokens
    # also go in short arrays (still above the 88 bytes the bulk path needs): one decline costs little
    groups = [simple[i:i + 48] for i in range(0, len(simple), 48)]
    for s in shifts:
        pads = _pad(s)
        for g in groups:
            bad += _check(native, g, pads)
    for s in shifts[:2]:
        bad += _check(native, tokens, _pad(s))  # the whole corpus as one array, every form mixed
    return bad


@pytest.mark.parametrize("name", list(CORPORA))
def test_long_arrays_every_block_phase(native, name):
    bad = _bulk_runs(native, CORPORA[name], [0] + list(range(2, 65)))
    assert not bad, (len(bad), bad[:5])


@pytest.mark.parametrize("name", list(CORPORA))
def test_short_arrays_strict_scanner(native, name):
    toks = CORPORA[name]
    bad, i, k = [], 0, 0
    while i < len(toks):
        size = 1 + k % 3
        bad += _check(native, toks[i:i + size], tail_first=bool(k & 1))
        i += size
        k += 1
    assert not bad, (len(bad), bad[:5])


@pytest.mark.parametrize("name", list(CORPORA))
def test_simd_token_path_off(native, name):
    native.set_json_simd(False)
    try:
        bad = _bulk_runs(native, CORPORA[name], [0] + list(range(2, 65, 5)))
    finally:
        native.set_json_simd(True)
    assert not bad, (len(bad), bad[:5])


def test_overflow_and_underflow_pinned(native):
    """What json.cpp does outside fp32's range, read from slow_float: from_chars reports a range error,
    strtof then gives +-inf above the overflow threshold and the correctly rounded subnormal or +-0
    below the normal range.  No error is raised."""
    over = ["3.4028235677973367e38", "340282356779733661637539395458142568448", "1e39", "-1e39", "3.5e38", "1e99999",
            "-12345678901234567890e30", "1e67"]
    under = ["7.006492321624085e-46", "-7.006492321624085e-46", "1e-46", "1e-99999", "-1e-67", "0." + "0" * 58 + "9"]
    for t in over:
        assert O.f32_bits(t) is None, t
    for t in under:
        assert O.f32_bits(t) in (0, 0x80000000), t
    assert O.f32_bits("7.006492321624086e-46") == 1 and O.f32_bits("3.4028235677973365e38") == 0x7F7FFFFF
    bad = _check(native, over + under) + _check(native, over + under, tail_first=True)
    for t in over + under:
        bad += _check(native, [t])
    assert not bad, bad


def test_oracle_on_known_values():
    """The oracle against values known from the format itself (no parser involved)."""
    known = {"0": 0, "-0": 0x80000000, "-0.000": 0x80000000, "0e99999": 0, "-0e-400": 0x80000000, "1": 0x3F800000,
             "1E5": 0x47C35000, "1e+5": 0x47C35000, "1e-05": 0x3727C5AC, "1e0005": 0x47C35000, "0.1": 0x3DCCCCCD,
             "16777216": 0x4B800000, "16777217": 0x4B800000, "16777218": 0x4B800001, "16777219": 0x4B800002,
             "16777217.0001": 0x4B800001, "16777216.9999": 0x4B800000, "33554434": 0x4C000000, "33554438": 0x4C000002,
             "3.4028234663852886e38": 0x7F7FFFFF, "3.4028235677973366e38": 0x7F7FFFFF, "3.4028235677973367e38": None,
             "1.1754943508222875e-38": 0x00800000,
             "1.1754942106924411e-38": 0x007FFFFF, "1.401298464324817e-45": 1, "7.006492321624085e-46": 0,
             "-7.006492321624086e-46": 0x80000001}
    for t, b in known.items():
        assert O.f32_bits(t) == b, (t, O.f32_bits(t), b)
    for t in ("16777217", "8388608.5", "1.000000059604644775390625"):
        assert O.midpoint_distance(t) == 0
    assert O.midpoint_distance("16777217.5") == Fraction(1, 33554435)  # 0.5 above the midpoint 16777217
    assert O.midpoint_distance("16777216.125") == Fraction(5, 134217729)  # 0.625 above 16777215.5, in the binade below
    assert O.must_accept("0.1234") and O.must_accept("16777216") and O.must_accept("-0e5")
    for t in ("16777217", "1e-40", "3.5e38", "12345678901234567890", "1e67", "1e-67", "01", "1" * 65, "1e" + "0" * 63):
        assert not O.must_accept(t), t
    # a double within fp32's normal range that is far from a midpoint casts to the same bits
    for name, toks in CORPORA.items():
        for t in toks:
            b = O.f32_bits(t)
            if b is not None and (b & 0x7FFFFFFF) >= 0x00800000 and O.midpoint_distance(t) > Fraction(1, 1 << 40):
                assert int(np.float32(float(t)).view(np.uint32)) == b, (name, t)


def test_device_classes_cover_every_converter():
    """The split the GPU tests use (checked here, where no GPU is needed): enough must-accept tokens of
    <= 10, 11-32 and 33-64 bytes to reach each device converter, hard values among them."""
    cls, must, may = O.device_classes(CORPORA)
    assert len(must) > 3000 and len(may) > 2000
    assert all(O.well_formed(t) for t in cls)
    assert not any(O.must_accept(t) for t in O.DEVICE_REJECTS)
    lens = [len(t) for t in must]
    assert min(lens) == 1 and max(lens) == 64
    assert sum(n <= 10 for n in lens) > 500 and sum(10 < n <= 32 for n in lens) > 500 and sum(n > 32 for n in lens) > 100
    assert sum(O.scan(t)[3] >= 17 and O.midpoint_distance(t) < Fraction(1, 1 << 39) for t in must) > 500
    assert sum(O.midpoint_distance(t) == 0 for t in may) > 50


def test_corpus_power_naive_conversion_fails():
    """Pure Python, no project code: "double product, then cast" must get at least a quarter of the
    18- and 19-digit near-midpoint tokens wrong, or the corpus has gone soft."""
    toks = [t for nd in (18, 19) for j in O.NEAR_JITTER for t in O.near_midpoints(nd, j, plain=False)]
    wrong = 0
    for t in toks:
        neg, mant, exp10, _ = O.scan(t)
        d = float(mant) * 10.0 ** exp10 if exp10 >= 0 else float(mant) / 10.0 ** -exp10
        b = int(np.float32(-d if neg else d).view(np.uint32))
        wrong += b != O.f32_bits(t)
    print("naive conversion wrong on %d of %d (%.0f%%)" % (wrong, len(toks), 100.0 * wrong / len(toks)))
    assert wrong >= 0.25 * len(toks), (wrong, len(toks))
