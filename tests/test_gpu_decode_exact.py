"""Device JSON decode (csrc/kernels/decode.hip) against the exact oracle of decimal_oracle.py, on every
route a token can take to a converter.

Three classes of token, three requirements:
  must accept   (decimal_oracle.must_accept)  status 0, exact token count, every value == f32_bits
  may fall back (every other well-formed one) status bit 1, or status 0 and the value == f32_bits
  malformed / out of contract                 status bit 1
Nothing is skipped on status: a must-accept sample that comes back flagged fails its test.

Routes (the converter that runs depends on them): no blank at all; one ", " early in the sample (the
chunk's hot path off); blanks around every token (byte-wise converter); a leading pad of 1-4 bytes (all
four start alignments); the hard token across a 64-byte lane region, across the 4096-byte chunk edge, as
a chunk's last token, as the sample's last token; 4-bit packed upload on the nibble kernels; packed
upload on the character kernels (decode variant 1).
"""
import numpy as np
import pytest

import decimal_oracle as O
from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

CORPORA = O.corpora()
CLASS, MUST, MAY = O.device_classes(CORPORA)
BAD = O.DEVICE_REJECTS
PER_SAMPLE = 300   # tokens per must-accept sample
LAUNCH = 1024      # samples per launch (kDecMaxB)
BLANKS = " \n\t\r"


def _bits(tok):
    b = O.f32_bits(tok)
    assert b is not None, tok
    return b


def _decode(texts, numel, packed=False):
    from die_amd.ops import kernels as K

    v, s, n = K.decode_json_numbers(texts, numel, packed=packed)
    return v.cpu().numpy().view(np.uint32), s.cpu().numpy(), n.cpu().numpy()


def _pad_tokens(nbytes):
    """Short tokens whose text, each with its comma, is exactly nbytes long."""
    assert nbytes >= 0 and nbytes not in (1,)
    q, r = divmod(nbytes, 4)
    if r == 1:
        return ["0.5"] * (q - 1) + ["0.25"]
    return ["0.5"] * q + {0: [], 2: ["1"], 3: ["12"]}[r]


def _blanked(i, tok):
    """Blanks around a token; the text between two separators stays within the 64 bytes the device
    converts, so a 63-byte token gets one blank and a 64-byte token none."""
    room = max(0, 64 - len(tok))
    lead = BLANKS[i % 4] if room >= 1 else ""
    trail = BLANKS[(i // 4) % 4] if room >= 2 else ""
    return lead + tok + trail


# layout(tokens) -> (text, tokens as decoded): how one sample's tokens become text
def _plain(toks):
    return ",".join(toks), toks


def _one_blank(toks):
    return toks[0] + ", " + ",".join(toks[1:]), toks


def _all_blanks(toks):
    return ",".join(_blanked(i, t) for i, t in enumerate(toks)), toks


def _lead_pad(k):
    def f(toks):
        toks = ["1" * k] + list(toks)
        return ",".join(toks), toks
    return f


def _at(offset_of):
    """The sample's middle token starts at byte offset_of(len(token), i) behind a pad of short tokens."""
    def f(toks, i=0):
        first, tok, last = toks
        pad = _pad_tokens(offset_of(len(tok), i))
        toks = pad + [tok] + ([last] if last is not None else [])
        return ",".join(toks), toks
    return f


LAYOUTS = {
    "no_blank": _plain,
    "one_blank": _one_blank,
    "all_blanks": _all_blanks,
    "pad1": _lead_pad(1), "pad2": _lead_pad(2), "pad3": _lead_pad(3), "pad4": _lead_pad(4),
}
# the hard token's start; i varies the position from sample to sample
PLACEMENTS = {
    "across_lane_region": lambda L, i: 64 * (2 + i % 5) - max(1, L // 2),
    "across_chunk_edge": lambda L, i: 4096 - max(1, (L * (1 + i % 3)) // 4),
    "ends_chunk": lambda L, i: 4096 - L - (i & 1),  # its ',' is the chunk's last byte, or the next chunk's first
    "ends_sample": lambda L, i: 192 + 4 * (i % 16) + 2 * (i % 2),
}


def _thin(tokens, limit):
    step = -(-len(tokens) // limit)
    return tokens[::step]


def _check_samples(groups, texts, packed=False, require_accept=True):
    """groups[i]: the tokens of sample i in order.  Returns (accepted, fallen back) sample indices."""
    numel = max(len(g) for g in groups)
    accepted, fell = [], []
    for b0 in range(0, len(texts), LAUNCH):
        vals, status, ntok = _decode(texts[b0:b0 + LAUNCH], numel, packed)
        for j, g in enumerate(groups[b0:b0 + LAUNCH]):
            st = int(status[j])
            if not require_accept and st & 1:
                fell.append(b0 + j)
                continue
            assert st == 0, (st, g[:3], len(g), texts[b0 + j][:120])
            assert int(ntok[j]) == len(g), (int(ntok[j]), len(g), g[:3])
            want = np.array([_bits(t) for t in g], np.uint32)
            got = vals[j, :len(g)]
            if not np.array_equal(got, want):
                k = int(np.flatnonzero(got != want)[0])
                raise AssertionError("token %r (class %s): device %#x, exact %#x" %
                                     (g[k], CLASS.get(g[k], "pad"), int(got[k]), int(want[k])))
            assert not vals[j, len(g):].any()
            accepted.append(b0 + j)
    return accepted, fell


def _report(title, tokens, accepted, fell):
    acc, fb = {}, {}
    for i in accepted:
        acc[CLASS[tokens[i]]] = acc.get(CLASS[tokens[i]], 0) + 1
    for i in fell:
        fb[CLASS[tokens[i]]] = fb.get(CLASS[tokens[i]], 0) + 1
    print("%s: %s" % (title, ", ".join("%s %d accepted / %d fell back" % (c, acc.get(c, 0), fb.get(c, 0))
                                        for c in CORPORA if c in acc or c in fb)))


def _must_samples(layout, lower=False):
    toks = [t.replace("E", "e") for t in MUST] if lower else MUST
    groups, texts = [], []
    for i in range(0, len(toks), PER_SAMPLE):
        text, g = layout(toks[i:i + PER_SAMPLE])
        groups.append(g)
        texts.append(text.encode())
    return groups, texts


def _may_samples(layout, lower=False):
    groups, texts = [], []
    for t in MAY:
        text, g = layout(["0.5", t.replace("E", "e") if lower else t, "0.25"])
        groups.append(g)
        texts.append(text.encode())
    return groups, texts


@pytest.mark.parametrize("route", list(LAYOUTS))
def test_must_accept_exact(native, route):
    groups, texts = _must_samples(LAYOUTS[route])
    accepted, _ = _check_samples(groups, texts)
    assert len(accepted) == len(groups)  # share of must-accept samples left uncompared: 0


@pytest.mark.parametrize("route", list(LAYOUTS))
def test_may_fall_back_exact_or_flagged(native, route):
    groups, texts = _may_samples(LAYOUTS[route])
    accepted, fell = _check_samples(groups, texts, require_accept=False)
    assert len(accepted) + len(fell) == len(MAY)
    _report("may fall back, " + route, MAY, accepted, fell)


@pytest.mark.parametrize("place", list(PLACEMENTS))
def test_must_accept_exact_placed(native, place):
    """One hard token per sample, placed by a pad of short tokens; pads and neighbours exact too."""
    lay = _at(PLACEMENTS[place])
    toks = _thin([t for t in MUST if len(t) > 10 and CLASS[t] != "ordinary"], LAUNCH)
    last = None if place == "ends_sample" else "0.25"
    groups, texts = [], []
    for i, t in enumerate(toks):
        text, g = lay(["0.5", t, last], i)
        groups.append(g)
        texts.append(text.encode())
    accepted, _ = _check_samples(groups, texts)
    assert len(accepted) == len(toks)


@pytest.mark.parametrize("place", list(PLACEMENTS))
def test_may_fall_back_placed(native, place):
    lay = _at(PLACEMENTS[place])
    toks = _thin([t for t in MAY if len(t) > 10], LAUNCH)
    last = None if place == "ends_sample" else "0.25"
    groups, texts = [], []
    for i, t in enumerate(toks):
        text, g = lay(["0.5", t, last], i)
        groups.append(g)
        texts.append(text.encode())
    accepted, fell = _check_samples(groups, texts, require_accept=False)
    _report("may fall back, " + place, toks, accepted, fell)


def _same_as_raw(texts, numel):
    raw = _decode(texts, numel)
    pk = _decode(texts, numel, packed=True)
    assert np.array_equal(pk[1], raw[1]) and np.array_equal(pk[2], raw[2])
    ok = raw[1] == 0
    assert np.array_equal(pk[0][ok], raw[0][ok])


@pytest.mark.parametrize("variant", [0, 1])
def test_packed_upload_exact_and_same_as_raw(native, variant):
    """4-bit packed upload: variant 0 decodes on the nibble kernels, variant 1 expands to characters
    for the character kernels.  Oracle-exact, and status, count and bits equal to the raw upload."""
    from die_amd.ops import kernels as K

    K.set_decode_variant(variant)
    try:
        groups, texts = _must_samples(_plain, lower=True)
        assert all(native.pack_nibbles(t) is not None for t in texts)
        accepted, _ = _check_samples(groups, texts, packed=True)
        assert len(accepted) == len(groups)
        _same_as_raw(texts, max(len(g) for g in groups))
        groups, texts = _may_samples(_plain, lower=True)
        assert all(native.pack_nibbles(t) is not None for t in texts)
        accepted, fell = _check_samples(groups, texts, packed=True, require_accept=False)
        _report("may fall back, packed variant %d" % variant, MAY, accepted, fell)
        for b0 in range(0, len(texts), LAUNCH):
            _same_as_raw(texts[b0:b0 + LAUNCH], 3)
    finally:
        K.set_decode_variant(0)


@pytest.mark.parametrize("route", ["no_blank", "one_blank", "all_blanks", "packed"])
def test_malformed_and_out_of_contract_flagged(native, route):
    lay = LAYOUTS.get(route, _plain)
    texts = [lay(["0.5", t, "0.25"])[0].encode() for t in BAD]
    _, status, _ = _decode(texts, 8, packed=route == "packed")
    missed = [t for t, st in zip(BAD, status) if not int(st) & 1]
    assert not missed, missed
