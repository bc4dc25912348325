"""Case grid, input families, float64 reference and element-wise error bound for the streaming
attention kernel (csrc/kernels/transformer.hip attention_stream_kernel; a plain helper module:
test_attention_oracle_bound.py runs it on the CPU, test_gpu_attention_sharp.py on the kernel).

Layout: q, O [B, S, H, D], k, v [B, S, Hkv, D] (query head h reads stored head h // (H // Hkv)), all
float64 holding exactly what the storage holds (bf16 values, or hi + lo of the split planes); the
additive terms of a mode (bias table, causal, key mask) as one [B, H, S, S] tensor with -inf = masked.

The bound.  With z_j = scale * q_i . k_j + term_ij and P_j = softmax_j(z) the reference is
O_d = sum_j P_j v_jd; A_d = sum_j P_j |v_jd|, Sx_i = scale * max_j sum_d |q_id| |k_jd| and
Bx_i = max_j |bias_ij| (both over the keys row i sees).  Every output element gets

  T = (u_p + u_ll + (exp(2 delta_i) - 1) + c * 2^-24) * A  +  u_s * (|O| + that)

whose terms follow the kernel's arithmetic (u = 2^-24 below, fp32's unit roundoff):

  p_round   P enters the second MFMA rounded to bf16, 8 significand bits: u_p = 2^-8.  fp32 mode:
            as hi + lo with lo rounded to bf16, |p - hi - lo| <= 2^-8 |p - hi| <= 2^-16 p.  (l sums the
            unrounded p, so this does not cancel.)
  lo_lo     fp32 mode computes V P as V_hi P_hi + V_lo P_hi + V_hi P_lo and drops V_lo P_lo,
            |V_lo| <= 2^-8 |V|, |P_lo| <= 2^-8 P: u_ll = 2^-16 (0 in bf16 mode).
  exponent  the kernel's exponent of key j is off by at most delta_i (natural units):
              the score: bf16 x bf16 products are exact in fp32, so only the fp32 accumulation of
                n = D (bf16) or 3 D (fp32 mode: K_hi Q_hi, K_lo Q_hi, K_hi Q_lo) terms rounds,
                <= 2 n u Sx (twice the worst case of any order, the MFMA's internal rounding not
                being known to be to nearest: conv_geometry.py's supposition);
              fp32 mode drops K_lo Q_lo: 2^-16 Sx;
              scale * log2(e) in float (the cast of scale, the constant, their product): 3 u Sx;
              the multiply or fma: u (Sx + Bx); the subtraction of the running maximum, at most
              twice as large: 2 u (Sx + Bx); the host's bias * log2(e) (constant, product): 2 u Bx.
            delta_i = (2 n + 6) u Sx + 5 u Bx (+ 2^-16 Sx).  Key j then weighs exp(z_j + e_j),
            |e_j| <= delta_i, so its share of the row moves by a factor within exp(+-2 delta_i).
  accum     c = 3 S + 4 nt + 9 for nt = ceil(S / 32) tiles: hardware exp2 at 1 ulp = 2 u, numerator
            against denominator 4; l sums S terms and the halves' shuffle, S + 1; o accumulates S
            products in the MFMA and is scaled by alpha nt times, 2 (S + nt), l scaled nt times, both
            roundings: 2 nt; 1 / l and o * (1 / l): 4.  (alpha itself multiplies l and o alike.)
  storage   the output is rounded to bf16, u_s = 2^-8, or to hi + lo, u_s = 2^-16
            (conv_geometry.storage), of the computed value: |O| plus the error so far.

None of these constants is fitted to a GPU result.  A key with p = 0 in the kernel (exp2 underflow,
the `cliff` family) is within the bound because its P is below 2^-126.

Input families (problem()): `randn`, Gaussian q, k, v * 1.5 as the other attention tests use; `spike`,
each query has one dominant key pi(i), >= 8 natural units over the rest, the first / last key of every
tile among them; `rising`, the row maximum rises by >= 20 exp2 units with every tile (the alpha
rescale of a large o); `cliff`, the maximum is in tile 0 and p underflows in all later tiles; `sunk`,
every score <= -12, so that a pad key (zero K, score 0) counted as visible would own the row -- among
Gaussian scores its share of a row is about 1e-3, below bf16's rounding of P, where no derived bound
can see it.  The structure is scaled into q after construction and asserted by the CPU test.
"""
import functools
import math

import torch

import conv_geometry as cg

MODES = ("none", "bias_shared", "bias_per_head", "causal", "causal_bias", "keymask", "keymask_holes", "keymask_bias")
FAMILIES = ("randn", "spike", "rising", "cliff", "sunk")
KT = 32    # keys per tile
QB = 128   # queries per block (multi-head mapping); GQA: four 32-query items per block
LN2 = math.log(2.0)
U = 2.0 ** -24


def _grid():
    cs = []
    # tile and block edges, head dim 64, 9 pairs: the natural block mapping
    for S, modes in ((17, ("none", "keymask")), (33, ("bias_per_head", "causal")), (64, ("causal_bias", "keymask_holes")),
                     (65, ("bias_shared", "keymask_bias")), (129, MODES), (300, ("none", "causal", "keymask_holes"))):
        cs += [(3, 3, 3, 64, S, m) for m in modes]
    # head dims (80: the third accumulator's rows 80..95 are never stored)
    for D, modes in ((32, ("none", "keymask_bias")), (80, ("none", "causal_bias", "keymask")),
                     (96, ("bias_shared", "causal")), (128, ("bias_per_head", "keymask_holes"))):
        cs += [(2, 3, 3, D, 129, m) for m in modes]
    # the XCD map: pairs % 8 == 0, two and three query blocks; the key-mask modes with eight samples
    cs += [(8 if m.startswith("keymask") else 4, 2, 2, 64, 129, m) for m in MODES]
    cs += [(4, 2, 2, 64, 300, m) for m in ("none", "bias_per_head", "causal_bias")] + [(8, 2, 2, 64, 300, "keymask_holes")]
    # grouped queries: mapped (B * Hkv % 8 == 0), groups of 2, 4 (one stored head) and 3 (unmapped)
    cs += [(4, 4, 2, 64, 129, m) for m in ("none", "causal", "keymask")]
    cs += [(4, 4, 2, 128, 65, "causal"), (8, 4, 1, 128, 129, "none"), (8, 4, 1, 64, 65, "keymask_holes"),
           (3, 6, 2, 64, 65, "keymask"), (3, 6, 2, 64, 129, "causal")]
    # the causal rotation: 192 pairs x 2 query blocks = 48 slots per XCD, per-head table
    cs += [(24, 8, 8, 32, 129, m) for m in ("causal", "causal_bias")]
    return cs


CASES = _grid()


def case_id(case):
    return "b%d_h%d_kv%d_d%d_s%d_%s" % case


def is_causal(mode):
    return mode.startswith("causal")


def is_keymask(mode):
    return mode.startswith("keymask")


def has_bias(mode):
    return "bias" in mode


def per_head(mode):
    """The modes whose table is [H, S, S]; bias_shared alone has one [S, S] table."""
    return has_bias(mode) and mode != "bias_shared"


# ---- the kernel's block map, as a model (for the grid assertions) ----------------------------------

def launch_grid(case):
    """(query blocks, heads the grid counts, B): kern::attention's grid."""
    B, H, Hkv, D, S, mode = case
    if Hkv != H:
        items = (S + KT - 1) // KT * (H // Hkv)
        return (items + 3) // 4, Hkv, B
    return (S + QB - 1) // QB, H, B


def block_map(case, xcd_map=1):
    """[(blockIdx (x, y, z), (qblk, head, image), rotation)] for every block, by the index arithmetic
    at the top of the kernel."""
    nqb, gy, gz = launch_grid(case)
    pairs = gy * gz
    out = []
    for z in range(gz):
        for y in range(gy):
            for x in range(nqb):
                qblk, h, b, rot = x, y, z, 0
                if xcd_map and pairs % 8 == 0:
                    lin = x + nqb * (y + gy * z)
                    slot = lin >> 3
                    pair = (lin & 7) * (pairs >> 3) + slot // nqb if xcd_map == 2 else (lin & 7) + 8 * (slot // nqb)
                    qblk = slot % nqb
                    if is_causal(case[5]):
                        rot = 3 * ((slot // nqb) * nqb // 32) % nqb
                        qblk = (qblk + rot) % nqb
                    h, b = pair % gy, pair // gy
                out.append(((x, y, z), (qblk, h, b), rot))
    return out


# ---- operands ---------------------------------------------------------------------------------------

_LENGTHS = (None, 0, 32, 64, 45, 1)  # visible keys of sample b (cyclic; None: all S), clipped to S


def visible(case):
    """bool [B, S] of a key-mask mode (True = visible key), else None."""
    B, H, Hkv, D, S, mode = case
    if not is_keymask(mode):
        return None
    vis = torch.zeros(B, S, dtype=torch.bool)
    for b in range(B):
        n = _LENGTHS[b % len(_LENGTHS)]
        n = S if n is None else min(n, S)
        vis[b, :n] = True
        if mode != "keymask" and n > 4:
            vis[b, 2:n - 1:5] = False  # holes; the last visible key stays, so kend = n
    return vis


def kend(vis):
    S = vis.shape[1]
    return (vis.long() * torch.arange(1, S + 1)).amax(1)


def bias_table(case, family, g):
    """fp32 table [1 or H, S, S] in natural units, or None.  bias_shared: keys j < i - 70 masked (from
    query 102 on the first tile is all -inf while the running maximum still is); bias_per_head: head 1
    masks keys j > i + 40 (trailing tiles all -inf).  Every row keeps its diagonal."""
    B, H, Hkv, D, S, mode = case
    if not has_bias(mode):
        return None
    hb = H if per_head(mode) else 1
    i = torch.arange(S)
    t = torch.randn(hb, S, S, generator=g) + torch.arange(hb)[:, None, None] * i[None, None, :] / S
    if family != "randn":
        t = t * 0.25  # the structured families get their scores from q . k
    t = t.float()
    if mode == "bias_shared":
        t[:, i[None, :] < i[:, None] - 70] = -math.inf
    if mode == "bias_per_head":
        t[1][i[None, :] > i[:, None] + 40] = -math.inf
    return t


def terms(case, table, vis):
    """The additive terms [B, H, S, S] float64 (-inf = masked) of bias table, causal flag, key mask."""
    B, H, Hkv, D, S, mode = case
    add = torch.zeros(B, H, S, S, dtype=torch.float64)
    if table is not None:
        add = add + table.double()[None]
    if is_causal(mode):
        i = torch.arange(S)
        add = add.masked_fill((i[None, :] > i[:, None])[None, None], -math.inf)
    if vis is not None:
        add = add.masked_fill(~vis[:, None, None, :], -math.inf)
    return add


def _heads(t, grp):
    """k / v [B, S, Hkv, D] -> per query head [B, S, H, D]."""
    return t if grp == 1 else t.repeat_interleave(grp, dim=2)


def scores(q, k, grp):
    return torch.einsum("bihd,bjhd->bhij", q, _heads(k, grp))


def special_keys(S):
    """First and last key of every 32-key tile and the last key of the partial tile."""
    return sorted(set(range(0, S, KT)) | set(range(KT - 1, S, KT)) | {S - 1})


def dominant_keys(case, add):
    """pi [B, H, S]: the `spike` family's dominant key of each query: the r-th of the n keys the row
    sees, r = (a i + 3) mod n with a >= 7 coprime to n -- where all rows of a pair see the same keys (no
    mask, a key mask) a bijection of them over the first n queries.  Where the set changes with the row
    (causal, the band tables) a query takes key i itself when that is a special key or i is even, so
    that every special key is some query's dominant key there too.  Rows without a visible key get 0."""
    B, H, Hkv, D, S, mode = case
    M = torch.isfinite(add)
    n = M.sum(-1)
    i = torch.arange(S)
    coprime = torch.tensor([next(a for a in range(7, 7 + max(m, 1) + 1) if math.gcd(a, max(m, 1)) == 1)
                            for m in range(S + 1)])
    r = (coprime[n] * i[None, None, :] + 3) % n.clamp_min(1)
    pick = ((M.cumsum(-1) == (r + 1)[..., None]) & M).float().argmax(-1)
    if not (is_causal(mode) or mode in ("bias_shared", "bias_per_head")):
        return pick
    own = M.diagonal(dim1=-2, dim2=-1)
    spec = torch.zeros(S, dtype=torch.bool)
    spec[special_keys(S)] = True
    spec |= i % 2 == 0
    return torch.where(own & spec[None, None, :], i[None, None, :].expand(B, H, S), pick)


def _need(target, db, ds):
    """The factor c >= 1 on q with c * ds + db >= target in every entry (ds > 0 asserted)."""
    ok = torch.isfinite(ds) & torch.isfinite(db)
    if not bool(ok.any()):
        return 1.0
    assert bool((ds[ok] > 0).all()), "the family's structure must come from q . k"
    return max(1.0, float(((target - db[ok]) / ds[ok]).max()))


def _tile_max(z):
    """[B, H, S, S] -> [B, H, S, nt] maxima over the 32-key tiles (-inf: nothing visible there)."""
    B, H, S, _ = z.shape
    Sp = (S + KT - 1) // KT * KT
    zp = torch.full((B, H, S, Sp), -math.inf, dtype=z.dtype)
    zp[..., :S] = z
    return zp.reshape(B, H, S, Sp // KT, KT).amax(-1)


def tile_tail_visible(add):
    """bool [B, H, S, nt]: the row sees one of the tile's last four keys (positions 28..31).  The
    `rising` family's rise of 20 exp2 units is required of these tiles: a tile a row sees only the
    head of (the causal diagonal, a key mask ending mid-tile, the partial last tile) rises by its share."""
    S = add.shape[-1]
    pos = torch.arange(S) % KT
    return torch.isfinite(_tile_max(add.masked_fill((pos < KT - 4)[None, None, None, :], -math.inf)))


def _make_qkv(case, family, g, add, scale):
    B, H, Hkv, D, S, mode = case
    grp = H // Hkv
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    v = rn(B, S, Hkv, D) * 1.5
    if family == "randn":
        return rn(B, S, H, D) * 1.5, rn(B, S, Hkv, D) * 1.5, v
    fin = torch.isfinite(add)
    bias = torch.where(fin, add, torch.zeros_like(add))
    if family == "spike":
        # q_i = 1.5 k_pi(i) + 0.3 noise on rows of equal norm, scaled up to a margin of 9 natural units
        k = rn(B, S, Hkv, D)
        k = 1.5 * math.sqrt(D) * k / k.norm(dim=-1, keepdim=True)
        pi = dominant_keys(case, add)
        idx = pi.permute(0, 2, 1)[..., None].expand(B, S, H, D)
        q = 1.5 * _heads(k, grp).gather(1, idx) + 0.3 * rn(B, S, H, D)
        s = scale * scores(q, k, grp)
        dom = torch.zeros_like(s, dtype=torch.bool).scatter_(-1, pi[..., None], True) & fin
        rest = fin & ~dom & dom.any(-1, keepdim=True)
        nan = torch.full_like(s, math.nan)
        ds = torch.where(rest, s.gather(-1, pi[..., None]) - s, nan)       # dominant minus every other visible key
        db = torch.where(rest, bias.gather(-1, pi[..., None]) - bias, nan)
        return q * _need(9.0, db, ds) * 1.02, k, v
    e = (torch.randint(0, 2, (D,), generator=g) * 2 - 1).double()
    j = torch.arange(S, dtype=torch.float64)
    if family == "rising":
        # the score grows by about 24 exp2 units per tile along e; q scaled up to >= 22 between the
        # maxima of consecutive visible tiles of every row
        beta = 24 * LN2 / math.sqrt(D)
        k = (j + 1)[None, :, None, None] / KT * beta * e + 0.3 * rn(B, S, Hkv, D)
        q = e + 0.1 * rn(B, S, H, D)
        s = scale * scores(q, k, grp)
        c = 1.0
        tail = tile_tail_visible(add)
        for _ in range(8):
            tm = _tile_max(torch.where(fin, c * s + bias, torch.full_like(s, -math.inf)))
            need = 1.0
            for t in range(1, tm.shape[-1]):
                both = tail[..., t] & torch.isfinite(tm[..., t - 1])
                if bool(both.any()):
                    rise = (tm[..., t] - tm[..., t - 1])[both]
                    assert bool((rise > 0).all())
                    need = max(need, float((22.5 * LN2 / rise).max()))
            if need <= 1.0:
                break
            c *= need
        return q * c, k, v
    if family == "sunk":
        # every score <= -12 natural units: a key that reads as zero K (a pad key) would own the row
        q = -3.5 * e + 1.5 * rn(B, S, H, D)
        k = 3.5 * e + 1.5 * rn(B, S, Hkv, D)
        s = scale * scores(q, k, grp)
        nan = torch.full_like(s, math.nan)
        return q * _need(12.5, torch.where(fin, -bias, nan), torch.where(fin, -s, nan)), k, v
    assert family == "cliff"
    # tile 0 holds the maximum; the later tiles lie >= 160 exp2 units below it (p underflows to 0)
    gamma = 130.0 / math.sqrt(D)
    k = rn(B, S, Hkv, D)
    k[:, KT:] = k[:, KT:] - gamma * e
    q = e + 0.1 * rn(B, S, H, D)
    s = scale * scores(q, k, grp)
    c = 1.0
    for _ in range(8):
        tm = _tile_max(torch.where(fin, c * s + bias, torch.full_like(s, -math.inf)))
        if tm.shape[-1] < 2:
            break
        later = tm[..., 1:].amax(-1)
        both = torch.isfinite(tm[..., 0]) & torch.isfinite(later)
        if not bool(both.any()):
            break
        gap = (tm[..., 0] - later)[both]
        assert bool((gap > 0).all())
        need = float((165 * LN2 / gap).max())
        if need <= 1.0:
            break
        c *= need
    return q * c, k, v


def attend(q, k, v, add, scale, grp):
    """float64 softmax(scale q k^T + add) v -> (O, A, P); a row without a visible key gives 0."""
    z = scale * scores(q, k, grp) + add
    m = z.amax(-1, keepdim=True)
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    w = torch.exp(z - m)
    l = w.sum(-1, keepdim=True)
    P = torch.where(l > 0, w / l.clamp_min(1e-300), torch.zeros_like(w))
    vq = _heads(v, grp)
    return torch.einsum("bhij,bjhd->bihd", P, vq), torch.einsum("bhij,bjhd->bihd", P, vq.abs()), P


def reference(q, k, v, add, scale, grp, table=None):
    """(O, A, Sx, Bx): O, A [B, S, H, D]; Sx, Bx [B, S, H, 1] over the keys each row sees."""
    O, A, _ = attend(q, k, v, add, scale, grp)
    fin = torch.isfinite(add)
    sx = scale * scores(q.abs(), k.abs(), grp)
    Sx = torch.where(fin, sx, torch.zeros_like(sx)).amax(-1)
    if table is None:
        Bx = torch.zeros_like(Sx)
    else:
        Bx = torch.where(fin, table.double().abs()[None].expand(add.shape), torch.zeros_like(add)).amax(-1)
    return O, A, Sx.permute(0, 2, 1)[..., None], Bx.permute(0, 2, 1)[..., None]


@functools.lru_cache(maxsize=8)
def problem(case, family, split):
    """The case's operands, references and bound, computed once and shared; callers must not modify
    them.  q, k, v: float64 of the storage's values; table: fp32 [Hb, S, S] or None; vis: bool [B, S] or
    None; add: all additive terms; O, A, Sx, Bx: reference(); T: bound()."""
    B, H, Hkv, D, S, mode = case
    grp = H // Hkv
    g = torch.Generator().manual_seed(7000 + 16 * CASES.index(case) + FAMILIES.index(family))
    scale = 1.0 / math.sqrt(D)
    vis = visible(case)
    table = bias_table(case, family, g)
    add = terms(case, table, vis)
    q, k, v = (cg.preround(t, split) for t in _make_qkv(case, family, g, add, scale))
    O, A, Sx, Bx = reference(q, k, v, add, scale, grp, table)
    p = dict(case=case, family=family, split=split, grp=grp, scale=scale, q=q, k=k, v=v, table=table, vis=vis, add=add,
             O=O, A=A, Sx=Sx, Bx=Bx)
    p["T"] = bound_of(p)
    return p


# ---- the bound --------------------------------------------------------------------------------------

TERMS = ("p_round", "lo_lo", "exponent", "accum", "storage")


def bound_of(p, without=()):
    """T [B, S, H, D] from a problem's A, Sx, Bx, |O| (module docstring).  `without`: term names left
    out -- only for the test that each term is needed."""
    B, H, Hkv, D, S, mode = p["case"]
    split = p["split"]
    A, Sx, Bx = p["A"], p["Sx"], p["Bx"]
    n = 3 * D if split else D
    nt = (S + KT - 1) // KT
    delta = ((2 * n + 6) * U + (2.0 ** -16 if split else 0.0)) * Sx + 5 * U * Bx
    rel = {"p_round": 2.0 ** -16 if split else 2.0 ** -8,
           "lo_lo": 2.0 ** -16 if split else 0.0,
           "exponent": torch.expm1(2 * delta),
           "accum": (3 * S + 4 * nt + 9) * U}
    E = sum(rel[t] for t in rel if t not in without) * A
    if "storage" not in without:
        E = E + cg.storage(p["O"].abs() + E, split)
    return E


def bound(case, family="randn", split=False):
    return problem(case, family, split)["T"]


def check(got, ref, T, what=""):
    """Assert |got - ref| <= T for every element of the [B, S, H, D] tensors (NaN is outside; there is
    no way to exempt an element); reports the count and the worst (b, s, h, d); returns the largest
    |err| / T."""
    try:
        return cg.check(got, ref, T, what)
    except AssertionError as e:
        raise AssertionError(str(e).replace("(b, oh, ow, n)", "(b, s, h, d)")) from None


# ---- a CPU model of the kernel's arithmetic -----------------------------------------------------------

def _planes(t, split):
    """float64 storage values -> the float32 planes the MFMAs read."""
    if not split:
        return [t.float()]
    hi = t.float().bfloat16().float()
    return [hi, (t - hi.double()).float()]


def emulate(p):
    """float32 model of attention_stream_kernel: 32-key tiles, online exp2 softmax with the running
    maximum, P rounded to bf16 (hi + lo in fp32 mode), the three-product scores and P V of fp32 mode, the
    storage rounding of the output.  Returns float64 [B, S, H, D]."""
    B, H, Hkv, D, S, mode = p["case"]
    split, grp = p["split"], p["grp"]
    f32 = torch.float32
    sl2 = torch.tensor(p["scale"], dtype=f32) * torch.tensor(1.4426950408889634, dtype=f32)
    qp = [t.permute(0, 2, 1, 3) for t in _planes(p["q"], split)]                  # [B, H, S, D]
    kp = [_heads(t, grp).permute(0, 2, 1, 3) for t in _planes(p["k"], split)]
    vp = [_heads(t, grp).permute(0, 2, 1, 3) for t in _planes(p["v"], split)]
    fin = torch.isfinite(p["add"])
    if p["table"] is not None:
        t2 = (p["table"] * 1.4426950408889634)[None].expand(B, -1, -1, -1)         # the host's fp32 table
        t2 = t2.expand(B, H, S, S)
    m = torch.full((B, H, S), -math.inf, dtype=f32)
    l = torch.zeros(B, H, S, dtype=f32)
    o = torch.zeros(B, H, S, D, dtype=f32)
    for j0 in range(0, S, KT):
        j1 = min(j0 + KT, S)
        kt = [t[:, :, j0:j1] for t in kp]
        sc = qp[0] @ kt[0].transpose(-1, -2)
        if split:
            sc = (qp[0] @ kt[1].transpose(-1, -2) + qp[1] @ kt[0].transpose(-1, -2)) + sc
        x = sc * sl2 if p["table"] is None else sc * sl2 + torch.where(fin[..., j0:j1], t2[..., j0:j1], 0.0)
        x = torch.where(fin[..., j0:j1], x, torch.full_like(x, -math.inf))
        mn = torch.maximum(m, x.amax(-1))
        m0 = torch.where(torch.isfinite(mn), mn, torch.zeros_like(mn))
        alpha = torch.exp2(m - m0)
        pr = torch.exp2(x - m0[..., None])
        l = l * alpha + pr.sum(-1)
        ph = pr.bfloat16().float()
        pv = ph @ vp[0][:, :, j0:j1]
        if split:
            pl = (pr - ph).bfloat16().float()
            pv = (ph @ vp[1][:, :, j0:j1] + pl @ vp[0][:, :, j0:j1]) + pv
        o = o * alpha[..., None] + pv
        m = mn
    inv = torch.where(l > 0, 1.0 / l, torch.zeros_like(l))
    out = (o * inv[..., None]).permute(0, 2, 1, 3).contiguous()
    return cg.preround(out, split)


# ---- subtly wrong kernels -----------------------------------------------------------------------------

# The family a mutant is judged on where Gaussian inputs cannot show it: the share of one key among S
# Gaussian scores is about 1 / S or less, which for a single row (the last key under the causal flag is
# seen by the last query alone) or a key scoring 0 can lie below bf16's rounding of P.  On `spike` the
# last key is its own query's dominant key; on `sunk` a key scoring 0 owns every row.
MUTANT_FAMILY = {"last_key_dropped": "spike", "pad_key_visible": "sunk"}


def mutants(p, only=None):
    """name -> the float64 result of a subtly wrong kernel (some are no-ops for a case: compare with
    the reference).  only: that one alone."""
    B, H, Hkv, D, S, mode = p["case"]
    q, k, v, add, scale, grp, vis, table = (p[n] for n in ("q", "k", "v", "add", "scale", "grp", "vis", "table"))
    ref = p["O"]
    ninf = -math.inf
    run = lambda **kw: attend(kw.get("q", q), kw.get("k", k), kw.get("v", v), kw.get("add", add), scale,  # noqa: E731
                              kw.get("grp", grp))[0]
    out = {}
    a = add.clone()
    a[..., S - 1] = ninf
    out["last_key_dropped"] = run(add=a)
    if only == "last_key_dropped":
        return {only: out[only]}
    # a pad key: zero K / V at index S, its term 0, visible to every row
    z1 = lambda t: torch.cat([t, torch.zeros_like(t[:, :1])], 1)  # noqa: E731
    ap = torch.cat([add, torch.zeros_like(add[..., :1])], -1)
    zp = scale * scores(q, z1(k), grp) + ap
    mp = zp.amax(-1, keepdim=True)
    wp = torch.exp(zp - mp)
    out["pad_key_visible"] = torch.einsum("bhij,bjhd->bihd", wp / wp.sum(-1, keepdim=True), _heads(z1(v), grp))
    if only == "pad_key_visible":
        return {only: out[only]}
    if is_causal(mode):
        i = torch.arange(S)
        out["causal_strict"] = run(add=add.masked_fill((i[None, :] >= i[:, None])[None, None], ninf))
    else:
        out["causal_strict"] = ref
    if vis is not None:
        ke = kend(vis)
        j = torch.arange(S)
        out["kend_minus_1"] = run(add=add.masked_fill((j[None, :] == ke[:, None] - 1)[:, None, None, :], ninf))
        up = (j[None, :] >= ke[:, None]) & (j[None, :] < (ke[:, None] + KT - 1) // KT * KT)  # pads up to the tile edge
        base = terms(p["case"], table, None)
        out["kend_roundup"] = run(add=torch.where(up[:, None, None, :], base, add))
    else:
        out["kend_minus_1"] = out["kend_roundup"] = ref
    if per_head(mode):
        out["bias_head_stride_0"] = run(add=terms(p["case"], table[:1], vis))
    else:
        out["bias_head_stride_0"] = ref
    out["v_next_head"] = run(v=v.roll(-1, 2)) if Hkv > 1 else ref
    if grp > 1:  # stored head h % grp (folded into range) instead of h // grp
        sel = torch.tensor([(h % grp) % Hkv for h in range(H)])
        out["gqa_head_mod"] = attend(q, k[:, :, sel], v[:, :, sel], add, scale, 1)[0]
    else:
        out["gqa_head_mod"] = ref
    # alpha not applied to o on the second tile: what tile 0 put into o keeps the old maximum's scale
    if S > KT:
        z = scale * scores(q, k, grp) + add
        tm = _tile_max(z)
        m0, m1 = tm[..., 0], torch.maximum(tm[..., 0], tm[..., 1])
        f = torch.where(torch.isfinite(m0), torch.exp(m1 - m0), torch.ones_like(m0))
        P = p_of(p)
        Pm = P.clone()
        Pm[..., :KT] = P[..., :KT] * f[..., None]
        out["alpha_skipped"] = torch.einsum("bhij,bjhd->bihd", Pm, _heads(v, grp))
    else:
        out["alpha_skipped"] = ref
    y = ref.clone()
    rows = list(range(KT - 1, S, KT)) or [S - 1]
    for r in rows:
        y[:, r] = ref[:, r - 1]
    out["tile_last_row_from_neighbour"] = y
    # one pair's first block never stored: the buffer still holds the same rows of another image
    y = ref.clone()
    y[0, :QB, H - 1] = ref[B - 1, :QB, H - 1]
    out["block_unwritten"] = y
    return out if only is None else {only: out[only]}


def p_of(p):
    return attend(p["q"], p["k"], p["v"], p["add"], p["scale"], p["grp"])[2]
