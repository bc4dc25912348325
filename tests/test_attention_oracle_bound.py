"""The attention checker (attention_oracle.py) on the CPU: for every case, input family and precision a
float32 model of the kernel's arithmetic passes the element-wise bound, every subtly wrong kernel that
changes a case's result at all is caught, the input families have the structure they claim, and the
grid keeps the block-mapping properties the kernel's index arithmetic depends on.  Runs without a GPU;
test_gpu_attention_sharp.py applies the same check to the kernel."""
import math

import pytest
import torch

import attention_oracle as ao

PRECISIONS = pytest.mark.parametrize("split", [False, True], ids=["bf16", "fp32"])
CASE = pytest.mark.parametrize("case", ao.CASES, ids=ao.case_id)


@PRECISIONS
@CASE
def test_emulation_passes_the_bound(case, split):
    for family in ao.FAMILIES:
        p = ao.problem(case, family, split)
        assert tuple(p["O"].shape) == (case[0], case[4], case[1], case[3])
        assert torch.isfinite(p["T"]).all() and (p["T"] >= 0).all()
        worst = ao.check(ao.emulate(p), p["O"], p["T"], "%s %s" % (ao.case_id(case), family))
        assert worst < 1.0


@PRECISIONS
@CASE
def test_bound_catches_every_live_mutant(case, split):
    """Every mutant that changes the result is caught, each on the input family of ao.MUTANT_FAMILY."""
    p = ao.problem(case, "randn", split)
    live = []
    for name, y in ao.mutants(p).items():
        if torch.equal(y, p["O"]):
            continue  # a no-op for this case (causal_strict without the causal flag, ...)
        live.append(name)
        p2 = p
        if name in ao.MUTANT_FAMILY:
            p2 = ao.problem(case, ao.MUTANT_FAMILY[name], split)
            y = ao.mutants(p2, only=name)[name]
            assert not torch.equal(y, p2["O"])
        with pytest.raises(AssertionError, match="outside the bound"):
            ao.check(y, p2["O"], p2["T"], name)
    assert len(live) >= 4, live
    B, H, Hkv, D, S, mode = case
    if S % ao.KT:
        assert "last_key_dropped" in live and "pad_key_visible" in live
    assert "block_unwritten" in live and "tile_last_row_from_neighbour" in live
    assert ("causal_strict" in live) == ao.is_causal(mode)
    assert ("kend_minus_1" in live) == ao.is_keymask(mode)
    assert ("bias_head_stride_0" in live) == ao.per_head(mode)
    assert ("gqa_head_mod" in live) == (Hkv != H and Hkv > 1)  # one stored head: every rule reads it
    assert ("alpha_skipped" in live) == (S > ao.KT)
    assert ("v_next_head" in live) == (Hkv > 1)


def test_mutant_names():
    p = ao.problem(ao.CASES[0], "randn", False)
    assert set(ao.mutants(p)) == {"last_key_dropped", "pad_key_visible", "causal_strict", "kend_minus_1", "kend_roundup",
                                  "bias_head_stride_0", "v_next_head", "gqa_head_mod", "alpha_skipped",
                                  "tile_last_row_from_neighbour", "block_unwritten"}
    assert any("kend_roundup" in _live(c) for c in ao.CASES if ao.is_keymask(c[5]))


def _live(case):
    p = ao.problem(case, "randn", False)
    return [n for n, y in ao.mutants(p).items() if not torch.equal(y, p["O"])]


# ---- the input families ---------------------------------------------------------------------------------

def _z(p):
    return p["scale"] * ao.scores(p["q"], p["k"], p["grp"]) + p["add"]


@CASE
def test_spike_family(case):
    """Every query with two visible keys has one dominant key, >= 8 natural units over the rest, and
    every special key (first / last of a tile, last of the partial tile) some row sees is one."""
    B, H, Hkv, D, S, mode = case
    for split in (False, True):
        p = ao.problem(case, "spike", split)
        z = _z(p)
        top = z.topk(2, -1).values
        two = torch.isfinite(top[..., 1])
        assert bool(two.any()) and float((top[..., 0] - top[..., 1])[two].min()) >= 8.0
        dom = z.argmax(-1)
        assert torch.equal(dom[two], ao.dominant_keys(case, p["add"])[two])
        seen = torch.isfinite(p["add"])
        for b in range(B):
            for h in range(H):
                keys = set(dom[b, h][torch.isfinite(top[b, h, :, 0])].tolist())
                for j in ao.special_keys(S):
                    if bool(seen[b, h, j, j]):
                        assert j in keys, (b, h, j)
                if not ao.is_causal(mode) and mode not in ("bias_shared", "bias_per_head"):
                    # the same keys for every row: the dominant keys cover all of them
                    assert keys == set(torch.nonzero(seen[b, h, 0]).flatten().tolist()), (b, h)
        # V rows are distinct: a wrong key is an O(1) error
        v = p["v"]
        assert float((v[:, 1:] - v[:, :-1]).abs().amax(-1).min()) > 0.5


@CASE
def test_rising_family(case):
    """Every tile whose last keys a row sees raises that row's maximum by >= 20 exp2 units."""
    for split in (False, True):
        p = ao.problem(case, "rising", split)
        tm = ao._tile_max(_z(p)) / ao.LN2
        tail = ao.tile_tail_visible(p["add"])
        n = 0
        for t in range(1, tm.shape[-1]):
            both = tail[..., t] & torch.isfinite(tm[..., t - 1])
            if bool(both.any()):
                n += int(both.sum())
                assert float((tm[..., t] - tm[..., :t].amax(-1))[both].min()) >= 20.0, t
        assert n > 0 or case[4] < 2 * ao.KT - 4


@CASE
def test_cliff_family(case):
    """Rows that see tile 0 have their maximum there, every later key >= 150 exp2 units below: p = 0."""
    for split in (False, True):
        p = ao.problem(case, "cliff", split)
        tm = ao._tile_max(_z(p)) / ao.LN2
        if tm.shape[-1] < 2:
            continue
        later = tm[..., 1:].amax(-1)
        both = torch.isfinite(tm[..., 0]) & torch.isfinite(later)
        assert bool(both.any())
        assert float((tm[..., 0] - later)[both].min()) >= 150.0


@CASE
def test_sunk_family(case):
    """Every visible score is <= -12 natural units: a key scoring 0 would take the whole row."""
    for split in (False, True):
        z = _z(ao.problem(case, "sunk", split))
        assert float(z[torch.isfinite(z)].max()) <= -12.0


# ---- the grid -------------------------------------------------------------------------------------------

def _cases(**kw):
    names = ("B", "H", "Hkv", "D", "S", "mode")
    return [c for c in ao.CASES if all(c[names.index(k)] == v for k, v in kw.items())]


def _mapped(case):
    nqb, gy, gz = ao.launch_grid(case)
    return (gy * gz) % 8 == 0


def test_grid_tile_edges_head_dims_and_modes():
    cs = ao.CASES
    assert len(set(cs)) == len(cs)
    for c in cs:
        B, H, Hkv, D, S, mode = c
        assert mode in ao.MODES and H % Hkv == 0 and D in (32, 64, 80, 96, 128)
        assert B * S * H * D <= 3.2e6
        if Hkv != H:
            assert D in (64, 128) and mode in ("none", "causal", "keymask", "keymask_holes")
    for S in (17, 33, 64, 65, 129, 300):
        assert any(not _mapped(c) for c in _cases(D=64, S=S, Hkv=3)), S
    assert {c[5] for c in _cases(D=64, S=129) if not _mapped(c) and c[1] == c[2]} == set(ao.MODES)
    for D in (32, 80, 96, 128):
        assert _cases(D=D, S=129), D
    assert {"none", "keymask"} <= {c[5] for c in _cases(D=80)}


def test_grid_runs_the_xcd_map_in_every_mode():
    for mode in ao.MODES:
        hit = [c for c in _cases(mode=mode) if c[1] == c[2] and _mapped(c) and ao.launch_grid(c)[0] >= 2]
        assert hit, mode
        for c in hit:
            for xm in (1, 2):
                want = sorted((x, y, z) for z in range(ao.launch_grid(c)[2]) for y in range(ao.launch_grid(c)[1])
                              for x in range(ao.launch_grid(c)[0]))
                blocks = ao.block_map(c, xm)
                assert sorted(t for _, t, _ in blocks) == want  # a bijection of the blocks
                assert any(src != dst for src, dst, _ in blocks)
    assert {ao.launch_grid(c)[0] for c in ao.CASES if c[1] == c[2] and _mapped(c)} >= {2, 3}
    gqa = [c for c in ao.CASES if c[1] != c[2] and _mapped(c)]
    assert {c[5] for c in gqa} >= {"none", "causal", "keymask"}
    assert {c[1] // c[2] for c in gqa} >= {2, 4} and any(c[1] != c[2] and not _mapped(c) for c in ao.CASES)


def test_grid_reaches_the_causal_rotation():
    for mode in ("causal", "causal_bias"):
        hit = []
        for c in _cases(mode=mode):
            nqb, gy, gz = ao.launch_grid(c)
            if _mapped(c) and nqb == 2 and gy * gz * nqb // 8 > 32 and any(rot for _, _, rot in ao.block_map(c)):
                hit.append(c)
        assert hit, mode
        if mode == "causal_bias":
            assert all(ao.per_head(c[5]) and c[1] > 1 for c in hit)
            p = ao.problem(hit[0], "randn", False)
            assert p["table"].shape[0] == hit[0][1] and not torch.equal(p["table"][0], p["table"][1])


def test_grid_key_masks_under_the_map():
    """Per-sample kend with an all-pad sample, tile-edge samples and (in the holes modes) a sample with
    holes, each at a batch index some block reaches only through the map."""
    for mode in ("keymask", "keymask_holes", "keymask_bias"):
        hit = [c for c in _cases(mode=mode) if _mapped(c) and c[1] == c[2] and ao.launch_grid(c)[0] >= 2]
        assert hit, mode
        for c in hit:
            vis = ao.visible(c)
            ke = ao.kend(vis).tolist()
            assert len(set(ke)) >= 4 and 0 in ke and 32 in ke and 64 in ke and c[4] in ke
            moved = {dst[2] for src, dst, _ in ao.block_map(c) if src[2] != dst[2]}
            holes = [b for b in range(c[0]) if int(vis[b].sum()) != ke[b]]
            assert bool(holes) == (mode != "keymask")
            for b in [ke.index(0), ke.index(32), ke.index(64)] + holes:
                assert b in moved, (c, b)
    assert any(_mapped(c) and ao.is_keymask(c[5]) for c in ao.CASES if c[1] != c[2])


# ---- check() and bound() --------------------------------------------------------------------------------

def test_check_reports_count_and_worst_index():
    ref = torch.zeros(2, 3, 4, 5, dtype=torch.float64)
    T = torch.full_like(ref, 1e-3)
    got = ref.clone()
    got[1, 2, 0, 3] = 0.5
    got[0, 1, 1, 1] = 2e-3
    with pytest.raises(AssertionError, match=r"2 of 120 elements outside the bound; worst \(b, s, h, d\) = \(1, 2, 0, 3\)"):
        ao.check(got, ref, T, "x")
    got[0, 0, 0, 0] = float("nan")
    with pytest.raises(AssertionError, match="3 of 120"):
        ao.check(got, ref, T, "x")
    assert ao.check(ref + 5e-4, ref, T) == pytest.approx(0.5)
    # T = 0 (an all-pad sample's rows): only the exact value passes
    assert ao.check(ref, ref, torch.zeros_like(ref)) == 0.0
    with pytest.raises(AssertionError, match="outside the bound"):
        ao.check(ref + 1e-30, ref, torch.zeros_like(ref))
    import inspect

    assert list(inspect.signature(ao.check).parameters) == ["got", "ref", "T", "what"]  # no way to exempt an element


def test_bound_terms():
    """Every term widens the bound.  The model itself needs P rounding and storage (bf16) and the exponent
    term (fp32 mode); lo_lo and accum are smaller than the exponent term's worst-case slack, so no correct
    model can show them: they stand on their derivation."""
    case = (4, 2, 2, 64, 300, "none")
    assert case in ao.CASES
    for split in (False, True):
        p = ao.problem(case, "randn", split)
        full = p["T"]
        for t in ao.TERMS:
            less = ao.bound_of(p, without=(t,))
            assert bool((less <= full).all())
            assert bool((less < full).any()) == (split or t != "lo_lo"), t
        u = 2.0 ** -16 if split else 2.0 ** -8
        assert bool((full >= u * (p["A"] + p["O"].abs())).all())  # never below P rounding + storage
        assert float((full / (p["A"] + p["O"].abs())).max()) < (2.0 ** -8 if split else 1.5 * u)
    # bf16: without the P rounding term the model (which rounds P) is outside
    p = ao.problem(case, "randn", False)
    with pytest.raises(AssertionError, match="outside the bound"):
        ao.check(ao.emulate(p), p["O"], ao.bound_of(p, without=("p_round",)))
    # bf16: rows with one key in sight (A = |O|) round the stored output by up to 2^-8 |O| on top of P's rounding
    p = ao.problem((4, 2, 2, 64, 129, "causal_bias"), "cliff", False)
    with pytest.raises(AssertionError, match="outside the bound"):
        ao.check(ao.emulate(p), p["O"], ao.bound_of(p, without=("storage",)))
    # fp32 mode: without the exponent term (the dropped K_lo Q_lo) the model is outside on `rising` scores
    p = ao.problem(case, "rising", True)
    with pytest.raises(AssertionError, match="outside the bound"):
        ao.check(ao.emulate(p), p["O"], ao.bound_of(p, without=("exponent",)))
    assert math.isclose(ao.U, 2.0 ** -24)
