"""The conv geometry checker (conv_geometry.py) on the CPU: for every case of the grid a correct fp32
conv passes the element-wise bound with room to spare, and every subtly wrong kernel that changes the
case's result at all is caught.  Runs without a GPU; the GPU tests apply the same check to the kernels."""
import pytest
import torch
import torch.nn.functional as F

import conv_geometry as cg


def _fp32_conv(p, case):
    """torch's fp32 CPU conv on the pre-rounded operands, standing in for the kernel."""
    s, (t, l, b, r), d = case[7], case[8], case[9]
    y = F.conv2d(F.pad(p["x"].float(), (l, r, t, b)), p["w"].float(), p["bias"].float(), stride=s, dilation=d)
    return y.permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("split", [False, True], ids=["bf16", "fp32"])
@pytest.mark.parametrize("case", cg.CASES, ids=cg.case_id)
def test_bound_passes_fp32_conv_and_catches_mutants(case, split):
    p = cg.problem(case, split)
    ref, S = p["ref"], p["S"]
    assert tuple(ref.shape) == (case[0],) + cg.out_hw(case) + (case[4],)
    T = cg.bound(case, 1, split) * S
    worst = cg.check(_fp32_conv(p, case), ref, T, "fp32 CPU conv")
    assert worst < 0.1, worst  # a correct fp32 conv sits far inside the bound
    # the model of the kernel's indexing is the reference when its fields are right
    assert torch.equal(cg.kernel_model(p["x"], p["w"], p["bias"], case), ref)
    live = []
    for name, y in cg.mutants(p["x"], p["w"], p["bias"], case).items():
        if torch.equal(y, ref):
            continue  # a no-op for this case (flipx on a 7x1 kernel, no_dil at dil 1, ...)
        live.append(name)
        with pytest.raises(AssertionError, match="outside the bound"):
            cg.check(y, ref, T, name)
    assert len(live) >= 4, live
    assert "one_tap" in live  # the sharpest one: a single missing product


def test_grid_covers_the_geometry_axes():
    """The grid keeps the properties the kernels index with (a reminder for whoever edits CASES)."""
    cs = cg.CASES
    assert len(cs) == 13 and len(set(cs)) == 13
    assert all(c[1] != c[2] for c in cs), "every image is non-square"
    assert any(c[5] != c[6] for c in cs) and any(c[9] > 1 for c in cs) and any(c[7] > 1 and c[9] > 1 for c in cs)
    assert any(c[8][0] != c[8][1] for c in cs), "pad_h != pad_w"
    assert any((c[8][0], c[8][1]) != (c[8][2], c[8][3]) for c in cs), "begin pads != end pads"


def test_check_reports_count_and_worst_index():
    ref = torch.zeros(2, 3, 4, 5, dtype=torch.float64)
    T = torch.full_like(ref, 1e-3)
    got = ref.clone()
    got[1, 2, 0, 3] = 0.5
    got[0, 1, 1, 1] = 2e-3
    with pytest.raises(AssertionError, match=r"2 of 120 elements .* worst \(b, oh, ow, n\) = \(1, 2, 0, 3\)"):
        cg.check(got, ref, T, "x")
    got[0, 0, 0, 0] = float("nan")
    with pytest.raises(AssertionError, match="3 of 120"):
        cg.check(got, ref, T, "x")
    assert cg.check(ref + 5e-4, ref, T) == pytest.approx(0.5)


@pytest.mark.parametrize("pad", [0, 1, 3])
def test_conv_problem_int_pad_is_four_equal_pads(native, pad):
    """ops.kernels.ConvProblem: an int pad gives the geometry it always gave, the 4-tuple of it the same,
    and uneven pads put the begin pads into pad_h / pad_w and the end pads only into Ho / Wo."""
    from die_amd.ops import kernels as K

    x = torch.zeros(2, 9, 13, 8, dtype=torch.bfloat16)
    w = torch.zeros(16, 8, 3, 5)

    def geom(p, **kw):
        g = dict(K.ConvProblem(x, w, pad=p, **kw).geom)
        g.pop("zeros")
        return g

    g = geom(pad, stride=2, dil=2)
    assert g == dict(B=2, H=9, W=13, Cin=8, Ho=(9 + 2 * pad - 4 - 1) // 2 + 1, Wo=(13 + 2 * pad - 8 - 1) // 2 + 1, N=16,
                     KH=3, KW=5, stride=2, pad_h=pad, pad_w=pad, dil=2, K=120, Kpad=128, relu=0, relu2=0)
    assert geom((pad,) * 4, stride=2, dil=2) == g
    u = geom((2, 1, 0, 3))
    assert (u["pad_h"], u["pad_w"], u["Ho"], u["Wo"]) == (2, 1, 9 + 2 - 2, 13 + 4 - 4)
    with pytest.raises(ValueError):
        K.ConvProblem(x, w, pad=(1, 2))
