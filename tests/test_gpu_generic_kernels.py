"""Kernel-level tests of the planner's general path: every kernel of csrc/kernels/generic.hip, the
batched MatMul of bmm.hip, and the pooling arguments the older tests never pass.

Each case runs in bf16 mode and in fp32 (split) mode against a float64 reference evaluated on exactly
the values the kernel reads (bf16-rounded inputs, or join_planes(split_planes(x))), and is compared
per element:

* kernels that only move bits (copies, pads, selects, nearest resize, comparisons, the output casts):
  bit equality of the raw planes;
* arithmetic, bf16 mode:  |got - ref| <= 2^-8 |ref| + 1e-6 max|inputs|  (one bf16 rounding: half an
  ulp of 8 significant bits, which reaches 2^-8 |ref| just above a power of two; the floor covers an
  fp32-math error that flips the rounding);
* arithmetic, split mode: |got - ref| <= 2^-16 |ref| + 1e-6 max|inputs|  (representation error 2^-17,
  common.h, plus fp32 libm, with a 2x margin);
* GELU, split mode: 2^-16 |ref| + 2e-5 |ref| [v < -2] + 4e-7, the accuracy common.h documents;
* bmm_rows: 2^-8 |ref| + 1e-5 (|A| |B|)_ij in bf16 mode, 2^-15 (|A| |B|)_ij in split mode.

No output element is left out of any comparison."""
import math

import pytest

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

SPLITS = [False, True]
REL = {False: 2.0 ** -8, True: 2.0 ** -16}
SENTINEL = -77.0  # bf16-exact; fills every plane of an output before the launch


def _t():
    import torch

    return torch


def _K():
    from die_amd.ops import kernels as K

    return K


def _gen(seed):
    return _t().Generator().manual_seed(seed)


def _randn(g, *shape):
    return _t().randn(*shape, generator=g, dtype=_t().float64)


def _uniform(g, lo, hi, *shape):
    return _t().rand(*shape, generator=g, dtype=_t().float64) * (hi - lo) + lo


def _read(x, split):
    """float64 values -> (the tensor handed to the wrapper, the float64 values the kernel reads from it)."""
    torch, K = _t(), _K()
    x = x.cuda()
    if split:
        xin = x.float()
        return xin, K.join_planes(K.split_planes(xin)).double()
    xin = x.to(torch.bfloat16)
    return xin, xin.double()


def _raw(v, split):
    """Values -> the raw storage holding them (bf16, or the hi / lo planes), as the wrappers and the
    kernels make it.  A kernel that copies bits is compared with _raw of the tensor the wrapper got:
    re-splitting hi + lo can give another (hi, lo) pair for the same value."""
    torch, K = _t(), _K()
    return K.split_planes(v.float()) if split else v.to(torch.bfloat16)


def _vals(raw, split):
    return (_K().join_planes(raw) if split else raw).double()


def _filled(shape, split, value=SENTINEL):
    torch = _t()
    return torch.full(((2,) if split else ()) + tuple(shape), value, dtype=torch.bfloat16, device="cuda")


def _bits(t):
    return t.contiguous().view(_t().int16)


def _index(flat, shape):
    idx = []
    for n in reversed(shape):
        idx.append(flat % n)
        flat //= n
    return tuple(reversed(idx))


def assert_bits(case, got, want):
    """Bit equality of two raw tensors (so -0.0 != 0.0 and every NaN pattern counts)."""
    torch = _t()
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, "%s: shape %s != %s" % (case, tuple(g.shape), tuple(w.shape))
    if not torch.equal(g, w):
        bad = (g != w).reshape(-1)
        first = _index(int(bad.nonzero()[0]), tuple(g.shape))
        pytest.fail("%s: %d of %d elements differ, first at %s: got bits 0x%04x, want 0x%04x"
                    % (case, int(bad.sum()), bad.numel(), first, int(g[first]) & 0xFFFF, int(w[first]) & 0xFFFF))


def assert_same_f32(case, got, want):
    """Bit equality of two fp32 tensors."""
    torch = _t()
    assert got.dtype == torch.float32 and got.shape == want.shape, "%s: %s %s" % (case, got.dtype, tuple(got.shape))
    g, w = got.contiguous().view(torch.int32), want.contiguous().view(torch.int32)
    if not torch.equal(g, w):
        bad = (g != w).reshape(-1)
        first = _index(int(bad.nonzero()[0]), tuple(g.shape))
        pytest.fail("%s: %d of %d elements differ, first at %s: got %r, want %r"
                    % (case, int(bad.sum()), bad.numel(), first, float(got[first]), float(want[first])))


def assert_zero_bits(case, raw):
    assert_bits(case, raw, _t().zeros_like(raw))


def assert_close(case, got, ref, rel, floor, extra=None):
    """|got - ref| <= rel |ref| + floor (+ extra) at every element; NaN / inf in got fails."""
    torch = _t()
    got, ref = got.double(), ref.double()
    assert got.shape == ref.shape, "%s: shape %s != %s" % (case, tuple(got.shape), tuple(ref.shape))
    err = (got - ref).abs()
    bound = rel * ref.abs() + floor
    if extra is not None:
        bound = bound + extra
    over = ~(err <= bound)  # also NaN
    # the worst element: the largest error as a fraction of its bound (an exact result counts 0)
    frac = torch.where(over, torch.full_like(err, float("inf")), err / bound.clamp_min(1e-300))
    frac = torch.where(over & torch.isfinite(err) & (bound > 0), err / bound.clamp_min(1e-300), frac)
    where = _index(int(frac.reshape(-1).argmax()), tuple(got.shape))
    print("%s: worst element %s |err| %.3e = %.3f of its bound %.3e (got %r, ref %r)"
          % (case, where, float(err[where]), float(frac[where]), float(bound[where]), float(got[where]), float(ref[where])))
    if bool(over.any()):
        pytest.fail("%s: %d of %d elements over the bar, worst at %s: got %r, ref %r, |err| %.3e > bound %.3e"
                    % (case, int(over.sum()), over.numel(), where, float(got[where]), float(ref[where]),
                       float(err[where]), float(bound[where])))


# ---- unary_rows ---------------------------------------------------------------------------------------

def _f32(v):
    """A Python float as the kernel receives it (a float argument), back in double."""
    return float(_t().tensor(v, dtype=_t().float32))


# (code, a, b, name)
UNARY = [(0, 0, 0, "identity"), (1, 0, 0, "relu"), (2, 0, 0, "gelu"), (3, -1.0, 2.0, "clip"), (4, 0, 0, "sigmoid"),
         (5, 0, 0, "tanh"), (6, 0.125, 0, "leaky_relu"), (7, 0, 0, "exp"), (8, 0, 0, "abs"), (9, 0, 0, "sqrt"),
         (10, 0, 0, "neg"), (11, 0, 0, "reciprocal"), (12, 0, 0, "log"), (13, 0, 0, "erf"), (14, 0.5, 0, "pow0.5"),
         (14, 2.0, 0, "pow2"), (14, 1.0, 0, "pow1"), (14, 3.0, 0, "pow3"), (14, -1.5, 0, "pow-1.5"),
         (15, 0.2, 0.5, "hardsigmoid"), (16, 0, 0, "hardswish"), (17, 0, 0, "softplus"), (18, 0.5, 0, "gt_const"),
         (19, 0.5, 0, "lt_const"), (20, 0.5, 0, "eq_const"), (21, 0.5, 0, "ge_const"), (22, 0.5, 0, "le_const"),
         (23, 0, 0, "not"), (24, 0, 0, "to_bool")]


def _unary_targets(code, n, g):
    """The values the activation should see: per code, finite results and every edge of the code."""
    torch = _t()
    special = []
    if code in (9, 11, 12, 14):
        v = _uniform(g, 0.25, 4.0, n)
        special = [1.0, 0.25, 4.0]
    elif code in (2, 4, 7, 17):
        v = _uniform(g, -8.0, 8.0, n)
        special = {2: [-2.0, -2.5, -6.0, 0.0, 2.0], 4: [0.0, -8.0, 8.0], 7: [-8.0, 8.0, 0.0],
                   17: [-30.0, 19.5, 20.0, 20.5, 25.0]}[code]
    elif code == 3:  # Clip(-1, 2): on, just inside and just outside both knots
        v = _uniform(g, -3.0, 4.0, n)
        special = [-1.0, 2.0, -1.0078125, 2.015625, -0.9921875, 1.9921875]
    elif code == 5:
        v = _uniform(g, -4.0, 4.0, n)
        special = [0.0, 10.0, -10.0]
    elif code == 13:
        v = _uniform(g, -3.0, 3.0, n)
    elif code == 15:  # HardSigmoid(0.2, 0.5): knots at -2.5 and 2.5
        v = _uniform(g, -4.0, 4.0, n)
        special = [-2.5, 2.5, -2.515625, 2.515625, -2.484375, 2.484375, 0.0]
    elif code == 16:  # HardSwish: knots at -3 and 3
        v = _uniform(g, -5.0, 5.0, n)
        special = [-3.0, 3.0, 0.0, -3.015625, 3.015625, -2.984375, 2.984375]
    elif 18 <= code <= 22:  # comparisons with a = 0.5: a third of the elements exactly 0.5
        v = _uniform(g, -1.0, 2.0, n)
        v[::3] = 0.5
    elif code in (23, 24):  # 0, -0.0 and non-zero
        v = _uniform(g, -1.0, 1.0, n)
        v[0::3] = 0.0
        v[1::3] = -0.0
    else:  # identity, relu, leaky relu, abs, neg: both signs and zero
        v = _randn(g, n) * 2
        special = [0.0]
    if special:
        v[1:1 + len(special)] = torch.tensor(special, dtype=torch.float64)
    return v


def _unary_ref(code, v, a, b):
    torch = _t()
    one, zero = torch.ones_like(v), torch.zeros_like(v)
    if code == 1:
        return v.clamp_min(0)
    if code == 2:
        return 0.5 * v * torch.special.erfc(-v / math.sqrt(2.0))
    if code == 3:
        return v.clamp(a, b)
    if code == 4:
        return torch.sigmoid(v)
    if code == 5:
        return torch.tanh(v)
    if code == 6:
        return torch.where(v >= 0, v, v * a)
    if code == 7:
        return torch.exp(v)
    if code == 8:
        return v.abs()
    if code == 9:
        return torch.sqrt(v)
    if code == 10:
        return -v
    if code == 11:
        return 1.0 / v
    if code == 12:
        return torch.log(v)
    if code == 13:
        return torch.erf(v)
    if code == 14:
        return torch.pow(v, a)
    if code == 15:
        return (a * v + b).clamp(0, 1)
    if code == 16:
        return v * (v / 6.0 + 0.5).clamp(0, 1)
    if code == 17:
        return torch.log1p(torch.exp(v))
    if code == 18:
        return torch.where(v > a, one, zero)
    if code == 19:
        return torch.where(v < a, one, zero)
    if code == 20:
        return torch.where(v == a, one, zero)
    if code == 21:
        return torch.where(v >= a, one, zero)
    if code == 22:
        return torch.where(v <= a, one, zero)
    if code == 23:
        return torch.where(v == 0, one, zero)
    if code == 24:
        return torch.where(v != 0, one, zero)
    return v.clone()


def _gelu_extra(v, ref):
    return 2e-5 * ref.abs() * (v < -2).double() + 4e-7


def _unary_problem(code, R, C, Cl, affine, split, seed):
    """x (as the kernel reads it), scale, shift, and v = x * scale + shift in float64.  With an affine,
    scale is a power of two and shift a multiple of 1/4 per column, and x = (target - shift) / scale:
    the edge values (knots, the compared constant, zero) are then reproduced exactly by the fp32 affine."""
    torch = _t()
    g = _gen(seed)
    target = _unary_targets(code, R * C, g).reshape(R, C)
    if affine:
        s = torch.tensor([0.5, 1.0, 2.0, 4.0], dtype=torch.float64).repeat(C)[:C]
        h = torch.tensor([0.0, 0.25, -0.5, 0.75, -0.25, 0.5, -0.75], dtype=torch.float64).repeat(C)[:C]
        x = (target - h) / s
    else:
        s = h = None
        x = target
    x[:, Cl:] = 0.0  # stored pad columns hold 0
    xin, xv = _read(x, split)
    if affine:
        s, h = s.cuda(), h.cuda()
        v = xv * s + h
    else:
        v = xv
    return xin, xv, s, h, v


@pytest.mark.parametrize("split", SPLITS, ids=["bf16", "split"])
@pytest.mark.parametrize("code,a,b,name", UNARY, ids=[u[3] for u in UNARY])
def test_unary_rows(native, code, a, b, name, split):
    torch, K = _t(), _K()
    R, C = 37, 24
    for Cl in (24, 19):
        for affine in (False, True):
            case = "unary %s (code %d) Cl=%d affine=%s %s" % (name, code, Cl, affine, "split" if split else "bf16")
            xin, xv, s, h, v = _unary_problem(code, R, C, Cl, affine, split, 1000 + code)
            out = _filled((R, C), split)
            K.unary_rows(xin, code, a, b, scale=None if s is None else s.float(), shift=None if h is None else h.float(),
                         Cl=Cl, split=split, out=out)
            torch.cuda.synchronize()
            ref = _unary_ref(code, v[:, :Cl], _f32(a), _f32(b))
            assert torch.isfinite(ref).all(), case
            assert_zero_bits(case + " pad columns", out[..., Cl:])
            if code >= 18:  # results exactly 0 or 1
                assert_bits(case, out[..., :Cl], _raw(ref, split))
                continue
            got = _vals(out, split)[:, :Cl]
            floor = 1e-6 * float(xv.abs().max())
            if code == 2 and split:
                assert_close(case, got, ref, REL[True], 0.0, _gelu_extra(v[:, :Cl], ref))
            else:
                assert_close(case, got, ref, REL[split], floor)


# ---- binary_rows --------------------------------------------------------------------------------------

BINARY = ["add", "sub", "mul", "div", "max", "min", "gt", "lt", "eq", "ge", "le"]


def _binary_ref(op, x, y):
    torch = _t()
    one, zero = torch.ones_like(x), torch.zeros_like(x)
    fns = [lambda: x + y, lambda: x - y, lambda: x * y, lambda: x / y, lambda: torch.maximum(x, y),
           lambda: torch.minimum(x, y), lambda: torch.where(x > y, one, zero), lambda: torch.where(x < y, one, zero),
           lambda: torch.where(x == y, one, zero), lambda: torch.where(x >= y, one, zero),
           lambda: torch.where(x <= y, one, zero)]
    return fns[op]()


def _binary_problem(op, ymode, B, rps, C, Cl, split, seed):
    g = _gen(seed)
    R = B * rps
    x = _randn(g, R, C) * 2
    yshape = (B, C) if ymode else (R, C)
    y = _uniform(g, 0.5, 2.0, *yshape) if op == 3 else _randn(g, *yshape) * 2
    if op >= 6:  # equal pairs decide ==, >= and <=
        if ymode:
            y[:, ::3] = x[2::rps, ::3]
        else:
            y.view(-1)[::3] = x.view(-1)[::3]
    x[:, Cl:] = 0.0
    y[:, Cl:] = 0.0
    xin, xv = _read(x, split)
    yin, yv = _read(y, split)
    yb = yv.repeat_interleave(rps, dim=0) if ymode else yv
    return xin, yin, xv, yb


@pytest.mark.parametrize("split", SPLITS, ids=["bf16", "split"])
@pytest.mark.parametrize("ymode", [0, 1], ids=["same_shape", "row_per_sample"])
@pytest.mark.parametrize("op", range(11), ids=BINARY)
def test_binary_rows(native, op, ymode, split):
    torch, K = _t(), _K()
    B, rps, C = 3, 5, 16
    for Cl in (16, 13):
        xin, yin, xv, yb = _binary_problem(op, ymode, B, rps, C, Cl, split, 2000 + 16 * op + ymode)
        if ymode:  # every sample's broadcast row differs from the other samples'
            assert not torch.equal(yb[0, :Cl], yb[rps, :Cl]) and not torch.equal(yb[rps, :Cl], yb[2 * rps, :Cl])
        if op >= 6:
            assert int((xv[:, :Cl] == yb[:, :Cl]).sum()) >= Cl and int((xv[:, :Cl] != yb[:, :Cl]).sum()) >= Cl
        pre = _binary_ref(op, xv[:, :Cl], yb[:, :Cl])
        for act, a, b in ((0, 0.0, 0.0), (1, 0.0, 0.0), (3, -0.5, 0.75)):
            case = "binary %s ymode=%d Cl=%d act=%d %s" % (BINARY[op], ymode, Cl, act, "split" if split else "bf16")
            out = _filled((B * rps, C), split)
            K.binary_rows(xin, yin, op, ymode=ymode, rows_per_sample=rps, act=act, a=a, b=b, Cl=Cl, split=split, out=out)
            torch.cuda.synchronize()
            ref = _unary_ref(act, pre, a, b)
            assert torch.isfinite(ref).all(), case
            assert_zero_bits(case + " pad columns", out[..., Cl:])  # 0 / 0 of the pads must not come out as NaN
            if op >= 6:
                assert_bits(case, out[..., :Cl], _raw(ref, split))
            else:
                floor = 1e-6 * max(float(xv.abs().max()), float(yb.abs().max()))
                assert_close(case, _vals(out, split)[:, :Cl], ref, REL[split], floor)


# ---- where_rows ---------------------------------------------------------------------------------------

def _where_problem(R, C, Cl, split, seed):
    torch = _t()
    g = _gen(seed)
    cond = torch.tensor([0.0, -0.0, 1.0, 2.5, -3.0], dtype=torch.float64).repeat(R * C)[:R * C].reshape(R, C).clone()
    cond[:, Cl:] = 0.0
    a, b = _randn(g, R, C), _randn(g, R, C)
    a[:, Cl:] = 9.0  # the kernel writes 0 to the pad columns whatever its operands hold there
    b[:, Cl:] = 9.0
    return _read(cond, split), _read(a, split), _read(b, split)


def _where_ref(cv, p, q, Cl, split):
    torch = _t()
    ref = torch.where(cv != 0, p, q).float()
    ref[:, Cl:] = 0.0
    return _raw(ref, split)


@pytest.mark.parametrize("split", SPLITS, ids=["bf16", "split"])
@pytest.mark.parametrize("arms", ["tensor_tensor", "scalar_tensor", "tensor_scalar", "scalar_scalar"])
def test_where_rows(native, arms, split):
    torch, K = _t(), _K()
    R, C = 15, 16
    av, bv = 1.25, -0.3
    for Cl in (13, 16):
        case = "where %s Cl=%d %s" % (arms, Cl, "split" if split else "bf16")
        (cin, cv), (ain, avals), (bin_, bvals) = _where_problem(R, C, Cl, split, 3000)
        ta, tb = arms.split("_")
        # a scalar reaches the kernel as a float and is stored like any computed value
        p = avals.float() if ta == "tensor" else torch.full_like(cv, av).float()
        q = bvals.float() if tb == "tensor" else torch.full_like(cv, bv).float()
        out = _filled((R, C), split)
        K.where_rows(cin, ain if ta == "tensor" else av, bin_ if tb == "tensor" else bv, Cl=Cl, split=split, out=out)
        torch.cuda.synchronize()
        assert_bits(case, out, _where_ref(cv, p, q, Cl, split))


# ---- the live batch -----------------------------------------------------------------------------------
# Each problem launches into out(shape) and returns what the computed samples must hold: either
# {"raw": expected storage} (bit-exact kernels) or {"ref", "floor"[, "rel", "extra"]} (arithmetic ones).

def _live_unary(split, live, out):
    K = _K()
    xin, xv = _read(_randn(_gen(4000), 15, 16), split)
    K.unary_rows(xin, 5, live=live, rows_per_sample=5, split=split, out=out((15, 16)))
    return dict(ref=_t().tanh(xv), floor=1e-6 * float(xv.abs().max()))


def _live_binary(split, live, out):
    K = _K()
    g = _gen(4001)
    xin, xv = _read(_randn(g, 15, 16), split)
    yin, yv = _read(_randn(g, 3, 16), split)
    K.binary_rows(xin, yin, 0, ymode=1, rows_per_sample=5, live=live, split=split, out=out((15, 16)))
    return dict(ref=xv + yv.repeat_interleave(5, dim=0), floor=1e-6 * max(float(xv.abs().max()), float(yv.abs().max())))


def _live_where(split, live, out):
    K = _K()
    (cin, cv), (ain, av), (bin_, bv) = _where_problem(15, 16, 16, split, 4002)
    K.where_rows(cin, ain, bin_, live=live, rows_per_sample=5, split=split, out=out((15, 16)))
    return dict(raw=_where_ref(cv, av.float(), bv.float(), 16, split))


def _live_resize_nearest(split, live, out):
    import generic_refs as G

    K = _K()
    xin, xv = _read(_randn(_gen(4003), 3, 5, 7, 8), split)
    K.resize_nhwc(xin, 10, 14, 2.0, 2.0, coord=1, mode=0, nearest=2, live=live, split=split, out=out((3, 10, 14, 8)))
    return dict(raw=G.resize_nearest_ref(_raw(xin, split), 10, 14, 2.0, 2.0, 1, 2))


def _live_resize_linear(split, live, out):
    import generic_refs as G

    K = _K()
    xin, xv = _read(_randn(_gen(4004), 3, 5, 7, 8), split)
    K.resize_nhwc(xin, 10, 14, 2.0, 2.0, coord=0, mode=1, live=live, split=split, out=out((3, 10, 14, 8)))
    return dict(ref=G.resize_linear_ref(xv, 10, 14, 2.0, 2.0, 0), floor=1e-6 * float(xv.abs().max()))


def _live_bmm(split, live, out):
    torch, K = _t(), _K()
    g = _gen(4005)
    ain, av = _read(_randn(g, 3, 20, 16), split)
    bin_, bv = _read(_randn(g, 3, 12, 16), split)
    K.bmm_rows(ain, bin_, 10, 12, 16, live=live, split=split, out=out((3, 20, 16)))
    ref = torch.zeros(3, 20, 16, dtype=torch.float64, device="cuda")
    absprod = torch.zeros_like(ref)
    ref[:, :, :10] = av[:, :, :12] @ bv[:, :, :10]
    absprod[:, :, :10] = av[:, :, :12].abs() @ bv[:, :, :10].abs()
    if split:
        return dict(ref=ref, rel=0.0, floor=0.0, extra=2.0 ** -15 * absprod)
    return dict(ref=ref, rel=2.0 ** -8, floor=0.0, extra=1e-5 * absprod)


LIVE = {"unary_rows": _live_unary, "binary_rows": _live_binary, "where_rows": _live_where,
        "resize_nhwc_nearest": _live_resize_nearest, "resize_nhwc_linear": _live_resize_linear, "bmm_rows": _live_bmm}


@pytest.mark.parametrize("split", SPLITS, ids=["bf16", "split"])
@pytest.mark.parametrize("live", [0, 2, 3, 6])
@pytest.mark.parametrize("kernel", sorted(LIVE))
def test_live_batch_limits_the_work(native, kernel, live, split):
    """B = 3 samples: the first min(live, B) are computed, the rest of the output keeps its bits in
    every plane; live > B behaves as B."""
    torch = _t()
    B = 3
    case = "%s live=%d %s" % (kernel, live, "split" if split else "bf16")
    made = []

    def out(shape):
        made.append(_filled(shape, split))
        return made[0]

    want = LIVE[kernel](split, live, out)
    torch.cuda.synchronize()
    raw = made[0]
    axis = 1 if split else 0  # the sample (or row) axis of the raw storage
    per = raw.shape[axis] // B  # rows per sample for the row kernels, 1 for [B, ...] outputs
    n = min(live, B)

    def samples(t, lo, hi, ax):
        return t.narrow(ax, lo * per, (hi - lo) * per)

    rest = samples(raw, n, B, axis)
    assert_bits(case + " untouched samples", rest, torch.full_like(rest, SENTINEL))
    if n == 0:
        return
    if "raw" in want:
        assert_bits(case + " live samples", samples(raw, 0, n, axis), samples(want["raw"], 0, n, axis))
    else:
        extra = want.get("extra")
        assert_close(case + " live samples", samples(_vals(raw, split), 0, n, 0), samples(want["ref"], 0, n, 0),
                     want.get("rel", REL[split]), want["floor"], None if extra is None else samples(extra, 0, n, 0))


# ---- the grid-stride loop -----------------------------------------------------------------------------

@pytest.mark.parametrize("split", SPLITS, ids=["bf16", "split"])
def test_unary_rows_past_the_grid_cap(native, split):
    """R * C / 8 = 2,099,520 items > 8192 blocks x 256 threads: some threads take a second loop trip."""
    torch, K = _t(), _K()
    R, C = 32768 + 37, 512
    assert R * C // 8 > 8192 * 256
    g = torch.Generator(device="cuda").manual_seed(5000)
    xin, xv = _read(torch.randn(R, C, generator=g, device="cuda", dtype=torch.float32).double(), split)
    out = _filled((R, C), split)
    K.unary_rows(xin, 5, split=split, out=out)
    torch.cuda.synchronize()
    assert_close("unary tanh %dx%d %s" % (R, C, "split" if split else "bf16"), _vals(out, split), torch.tanh(xv),
                 REL[split], 1e-6 * float(xv.abs().max()))


@pytest.mark.parametrize("split", SPLITS, ids=["bf16", "split"])
def test_resize_linear_past_the_grid_cap(native, split):
    """2 x 130 x 130 x 64 = 2,163,200 items > 8192 x 256."""
    import generic_refs as G

    torch, K = _t(), _K()
    B, H, Ho, C = 2, 65, 130, 512
    assert B * Ho * Ho * C // 8 > 8192 * 256
    g = torch.Generator(device="cuda").manual_seed(5001)
    xin, xv = _read(torch.randn(B, H, H, C, generator=g, device="cuda", dtype=torch.float32).double(), split)
    out = _filled((B, Ho, Ho, C), split)
    K.resize_nhwc(xin, Ho, Ho, 2.0, 2.0, coord=0, mode=1, split=split, out=out)
    torch.cuda.synchronize()
    ref = G.resize_linear_ref(xv, Ho, Ho, 2.0, 2.0, 0)
    assert_close("resize linear 65->130 C=512 %s" % ("split" if split else "bf16"), _vals(out, split), ref, REL[split],
                 1e-6 * float(xv.abs().max()))


# ---- resize_nhwc --------------------------------------------------------------------------------------

def _resize_pairs():
    import generic_refs as G

    n = len(G.RESIZE_SIZES)
    return [(G.RESIZE_SIZES[i], G.RESIZE_SIZES[(i + 1) % n]) for i in range(n)]


def _pixels(B, H, W, C, split):
    """Distinct values per (sample, pixel) within every channel, exact in bf16: +-(pixel + 1) * 2^(c - 4),
    the sign telling the samples apart (split mode: times 1 + 2^-10, so the lo plane carries bits too)."""
    torch = _t()
    assert B == 2 and H * W < 128
    p = torch.arange(1, H * W + 1, dtype=torch.float64).reshape(1, H, W, 1)
    c = torch.pow(2.0, torch.arange(C, dtype=torch.float64) - 4).reshape(1, 1, 1, C)
    sign = torch.tensor([1.0, -1.0], dtype=torch.float64).reshape(2, 1, 1, 1)
    x = sign * p * c
    return x * (1 + 2.0 ** -10) if split else x


RESIZE_MODES = [(coord, 0, nearest) for coord in range(5) for nearest in range(4)] + [(coord, 1, 0) for coord in range(5)]


def _resize_id(m):
    import generic_refs as G

    return "%s-%s" % (G.COORDS[m[0]], "linear" if m[1] else G.NEAREST[m[2]])


@pytest.mark.parametrize("split", SPLITS, ids=["bf16", "split"])
@pytest.mark.parametrize("mode", RESIZE_MODES, ids=_resize_id)
def test_resize_nhwc(native, mode, split):
    """Every coordinate mode x nearest mode, and linear x every coordinate mode, on size pairs whose H
    and W scales differ.  The kernel gets the float32 scale; the reference uses the exact ratio in
    float64 (test_generic_refs.py: both pick the same pixel everywhere on these sizes)."""
    import generic_refs as G

    torch, K = _t(), _K()
    coord, linear, nearest = mode
    for (H, Ho), (W, Wo) in _resize_pairs():
        case = "resize %s H %d->%d W %d->%d %s" % (_resize_id(mode), H, Ho, W, Wo, "split" if split else "bf16")
        xin, xv = _read(_pixels(2, H, W, 8, split), split)
        out = _filled((2, Ho, Wo, 8), split)
        K.resize_nhwc(xin, Ho, Wo, G.resize_scale(H, Ho), G.resize_scale(W, Wo), coord=coord, mode=linear,
                      nearest=nearest, split=split, out=out)
        torch.cuda.synchronize()
        if linear:
            ref = G.resize_linear_ref(xv, Ho, Wo, Ho / H, Wo / W, coord)
            assert_close(case, _vals(out, split), ref, REL[split], 1e-6 * float(xv.abs().max()))
        else:
            assert_bits(case, out, G.resize_nearest_ref(_raw(xin, split), Ho, Wo, Ho / H, Wo / W, coord, nearest))


@pytest.mark.parametrize("split", SPLITS, ids=["bf16", "split"])
def test_resize_ties_separate_round_prefer_floor_from_ceil(native, split):
    """asymmetric x2 puts every odd output index on an exact .5 tie: there, and only there, the two
    rounding modes read different pixels (the last odd index clamps to the edge in both)."""
    torch, K = _t(), _K()
    xin, _ = _read(_pixels(2, 5, 7, 8, split), split)
    got = []
    for nearest in (0, 1):
        out = _filled((2, 10, 14, 8), split)
        K.resize_nhwc(xin, 10, 14, 2.0, 2.0, coord=1, mode=0, nearest=nearest, split=split, out=out)
        got.append(_vals(out, split))
    torch.cuda.synchronize()
    lo, hi = got
    assert torch.equal(lo[:, 0::2, 0::2], hi[:, 0::2, 0::2])
    assert (lo[:, 1:-1:2] != hi[:, 1:-1:2]).all() and (lo[:, :, 1:-1:2] != hi[:, :, 1:-1:2]).all()
    assert torch.equal(lo[:, -1, 0::2], hi[:, -1, 0::2]) and torch.equal(lo[:, 0::2, -1], hi[:, 0::2, -1])


# ---- pad_nhwc -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("split", SPLITS, ids=["bf16", "split"])
@pytest.mark.parametrize("sy,sx", [(1, 1), (2, 2), (2, 3)])
@pytest.mark.parametrize("t,l", [(0, 0), (1, 2), (3, 0)])
def test_pad_nhwc(native, t, l, sy, sx, split):
    import generic_refs as G

    torch, K = _t(), _K()
    B, H, W, C = 2, 3, 5, 16
    Ho, Wo = (H - 1) * sy + 1 + t + 2, (W - 1) * sx + 1 + l + 1  # slack below and to the right
    xin, xv = _read(_randn(_gen(6000), B, H, W, C), split)
    out = _filled((B, Ho, Wo, C), split)  # the sentinel shows any element the kernel does not write
    K.pad_nhwc(xin, Ho, Wo, t, l, sy=sy, sx=sx, split=split, out=out)
    torch.cuda.synchronize()
    assert_bits("pad t=%d l=%d sy=%d sx=%d %s" % (t, l, sy, sx, "split" if split else "bf16"), out,
                G.pad_insert_ref(_raw(xin, split), Ho, Wo, t, l, sy, sx))


# ---- copy_cols ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("split", SPLITS, ids=["bf16", "split"])
def test_copy_cols(native, split):
    """A column window out of a row slice of a taller tensor into a row slice of another: in split mode
    the plane distances are those of the parents, not R * ld."""
    torch, K = _t(), _K()
    R, ldx, colx, ldy, coly, ncols = 11, 40, 8, 56, 16, 24
    g = _gen(7000)
    lead = (2,) if split else ()
    xparent = _randn(g, *lead, R + 4, ldx).to(torch.bfloat16).cuda()
    yparent = _randn(g, *lead, R + 3, ldy).to(torch.bfloat16).cuda()
    before = yparent.clone()
    x, y = xparent[..., 2:2 + R, :], yparent[..., 1:1 + R, :]
    if split:
        assert x.stride(0) != R * ldx and y.stride(0) != R * ldy
    K.copy_cols(x, y, colx, coly, ncols, split=split)
    torch.cuda.synchronize()
    want = before.clone()
    want[..., 1:1 + R, coly:coly + ncols] = xparent[..., 2:2 + R, colx:colx + ncols]
    assert_bits("copy_cols %s" % ("split" if split else "bf16"), yparent, want)
    for bad in ((4, coly, ncols), (colx, 12, ncols), (colx, coly, 20)):  # refused before any launch
        with pytest.raises(native.NativeError):
            K.copy_cols(x, y, *bad, split=split)
    torch.cuda.synchronize()
    assert_bits("copy_cols after the refused launches", yparent, want)


# ---- rows_prep, input_prep_wide, rows_to_f32, nhwc_to_nchw_f32_strided --------------------------------

@pytest.mark.parametrize("split", SPLITS, ids=["bf16", "split"])
def test_rows_prep(native, split):
    torch, K = _t(), _K()
    R, F, Fp = 2 * 15, 13, 16
    x = _randn(_gen(8000), R, F).float().cuda()
    out = _filled((R, Fp), split)
    K.rows_prep(x, Fp, split=split, out=out)
    torch.cuda.synchronize()
    case = "rows_prep F=13 -> 16 %s" % ("split" if split else "bf16")
    assert_zero_bits(case + " pad columns", out[..., F:])
    assert_close(case, _vals(out, split)[:, :F], x.double(), REL[split], 1e-6 * float(x.abs().max()))


@pytest.mark.parametrize("split", SPLITS, ids=["bf16", "split"])
@pytest.mark.parametrize("affine", [False, True], ids=["plain", "affine"])
def test_input_prep_wide(native, affine, split):
    torch, K = _t(), _K()
    B, C, H, W, Cp = 2, 12, 3, 5, 16
    g = _gen(8001)
    x = _randn(g, B, C, H, W).float().cuda()
    s = (_uniform(g, 0.5, 2.0, C)).float().cuda() if affine else None
    h = _randn(g, C).float().cuda() if affine else None
    out = _filled((B, H, W, Cp), split)
    K.input_prep_wide(x, Cp, scale=s, shift=h, split=split, out=out)
    torch.cuda.synchronize()
    ref = x.double()
    if affine:
        ref = ref * s.double().view(1, C, 1, 1) + h.double().view(1, C, 1, 1)
    case = "input_prep_wide C=12 -> 16 affine=%s %s" % (affine, "split" if split else "bf16")
    assert_zero_bits(case + " pad channels", out[..., C:])
    floor = 1e-6 * max(float(x.abs().max()), float(ref.abs().max()))
    assert_close(case, _vals(out, split)[..., :C], ref.permute(0, 2, 3, 1), REL[split], floor)


def _stored(shape, logical, split, seed):
    """A stored tensor whose pad columns hold something: the output casts must drop them unread."""
    x = _randn(_gen(seed), *shape)
    x[..., logical:] = 5.0
    return _read(x, split)


@pytest.mark.parametrize("split", SPLITS, ids=["bf16", "split"])
def test_rows_to_f32(native, split):
    torch, K = _t(), _K()
    xin, xv = _stored((2 * 15, 16), 13, split, 8002)
    got = K.rows_to_f32(xin, 13, split=split)
    torch.cuda.synchronize()
    assert_same_f32("rows_to_f32 ld=16 -> 13 %s" % ("split" if split else "bf16"), got, xv[:, :13].float())


@pytest.mark.parametrize("split", SPLITS, ids=["bf16", "split"])
def test_nhwc_to_nchw_f32_strided(native, split):
    torch, K = _t(), _K()
    xin, xv = _stored((2, 3, 5, 16), 12, split, 8003)
    got = K.nhwc_to_nchw_f32_strided(xin, 12, split=split)
    torch.cuda.synchronize()
    assert_same_f32("nhwc_to_nchw_f32_strided Cs=16 -> 12 %s" % ("split" if split else "bf16"), got,
                    xv[..., :12].permute(0, 3, 1, 2).float())


def test_rows_prep_round_trip_in_split_mode(native):
    torch, K = _t(), _K()
    R, F, Fp = 2 * 15, 13, 16
    x = _randn(_gen(8004), R, F).float().cuda()
    stored = K.rows_prep(x, Fp, split=True)
    back = K.rows_to_f32(stored, F, split=True)
    torch.cuda.synchronize()
    assert_close("rows_prep -> rows_to_f32 (split)", back, x.double(), 2.0 ** -16, 0.0)


# ---- bmm_rows -----------------------------------------------------------------------------------------

BMM = [(1, 1, 1, 1, 8, 8, 8), (3, 64, 64, 32, 32, 64, 64), (2, 65, 70, 33, 40, 72, 72), (2, 50, 20, 50, 56, 24, 24),
       (1, 130, 129, 100, 104, 136, 200)]


@pytest.mark.parametrize("split", SPLITS, ids=["bf16", "split"])
@pytest.mark.parametrize("shape", BMM, ids=["x".join(map(str, s)) for s in BMM])
def test_bmm_rows(native, shape, split):
    """The pad columns of A ([K, lda)) and B ([N, ldb)) hold NaN: by the kernel's contract they do not matter."""
    torch, K_ = _t(), _K()
    batch, M, N, K, lda, ldb, ldc = shape
    g = _gen(9000 + M)
    A, Bm = _randn(g, batch, M, lda), _randn(g, batch, K, ldb)
    A[:, :, K:] = float("nan")
    Bm[:, :, N:] = float("nan")
    ain, av = _read(A, split)
    bin_, bv = _read(Bm, split)
    out = _filled((batch, M, ldc), split)
    K_.bmm_rows(ain, bin_, N, K, ldc, split=split, out=out)
    torch.cuda.synchronize()
    case = "bmm %s %s" % ("x".join(map(str, shape)), "split" if split else "bf16")
    a, b = av[:, :, :K], bv[:, :K, :N]
    ref, absprod = a @ b, a.abs() @ b.abs()
    assert_zero_bits(case + " output columns [N, ldc)", out[..., N:])
    got = _vals(out, split)[:, :, :N]
    assert torch.isfinite(got).all(), case
    if split:
        assert_close(case, got, ref, 0.0, 0.0, 2.0 ** -15 * absprod)
    else:
        assert_close(case, got, ref, 2.0 ** -8, 0.0, 1e-5 * absprod)


@pytest.mark.parametrize("split", SPLITS, ids=["bf16", "split"])
def test_bmm_rows_refuses_bad_pitches(native, split):
    torch, K = _t(), _K()
    out = _filled((1, 4, 8), split)
    ok = torch.ones(1, 4, 8, device="cuda", dtype=torch.float32 if split else torch.bfloat16)
    with pytest.raises(native.NativeError):  # lda < K
        K.bmm_rows(ok, torch.ones(1, 12, 8, device="cuda", dtype=ok.dtype), 8, 12, 8, split=split, out=out)
    with pytest.raises(native.NativeError):  # ldb % 8
        K.bmm_rows(ok, torch.ones(1, 8, 12, device="cuda", dtype=ok.dtype), 8, 8, 8, split=split, out=out)
    torch.cuda.synchronize()
    assert_bits("bmm refused: nothing launched", out, torch.full_like(out, SENTINEL))


# ---- pool2d and global_avgpool: the arguments the older tests never pass ------------------------------

POOL = [  # k, stride, pad, is_max, count_include_pad
    (3, 2, 1, False, True),
    ((3, 2), (2, 1), (1, 0), True, False),
    ((3, 2), (2, 1), (1, 0), False, False),
    ((3, 2), (2, 1), (1, 0), False, True),
]


def _pool_ref(xv, k, stride, pad, is_max, cip):
    import torch.nn.functional as F

    x = xv.permute(0, 3, 1, 2)
    y = F.max_pool2d(x, k, stride, pad) if is_max else F.avg_pool2d(x, k, stride, pad, count_include_pad=cip)
    return y.permute(0, 2, 3, 1)


@pytest.mark.parametrize("split", SPLITS, ids=["bf16", "split"])
@pytest.mark.parametrize("fused", [None, 0, 1], ids=["plain", "affine", "affine_relu"])
@pytest.mark.parametrize("cfg", POOL, ids=["avg3x3s2p1_cip", "max3x2", "avg3x2", "avg3x2_cip"])
def test_pool2d_windows_padding_count_and_fused_affine(native, cfg, fused, split):
    """The per-channel affine and the activation apply to the pooled value: y = act(pool(x) * scale + shift)."""
    torch, K = _t(), _K()
    k, stride, pad, is_max, cip = cfg
    g = _gen(10000)
    xin, xv = _read(_randn(g, 2, 9, 9, 16) - 0.5, split)  # mixed signs, mostly negative windows too
    s = h = None
    if fused is not None:
        s, h = _uniform(g, -1.5, 1.5, 16).float().cuda(), _randn(g, 16).float().cuda()
    got = K.pool2d_nhwc(xin, k, stride, pad, is_max=is_max, count_include_pad=cip, split=split, scale=s, shift=h,
                        act=fused or 0)
    torch.cuda.synchronize()
    ref = _pool_ref(xv, k, stride, pad, is_max, cip)
    if fused is not None:
        ref = ref * s.double() + h.double()
        if fused == 1:
            ref = ref.clamp_min(0)
    case = "pool2d k=%s s=%s p=%s max=%s cip=%s fused=%s %s" % (k, stride, pad, is_max, cip, fused,
                                                               "split" if split else "bf16")
    assert_close(case, got, ref, REL[split], 1e-6 * float(xv.abs().max()))


@pytest.mark.parametrize("split", SPLITS, ids=["bf16", "split"])
@pytest.mark.parametrize("affine", [False, True], ids=["plain", "affine_relu"])
@pytest.mark.parametrize("mode", [1, 2], ids=["sum", "max"])
def test_global_pool_sum_and_max(native, mode, affine, split):
    """Half the channels hold negative values only: a maximum that starts from 0 would be wrong there."""
    torch, K = _t(), _K()
    g = _gen(11000)
    x = _randn(g, 3, 7, 7, 24)
    x[..., ::2] -= 5.0
    xin, xv = _read(x, split)
    assert float(xv[..., ::2].max()) < 0
    s = h = None
    v = xv
    if affine:
        s, h = _uniform(g, -1.5, 1.5, 24).float().cuda(), _randn(g, 24).float().cuda()
        v = (xv * s.double() + h.double()).clamp_min(0)
    stored, f32 = K.global_avgpool_nhwc(xin, scale=s, shift=h, relu=affine, split=split, mode=mode)
    torch.cuda.synchronize()
    ref = v.sum(dim=(1, 2)) if mode == 1 else v.amax(dim=(1, 2))
    case = "global pool mode=%d affine=%s %s" % (mode, affine, "split" if split else "bf16")
    floor = 1e-6 * float(xv.abs().max())
    assert_close(case + " stored", stored, ref, REL[split], floor)
    assert_close(case + " fp32 output", f32, ref, REL[True], floor)
