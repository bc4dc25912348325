"""torch-facing wrappers around the hand-written gfx950 kernels (csrc/kernels/*.hip).

Used by the GPU numerics tests: each wrapper takes torch tensors on `cuda`, launches the native
kernel on torch's current stream through the C ABI (`capi_kernels.cpp`), and returns torch tensors.
They fail loudly (NativeError) when the native library is missing; there is no eager fallback.
"""
from __future__ import annotations

import json
from typing import Optional

import numpy as np

from .. import native


def _ptr(t) -> int:
    return 0 if t is None else int(t.data_ptr())


def _stream() -> int:
    import torch

    return int(torch.cuda.current_stream().cuda_stream)


def _check(rc: int, what: str):
    if rc != 0:
        raise native.NativeError("%s launch failed (hipError %d)" % (what, rc))


def bf16_bits(t):
    """bf16 tensor -> int16 view (the kernels take raw uint16 storage)."""
    import torch

    return t.contiguous().view(torch.int16)


def split_planes(t):
    """fp32 tensor -> its split form (csrc/kernels/common.h): [2, *shape] bf16, plane 0 = hi = bf16(t),
    plane 1 = lo = bf16(t - hi) (both round to nearest even, like the device)."""
    import torch

    t = t.float()
    hi = t.to(torch.bfloat16)
    lo = (t - hi.float()).to(torch.bfloat16)
    return torch.stack([hi, lo]).contiguous()


def join_planes(p):
    """[2, ...] split planes -> fp32 (hi + lo)."""
    return p[0].float() + p[1].float()


def pack_conv_weight(w, cin_store: Optional[int] = None, npad: int = 128, split: bool = False):
    """[Cout, Cin, KH, KW] float -> [Npad][Kpad] bf16 with k = (ky*KW + kx)*Cin_store + ci.
    split: [2][Npad][Kpad] (hi plane, then lo plane)."""
    import torch

    cout, cin, kh, kw = w.shape
    cs = cin_store or cin
    K = kh * kw * cs
    Kpad = (K + 63) // 64 * 64
    Np = (cout + npad - 1) // npad * npad
    wp = torch.zeros((Np, kh, kw, cs), dtype=torch.float32, device=w.device)
    wp[:cout, :, :, :cin] = w.permute(0, 2, 3, 1).float()
    wp = wp.reshape(Np, K)
    full = torch.zeros((Np, Kpad), dtype=torch.float32, device=w.device)
    full[:, :K] = wp
    out = split_planes(full) if split else full.to(torch.bfloat16)
    return out, K, Kpad


# launch configs of the conv kernel: tile + 4 * variant (kernels.h TileCfg)
NUM_CFGS = 40  # kernels.h TileCfg (variant 7 = the 8-wave wide tile, cfg 28 only; variant 8 = skinny rows, cfg 32 only;
#               variant 9 = the four-tile 3x3 kernel, cfg 39 only)


def _pads4(pad):
    """int -> the same pad on all four sides; (top, left, bottom, right) -> itself, as ints."""
    if isinstance(pad, (tuple, list)):
        if len(pad) != 4:
            raise ValueError("pad must be an int or (top, left, bottom, right), got %r" % (pad,))
        return tuple(int(v) for v in pad)
    return (int(pad),) * 4


class ConvProblem:
    """One implicit-GEMM conv problem with packed weights and preallocated outputs, re-launchable with
    any (config, split-K, fused) choice -- used by conv2d_nhwc and by tools/conv_bench.py.
    x_nhwc: [B,H,W,Cin] bf16 (split: any float dtype, converted to hi/lo planes), w: [Cout,Cin,KH,KW]
    float.  pad: one int for all four sides, or (top, left, bottom, right) -- the kernels offset by
    top / left and bound-check the input, the bottom / right pads only enter Ho / Wo.
    split = fp32 mode: x/res/out/out2 are split planes and the weights are packed hi + lo."""

    def __init__(self, x_nhwc, w, bias=None, stride=1, pad=0, dil=1, relu=False, res=None, out_f32=False,
                 scale2=None, shift2=None, relu2=False, max_splits=16, split=False):
        import torch

        B, H, W, Cs = x_nhwc.shape
        cout, cin, kh, kw = w.shape
        self.split = split
        self.wp, K, Kpad = pack_conv_weight(w, Cs, split=split)
        pt, pl, pb, pr = _pads4(pad)
        Ho = (H + pt + pb - dil * (kh - 1) - 1) // stride + 1
        Wo = (W + pl + pr - dil * (kw - 1) - 1) // stride + 1
        dev = x_nhwc.device

        def padded(v):
            if v is None:
                return None
            n = (v.numel() + 127) // 128 * 128
            o = torch.zeros(n, dtype=torch.float32, device=dev)
            o[: v.numel()] = v.float()
            return o

        np_ = (2,) if split else ()
        self.x = split_planes(x_nhwc) if split else x_nhwc.contiguous()
        self.res = None if res is None else (split_planes(res.reshape(B, Ho, Wo, cout)) if split else res.contiguous())
        self.bias_p, self.s2_p, self.b2_p = padded(bias), padded(scale2), padded(shift2)
        self.out_f32 = out_f32
        self.out = (torch.empty((B, Ho, Wo, cout), dtype=torch.float32, device=dev) if out_f32 else
                    torch.empty(np_ + (B, Ho, Wo, cout), dtype=torch.bfloat16, device=dev))
        self.out2 = (torch.empty(np_ + (B, Ho, Wo, cout), dtype=torch.bfloat16, device=dev)
                     if scale2 is not None else None)
        self.geom = dict(B=B, H=H, W=W, Cin=Cs, Ho=Ho, Wo=Wo, N=cout, KH=kh, KW=kw, stride=stride, pad_h=pt,
                         pad_w=pl, dil=dil, K=K, Kpad=Kpad, relu=int(relu), relu2=int(relu2))
        if split:
            self.geom.update(split=1, wplane=int(self.wp[0].numel()))
        self.zeros = torch.zeros(Kpad + 64, dtype=torch.int16, device=dev)  # zero page >= Kpad + 64
        self.geom["zeros"] = int(self.zeros.data_ptr())
        self.ws = torch.empty(max(1, max_splits) * B * Ho * Wo * cout if max_splits > 1 else 1, dtype=torch.float32,
                              device=dev)
        # fused split-K: the last split block of a tile reduces in-kernel (counters start at zero and
        # are reset by that block)
        self.counters = torch.zeros(65536, dtype=torch.int32, device=dev)
        self.flops = 2.0 * B * Ho * Wo * cout * cin * kh * kw
        self._L = native.kernels()

    def launch(self, tile=-1, splits=1, fused_splitk=True, order=0, extra=None, sk=0) -> int:
        """Launch on torch's current stream; returns the hipError code (1 = config not applicable).
        order: XCD tile order (ConvArgs::order: 0 heuristic, 1 N-fastest, 2 M-fastest).
        extra: more ConvArgs fields by geometry-JSON key (device pointers as ints), e.g. the LayerNorm
        statistics row_stats / col_sum / row_parts / stats_out and ln_eps.
        sk > 0: a stream-K launch of sk blocks (ConvArgs::sk; in-kernel reduction, splits ignored)."""
        g = dict(self.geom, splits=int(splits), order=int(order))
        g.update(extra or {})
        if sk > 0:
            bm, bn = [(128, 128), (128, 64), (64, 128), (64, 64)][tile % 4] if tile >= 0 else (64, 64)
            if self.ws.numel() < sk * 2 * bm * bn:
                return 1  # workspace too small for this P: not applicable
            g["sk"] = int(sk)
            g["ws"] = int(self.ws.data_ptr())
            g["counters"] = int(self.counters.data_ptr())
            g["counters_n"] = int(self.counters.numel())
        elif splits > 1:
            g["ws"] = int(self.ws.data_ptr())
            if fused_splitk:
                g["counters"] = int(self.counters.data_ptr())
                g["counters_n"] = int(self.counters.numel())
        return self._L.die_kern_conv(json.dumps(g).encode(), _ptr(self.x), _ptr(self.wp), _ptr(self.bias_p),
                                     _ptr(self.res), 0 if self.out_f32 else _ptr(self.out),
                                     _ptr(self.out) if self.out_f32 else 0, _ptr(self.s2_p), _ptr(self.b2_p),
                                     _ptr(self.out2), tile, _stream())

    def results(self):
        """(out, out2); split planes joined to fp32."""
        if not self.split:
            return self.out, self.out2
        out = self.out if self.out_f32 else join_planes(self.out)
        return out, None if self.out2 is None else join_planes(self.out2)


def conv2d_nhwc(x_nhwc, w, bias=None, stride=1, pad=0, dil=1, relu=False, res=None, out_f32=False,
                scale2=None, shift2=None, relu2=False, tile=-1, splits=1, fused_splitk=True, split=False):
    """Implicit-GEMM conv.  x_nhwc: [B,H,W,Cin] bf16, w: [Cout,Cin,KH,KW] float; pad as ConvProblem takes it.
    Returns (out, out2) in NHWC ([B,Ho,Wo,Cout]); out is f32 if out_f32 else bf16.
    split (fp32 mode): x/res any float dtype; outputs are the fp32 values of the split planes."""
    pr = ConvProblem(x_nhwc, w, bias, stride, pad, dil, relu, res, out_f32, scale2, shift2, relu2, max_splits=splits,
                     split=split)
    rc = pr.launch(tile, splits, fused_splitk)
    if rc != 0 and tile >= 0 and rc == 1:  # hipErrorInvalidValue: config not applicable to this shape
        return None, None
    _check(rc, "conv_igemm")
    return pr.results()


def pair_permute(n_rows: int):
    """Row permutation of conv_pair weights (kernels.h pair_permute_row): physical row of logical n."""
    perm = []
    for n in range(n_rows):
        b, r = n & ~31, n & 31
        g, h, t = r >> 3, (r >> 2) & 1, r & 3
        perm.append(b + 16 * h + 4 * g + t)
    return perm


def _pack_pair_weight(w, split):
    """[N, K] float -> rows permuted by pair_permute, N padded to 128, bf16 or split planes."""
    import torch

    n, k = w.shape
    npad = (n + 127) // 128 * 128
    full = torch.zeros((npad, k), dtype=torch.float32, device=w.device)
    perm = torch.tensor(pair_permute(n), device=w.device)
    full[perm] = w.float()
    return split_planes(full) if split else full.to(torch.bfloat16)


def conv_pair(y, w1, b1, res, s2, h2, w2, b2, relu=True, relu2=True, split=False, store_x=True, store_a=False,
              shared_w=-1):
    """Fused expand + next-reduce 1x1 pair (kernels/conv_pair.hip) over rows.
    y [M, K1], w1 [N1, K1], b1 [N1], res [M, N1], s2/h2 [N1], w2 [N2, N1], b2 [N2] (float).
    Returns (x, out): x = y @ w1.T + b1 + res  [M, N1] (None unless store_x) and
    out = act(act2(x * s2 + h2) @ w2.T + b2)  [M, N2], as fp32 (split planes joined) or bf16;
    store_a: also the stored pre-activation a = act2(x * s2 + h2) [M, N1] (PairArgs::aout), as a
    third element.  shared_w: PairArgs::shared_w (-1 auto, 0 separate W1 / W2 buffers, 1 one shared buffer)."""
    import torch

    M, K1 = y.shape
    N1, N2 = w1.shape[0], w2.shape[0]
    dev = y.device
    np_ = (2,) if split else ()
    yy = _in(y, split)
    rr = _in(res, split)
    wp1 = _pack_pair_weight(w1, split)
    wp2 = _pack_pair_weight(w2, split)
    f = lambda v: v.float().contiguous()
    xo = torch.empty(np_ + (M, N1), dtype=torch.bfloat16, device=dev) if store_x else None
    out = torch.empty(np_ + (M, N2), dtype=torch.bfloat16, device=dev)
    zeros = torch.zeros(4096, dtype=torch.int16, device=dev)
    g = dict(M=M, K1=K1, N1=N1, N2=N2, relu=int(relu), relu2=int(relu2), split=int(split), zeros=int(zeros.data_ptr()),
             shared_w=int(shared_w))
    ao = torch.empty(np_ + (M, N1), dtype=torch.bfloat16, device=dev) if store_a else None
    if store_a:
        g["aout"] = int(ao.data_ptr())
    if split:
        g.update(wplane1=int(wp1[0].numel()), wplane2=int(wp2[0].numel()))
    bb1, ss2, hh2, bb2 = f(b1), f(s2), f(h2), f(b2)
    rc = native.kernels().die_kern_conv_pair(json.dumps(g).encode(), _ptr(yy), _ptr(wp1), _ptr(bb1), _ptr(rr),
                                             _ptr(xo), _ptr(ss2), _ptr(hh2), _ptr(wp2), _ptr(bb2), _ptr(out),
                                             _stream())
    _check(rc, "conv_pair")
    if store_a:
        return (None if xo is None else _out(xo, split)), _out(out, split), _out(ao, split)
    return (None if xo is None else _out(xo, split)), _out(out, split)


def _in(x, split):
    return split_planes(x) if split else x.contiguous()


def _out(y, split):
    return join_planes(y) if split else y


def input_prep(x_nchw, scale=None, shift=None, cp=4, split=False):
    import torch

    B, C, H, W = x_nchw.shape
    out = torch.empty(((2,) if split else ()) + (B, H, W, cp), dtype=torch.bfloat16, device=x_nchw.device)
    L = native.kernels()
    xin = x_nchw.contiguous().float()  # locals keep every launched-on buffer alive through the launch
    rc = L.die_kern_input_prep(_ptr(xin), _ptr(scale), _ptr(shift), _ptr(out), B, C, H, W, cp,
                               _stream(), int(split))
    _check(rc, "input_prep")
    return _out(out, split)


def _live(live, dev):
    """The device-side live batch (kernels.h `live`): an int64 scalar on the device, None = all samples."""
    import torch

    return None if live is None else torch.tensor([int(live)], dtype=torch.int64, device=dev)


def _f32(v):
    return None if v is None else v.float().contiguous()


def _storage(out, shape, split, dev):
    """Raw output storage: bf16 `shape`, or the hi / lo planes [2, *shape] in fp32 mode.  A caller's
    pre-filled `out` is written in place (what a kernel leaves alone stays as it was)."""
    import torch

    full = ((2,) if split else ()) + tuple(shape)
    if out is None:
        return torch.empty(full, dtype=torch.bfloat16, device=dev)
    if tuple(out.shape) != full or out.dtype != torch.bfloat16 or not out.is_contiguous():
        raise ValueError("out must be contiguous bf16 %s, got %s %s" % (full, out.dtype, tuple(out.shape)))
    return out


def _pair(v):
    return (int(v[0]), int(v[1])) if isinstance(v, (tuple, list)) else (int(v), int(v))


def pool2d_nhwc(x, k, stride, pad, is_max=True, count_include_pad=False, split=False, scale=None, shift=None,
                act=0, live=None, out=None):
    """k / stride / pad: one int or (h, w).  scale / shift [C] fp32: the fused per-channel affine on the
    pooled value, then act (1 = ReLU).  live / out: as the generic kernels below take them."""
    B, H, W, C = x.shape
    (kh, kw), (sh, sw), (ph, pw) = _pair(k), _pair(stride), _pair(pad)
    Ho = (H + 2 * ph - kh) // sh + 1
    Wo = (W + 2 * pw - kw) // sw + 1
    y = _storage(out, (B, Ho, Wo, C), split, x.device)
    xin, sc, sf, lv = _in(x, split), _f32(scale), _f32(shift), _live(live, x.device)
    rc = native.kernels().die_kern_pool2d(_ptr(xin), _ptr(y), B, H, W, C, Ho, Wo, kh, kw, sh, sw, ph, pw,
                                          int(is_max), int(count_include_pad), _stream(), int(split), _ptr(lv),
                                          _ptr(sc), _ptr(sf), int(act))
    _check(rc, "pool2d")
    return _out(y, split)


def global_avgpool_nhwc(x, scale=None, shift=None, relu=False, split=False, mode=0, live=None, out=None):
    """mode: 0 mean, 1 sum, 2 max over the H*W pixels (after the optional per-pixel relu(x*scale+shift))."""
    import torch

    B, H, W, C = x.shape
    o = _storage(out, (B, C), split, x.device)
    out32 = torch.empty((B, C), dtype=torch.float32, device=x.device)
    xin, lv = _in(x, split), _live(live, x.device)
    rc = native.kernels().die_kern_gap(_ptr(xin), _ptr(o), _ptr(out32), _ptr(scale), _ptr(shift),
                                       int(relu), B, H * W, C, _stream(), int(split), _ptr(lv), int(mode))
    _check(rc, "global_avgpool")
    return _out(o, split), out32


def affine_act(x, scale=None, shift=None, z=None, relu=False, split=False):
    import torch

    C = x.shape[-1]
    M = x.numel() // C
    y = torch.empty(((2,) if split else ()) + tuple(x.shape), dtype=torch.bfloat16, device=x.device)
    zz = None if z is None else _in(z, split)
    xin = _in(x, split)
    rc = native.kernels().die_kern_affine(_ptr(xin), _ptr(zz), _ptr(scale), _ptr(shift), int(relu), _ptr(y),
                                          M, C, _stream(), int(split))
    _check(rc, "affine_act")
    return _out(y, split)


# ---- transformer kernels (csrc/kernels/transformer.hip) ---------------------------------------------

def linear(x, w, bias=None, act=0, res=None, tile=-1, splits=1, split=False):
    """Rows GEMM on the MFMA conv kernel: x [..., K] bf16, w [N, K] float -> act(x @ w^T + bias + res).
    act: 0 none, 1 relu, 2 erf-GELU.  split: fp32 mode (fp32 result)."""
    K = x.shape[-1]
    lead = x.shape[:-1]
    M = x.numel() // K
    N = w.shape[0]
    r = None if res is None else res.reshape(M, 1, 1, N)
    out, _ = conv2d_nhwc(x.reshape(M, 1, 1, K), w.reshape(N, K, 1, 1), bias=bias, relu=act, res=r, tile=tile,
                         splits=splits, split=split)
    return None if out is None else out.reshape(*lead, N)


def layernorm(x, gamma, beta, eps=1e-5, split=False, variant=0):
    return layernorm_rows(x, gamma, beta, eps, split, variant)


def layernorm_rows(x, gamma, beta=None, eps=1e-5, split=False, variant=0, cl=0, stats=False, rms=False):
    """kern::layernorm_rows with every argument: x [..., C] (bf16, or fp32 with split), the statistics
    over the first `cl` columns (0 = C; the rest are stored pad columns, written 0).  rms: RMSNorm,
    y = x * rsqrt(mean(x^2) + eps) * gamma (beta unused).  stats: statistics mode, returns the fp32
    [rows, 2] (mean, rstd) pairs ((0, rstd) with rms) instead of the rows."""
    import torch

    C = x.shape[-1]
    rows = x.numel() // C
    y = torch.empty(((2,) if split else ()) + tuple(x.shape), dtype=torch.bfloat16, device=x.device)
    st = torch.empty((rows, 2), dtype=torch.float32, device=x.device) if stats else None
    xin, gm = _in(x, split), gamma.float().contiguous()
    bt = None if beta is None else beta.float().contiguous()
    rc = native.kernels().die_kern_layernorm(_ptr(xin), 0 if stats else _ptr(y), _ptr(gm), _ptr(bt), float(eps), rows, C,
                                             _stream(), int(split), int(cl), int(variant), _ptr(st), int(rms))
    _check(rc, "layernorm_rows")
    return st if stats else _out(y, split)


def rope_rows(xbuf, cos, sin, B, S, H, D, col=0, split=False, ybuf=None, check=True):
    """Rotary position embedding (kern::rope_rows) on stored rows.  xbuf: bf16 [B*S, ldx] (split:
    [2, B*S, ldx], the hi / lo planes) with head h at columns col + [h*D, (h+1)*D) -- col / ldx place
    the block inside a wider (fused QKV) buffer; cos / sin: fp32 [S, D]; ybuf (default: a fresh dense
    one): bf16 [(2,) B*S, ldy], head h at columns [h*D, (h+1)*D), written in place.  Returns ybuf, or
    with check=False the pair (hipError code, ybuf) without raising."""
    import torch

    ldx = int(xbuf.shape[-1])
    if ybuf is None:
        ybuf = torch.empty(((2,) if split else ()) + (B * S, H * D), dtype=torch.bfloat16, device=xbuf.device)
    ldy = int(ybuf.shape[-1])
    assert xbuf.is_contiguous() and ybuf.is_contiguous() and cos.is_contiguous() and sin.is_contiguous()
    assert xbuf.dtype == torch.bfloat16 and ybuf.dtype == torch.bfloat16
    assert cos.dtype == torch.float32 and sin.dtype == torch.float32
    rc = native.kernels().die_kern_rope_rows(_ptr(xbuf) + 2 * int(col), _ptr(ybuf), _ptr(cos), _ptr(sin), B, S, H, D, ldx,
                                             ldy, _stream(), int(split))
    if not check:
        return rc, ybuf
    _check(rc, "rope_rows")
    return ybuf


def tokens_assemble(patches, cls=None, pos=None, split=False):
    """patches [B, S0, C] bf16, cls [C] f32, pos [S0+1, C] f32 -> [B, S0+1, C] bf16."""
    import torch

    B, S0, C = patches.shape
    out = torch.empty(((2,) if split else ()) + (B, S0 + 1, C), dtype=torch.bfloat16, device=patches.device)
    pin = _in(patches, split)
    rc = native.kernels().die_kern_tokens(_ptr(pin), _ptr(cls), _ptr(pos), _ptr(out), B, S0, C,
                                          _stream(), int(split))
    _check(rc, "tokens_assemble")
    return _out(out, split)


def gather_rows(x, idx, split=False):
    import torch

    B, S, C = x.shape
    y = torch.empty(((2,) if split else ()) + (B, C), dtype=torch.bfloat16 if split else x.dtype, device=x.device)
    xin = _in(x, split)
    rc = native.kernels().die_kern_gather_rows(_ptr(xin), _ptr(y), B, S, int(idx), C, _stream(), int(split))
    _check(rc, "gather_rows")
    return _out(y, split)


_PAD_OPS = {"eq": 0, "gt": 1, "lt": 2}


def embed_tokens(ids, table, pos=None, type_row=None, pad_test=None, split=False, types=None, type_table=None,
                 mask=None, mask_trunc=False, packed=None):
    """Embedding lookup on token ids carried as numbers: ids [B, S] (any float / int dtype; the kernel
    reads them as fp32), table [V, D] fp32, pos [S, D], type_row [D] ->
    rows[b, s] = table[idx(ids[b, s])] + pos[s] + type_row summed in fp32, with idx = truncate and
    clamp to [0, V - 1] (NaN -> 0).  rows: [B, S, Dp] bf16 (split: fp32 from the hi / lo planes), Dp = D
    rounded up to 8, the pad columns 0.
    pad_test: None, a pad id, or (op, value) with op in "eq" / "gt" / "lt": a key is PADDING where
    `id op value` holds.  Then also returns the attention key data: kvis [B, Sp] fp32 (0 visible,
    -inf padding and columns >= S; Sp = S rounded up to 32) and kend [B] int32 = 1 + the last
    visible key (0: none); else (rows, None, None).
    A table whose rows are 16-byte aligned with a pitch that is a multiple of 4 and >= Dp is read in
    place (a row slice of a larger table, say); any other is copied to pitch Dp.
    Models with attention_mask / token_type_ids inputs (request rows of several segments; without any
    of the following the ids are read densely by the single-input kernel, as before):
    types [B, S] + type_table [T, D]: rows += type_table[idx(types[b, s])] (the same clamp against T;
    the table is read in place under the same rule as `table`); excludes type_row.
    mask [B, S]: the key data comes from the mask, a key is visible where mask != 0 (mask_trunc: where
    trunc(mask) != 0, an integer-declared mask input); excludes pad_test.
    packed = dict(S=, ids=, types=, mask=): `ids` is ONE tensor [B, L] of request rows holding the
    segments at these element offsets (types / mask: None = absent), read in place with pitch L."""
    import torch

    dev = table.device
    if packed is None:  # separate tensors: pack them ids | types | mask
        B, S = ids.shape
        parts, packed = [ids], dict(S=S, ids=0, types=None, mask=None)
        for name, t in (("types", types), ("mask", mask)):
            if t is not None:
                packed[name] = S * len(parts)
                parts.append(t)
        rows = torch.cat([t.to(device=dev, dtype=torch.float32) for t in parts], dim=1).contiguous()
        L = rows.shape[1] if len(parts) > 1 else 0  # ld_in = 0: dense ids, the single-input kernel
    else:
        rows = ids.to(device=dev, dtype=torch.float32).contiguous()
        B, S, L = rows.shape[0], int(packed["S"]), rows.shape[1]
    o_ids, o_types, o_mask = packed["ids"], packed.get("types"), packed.get("mask")
    for off in (o_ids, o_types, o_mask):  # the kernel reads [off, off + S) of every row: keep it inside
        if off is not None and not (0 <= int(off) and int(off) + S <= rows.shape[1]):
            raise ValueError("embed_tokens: segment offset %r with S = %d outside the request row of %d"
                             % (off, S, rows.shape[1]))
    if (o_types is not None) != (type_table is not None) or (o_types is not None and type_row is not None):
        raise ValueError("embed_tokens: a type input needs type_table and excludes type_row")
    if o_mask is not None and pad_test is not None:
        raise ValueError("embed_tokens: mask excludes pad_test")
    V, D = table.shape
    Dp = (D + 7) // 8 * 8

    def padded(t, nrows):
        if t is None:
            return None
        t = t.to(device=dev, dtype=torch.float32).reshape(nrows, D)
        if Dp == D:
            return t.contiguous()
        o = torch.zeros((nrows, Dp), dtype=torch.float32, device=dev)
        o[:, :D] = t
        return o

    def in_place(t):
        if (t.dtype == torch.float32 and t.dim() == 2 and t.stride(1) == 1 and t.stride(0) >= Dp and t.stride(0) % 4 == 0
                and t.data_ptr() % 16 == 0):
            return t, int(t.stride(0))
        return padded(t, t.shape[0]), Dp

    tab, ldt = in_place(table)
    T = 0
    if type_table is not None:
        T = type_table.shape[0]
        ttab, ldtt = in_place(type_table)
    else:
        ttab, ldtt = padded(type_row, 1), Dp
    ps = padded(pos, S)
    out = torch.empty(((2,) if split else ()) + (B, S, Dp), dtype=torch.bfloat16, device=dev)
    kvis = kend = None
    Sp = op = neg = 0
    val = 0.0
    if o_mask is not None:
        op, val, neg = 0, 0.0, 1  # visible = not (mask == 0)
    elif pad_test is not None:
        name, val = pad_test if isinstance(pad_test, (tuple, list)) else ("eq", pad_test)
        op, neg = _PAD_OPS[name], 1  # visible = not (id op value)
    if o_mask is not None or pad_test is not None:
        Sp = (S + 31) // 32 * 32
        kvis = torch.empty((B, Sp), dtype=torch.float32, device=dev)
        kend = torch.empty((B,), dtype=torch.int32, device=dev)
    base = rows.data_ptr()

    def seg(off):
        return 0 if off is None else base + 4 * int(off)

    geom = dict(ids=seg(o_ids), types=seg(o_types), mask=seg(o_mask), ld_in=int(L), table=_ptr(tab), ldt=ldt, pos=_ptr(ps),
                ttab=_ptr(ttab), ldtt=ldtt, T=int(T), out=_ptr(out), B=B, S=S, V=V, C=Dp, split=int(split),
                kvis=_ptr(kvis), kend=_ptr(kend), Sp=Sp, pad_op=op, pad_c=float(val), pad_neg=neg,
                pad_trunc=int(bool(mask_trunc) and o_mask is not None))
    _check(native.kernels().die_kern_embed_tokens(native.geometry(geom), _stream()), "embed_tokens")
    return _out(out, split), kvis, kend


def key_mask_data(visible):
    """bool [B, S] (True = visible key) -> the attention kernels' key data (kvis [B, Sp] fp32 with 0 /
    -inf and -inf in the columns >= S, kend [B] int32 = 1 + the last visible key), as embed_tokens()
    writes it."""
    import torch

    B, S = visible.shape
    Sp = (S + 31) // 32 * 32
    vis = visible.bool()
    kvis = torch.full((B, Sp), float("-inf"), dtype=torch.float32, device=vis.device)
    kvis[:, :S] = torch.where(vis, 0.0, float("-inf"))
    pos = torch.arange(1, S + 1, device=vis.device, dtype=torch.int32)
    kend = (vis.to(torch.int32) * pos).amax(dim=1).to(torch.int32).contiguous()
    return kvis, kend


def pool_tokens(x, key_mask=None, clip_min=0.0, normalize=False, eps=1e-12, split=False, out_f32=True, dim=None,
                counters=None):
    """Token pooling + L2 normalisation: x [B, S, C] (bf16, or fp32 with split) -> one vector per sample.
    key_mask: the (kvis, kend) pair of key_mask_data() / embed_tokens(): the mean runs over the visible
    tokens only, sum / max(count, clip_min), and a sample with none gets zeros; None: the mean of all S
    rows.  normalize: then v / max(||v||_2, eps) over the first `dim` columns (default C; the rest
    are stored pad columns, written 0).  Returns (rows [B, C] bf16 -- fp32 from the hi / lo planes
    with split --, fp32 [B, dim] or None).  counters: an int32 tensor of >= B zeros for the
    cross-block hand-off of a normalised row wider than 64 columns (default: a fresh one); the kernel
    leaves it at 0."""
    import torch

    B, S, C = x.shape
    D = C if dim is None else int(dim)
    dev = x.device
    out = torch.empty(((2,) if split else ()) + (B, C), dtype=torch.bfloat16, device=dev)
    out32 = torch.empty((B, D), dtype=torch.float32, device=dev) if out_f32 else None
    xin = _in(x, split)
    kvis, kend = key_mask if key_mask is not None else (None, None)
    Sp = 0 if kvis is None else int(kvis.shape[1])
    L = native.kernels()
    ws_bytes = int(L.die_kern_pool_tokens_ws_bytes(B, C))
    ws = torch.empty((ws_bytes // 4,), dtype=torch.float32, device=dev)
    if counters is None:
        counters = torch.zeros((B,), dtype=torch.int32, device=dev)
    geom = dict(x=_ptr(xin), out=_ptr(out), out_f32=_ptr(out32), B=B, S=S, C=C, D=D, kvis=_ptr(kvis), kend=_ptr(kend), Sp=Sp,
                clip_min=float(clip_min), normalize=int(normalize), eps=float(eps), split=int(split), ws=_ptr(ws),
                ws_bytes=ws_bytes, counters=_ptr(counters), counters_n=int(counters.numel()))
    _check(L.die_kern_pool_tokens(native.geometry(geom), _stream()), "pool_tokens")
    return _out(out, split), out32


_LOG2E = 1.4426950408889634


def _attention_bias(bias, S, heads, pad=0.0):
    """bias [S, S] or [H, S, S] fp32, natural units -> (the kernel's table [Hb][S][Sp] with Sp = S
    rounded up to 32, pre-multiplied by log2(e) (the kernel's softmax runs in exp2), Hb, Sp).
    pad: what the pad columns [S, Sp) hold (any finite value: the kernel masks those keys)."""
    import torch

    if bias.dim() == 2:
        bias = bias[None]
    if bias.dim() != 3 or bias.shape[0] not in (1, heads) or tuple(bias.shape[1:]) != (S, S):
        raise ValueError("attention bias must be [S, S] or [H, S, S] with S = %d, H = %d, got %s"
                         % (S, heads, tuple(bias.shape)))
    Sp = (S + 31) // 32 * 32
    table = torch.full((bias.shape[0], S, Sp), float(pad), dtype=torch.float32, device=bias.device)
    table[..., :S] = bias.float() * _LOG2E
    return table, int(bias.shape[0]), Sp


def _attention_launch(q, k, v, out, B, S, heads, D, ldq, ldk, ldv, ldo, sc, split, bias, causal, what, key_mask=None,
                      kv_heads=None, bias_pad=0.0):
    kvis = kend = table = None
    hb = 0
    if key_mask is not None:
        if not isinstance(key_mask, (tuple, list)) and tuple(key_mask.shape) != (B, S):
            raise ValueError("key mask must be bool [B, S] = [%d, %d], got %s" % (B, S, tuple(key_mask.shape)))
        kvis, kend = key_mask if isinstance(key_mask, (tuple, list)) else key_mask_data(key_mask)
        if tuple(kvis.shape) != (B, (S + 31) // 32 * 32) or tuple(kend.shape) != (B,):
            raise ValueError("key mask must be bool [B, S] or (kvis [B, Sp] fp32, kend [B] int32), B = %d, S = %d" % (B, S))
    if bias is not None:
        table, hb, _ = _attention_bias(bias, S, heads, bias_pad)
    geom = dict(q=q, k=k, v=v, out=out, B=B, S=S, H=heads, D=D, ldq=ldq, ldk=ldk, ldv=ldv, ldo=ldo, scale=sc, split=split,
                bias=_ptr(table), bias_heads=hb, Sp=(S + 31) // 32 * 32 if (table is not None or kvis is not None) else 0,
                causal=int(bool(causal)), kvis=_ptr(kvis), kend=_ptr(kend), kv_heads=0 if kv_heads is None else int(kv_heads))
    _check(native.kernels().die_kern_attention(native.geometry(geom), _stream()), what)


def attention_launch(q, k, v, out, B, S, heads, D, ldq, ldk, ldv, ldo, scale, split=False, bias=None, causal=False,
                     key_mask=None, kv_heads=None, bias_pad=0.0):
    """The kernel's own calling convention, for callers that own the storage (tests of row pitches,
    column offsets and caller-owned outputs): q, k, v, out are device addresses of the first element of
    [B * S] rows of 16-bit elements at pitches ldq, ldk, ldv (multiples of 8) and ldo (a multiple of
    4), q and out with heads * D columns, k and v with (kv_heads or heads) * D.  split: each is the hi
    plane and its lo plane lies B * S * pitch elements behind it.  The masks are attention()'s;
    bias_pad fills the table's pad columns."""
    _attention_launch(int(q), int(k), int(v), int(out), B, S, heads, D, ldq, ldk, ldv, ldo, float(scale), int(bool(split)),
                      bias, causal, "attention", key_mask, kv_heads, bias_pad)


def attention(q, k, v, heads, scale=None, bias=None, causal=False, key_mask=None, kv_heads=None, out=None, bias_pad=0.0):
    """q/k/v: [B, S, H*D] bf16 (may be column slices of a wider tensor, row stride = stride(1)).
    Returns softmax(scale * Q K^T + bias) V merged back to [B, S, H*D] bf16.
    bias: fp32 [S, S] (shared by the heads) or [H, S, S], natural units, -inf = masked, the same for
    every image of the batch; causal: key j is visible to query i iff j <= i (on top of any bias).
    A query row with no visible key at all is undefined (NaN in ONNX): the caller must not pass one.
    key_mask: per-sample padding, bool [B, S] with True = visible key, or the (kvis, kend) pair of
    embed_tokens() / key_mask_data(); combines with a bias, not with causal (an error).  A sample
    without any visible key gets all-zero rows.
    kv_heads: grouped-query / multi-query attention -- k / v are [B, S, kv_heads * D] and query head h
    reads their head h // (heads // kv_heads).  Head dim 64 or 128, no bias; kv_heads = heads is the
    multi-head launch.
    out: a [B, S, H*D] bf16 tensor to write into (like q, it may be a column slice of wider rows);
    bias_pad: the value in the bias table's pad columns (any finite one gives the same result)."""
    import torch

    B, S, C = q.shape
    D = C // heads
    if out is None:
        out = torch.empty((B, S, C), dtype=torch.bfloat16, device=q.device)
    assert tuple(out.shape) == (B, S, C) and out.dtype == torch.bfloat16
    for t in (q, k, v, out):
        assert t.stride(2) == 1 and t.stride(0) == S * t.stride(1), "rows must be [B*S][ld] with unit column stride"
    sc = float(scale if scale is not None else 1.0 / np.sqrt(D))
    _attention_launch(_ptr(q), _ptr(k), _ptr(v), _ptr(out), B, S, heads, D, q.stride(1), k.stride(1), v.stride(1),
                      out.stride(1), sc, 0, bias, causal, "attention", key_mask, kv_heads, bias_pad)
    return out


def set_attention_variant(v):
    """Process-wide streaming-attention variant (kernels.h set_attention_variant): 0 = K/V staged one
    tile ahead (default), 1 = two tiles ahead, 4 = kv_heads == heads launched through the GQA mode (tests)."""
    native.kernels().die_kern_set_attention_variant(int(v))


def attention_qkv_split(qkv, heads, scale=None, bias=None, causal=False, key_mask=None, kv_heads=None, bias_pad=0.0):
    """fp32 mode: qkv [B, S, 3*C] float (Q | K | V columns) -> fp32 [B, S, C] through the split kernel
    (planes of the packed QKV rows, like the engine's fused QKV GEMM output).  bias / causal: as
    attention() takes them (the bias is fp32 in both precisions); key_mask: likewise.
    kv_heads: qkv is [B, S, (heads + 2 * kv_heads) * D] (Q | K | V with kv_heads heads each in K and V)."""
    import torch

    B, S, C3 = qkv.shape
    if kv_heads is not None:
        D = C3 // (heads + 2 * int(kv_heads))
        C, Ckv = heads * D, int(kv_heads) * D
        planes = split_planes(qkv)
        out = torch.empty((2, B, S, C), dtype=torch.bfloat16, device=qkv.device)
        sc = float(scale if scale is not None else 1.0 / np.sqrt(D))
        base = _ptr(planes)
        _attention_launch(base, base + 2 * C, base + 2 * (C + Ckv), _ptr(out), B, S, heads, D, C3, C3, C3, C, sc, 1, bias,
                          causal, "attention (split)", key_mask, kv_heads, bias_pad)
        return join_planes(out)
    C = C3 // 3
    D = C // heads
    planes = split_planes(qkv)  # [2, B, S, 3C]
    out = torch.empty((2, B, S, C), dtype=torch.bfloat16, device=qkv.device)
    sc = float(scale if scale is not None else 1.0 / np.sqrt(D))
    base = _ptr(planes)
    _attention_launch(base, base + 2 * C, base + 4 * C, _ptr(out), B, S, heads, D, C3, C3, C3, C, sc, 1, bias, causal,
                      "attention (split)", key_mask, None, bias_pad)
    return join_planes(out)


# ---- device JSON decode (csrc/kernels/decode.hip) ---------------------------------------------------

def set_decode_variant(v):
    """Process-wide decode variant (kernels.h set_decode_variant): 0 = packed samples on the nibble-level
    kernels (default), 1 = packed samples expanded to characters by the character kernels (tests)."""
    native.kernels().die_kern_set_decode_variant(int(v))


def decode_json_numbers(texts, numel, text_cap=None, slot_order=None, packed=False):
    """Decode number-list texts (bytes, the inside of a JSON array; None = skipped sample) on the GPU.
    slot_order: optional permutation; sample i's text is then placed in arena slot slot_order[i]
    and located through the per-sample offset table (the engine's staged-upload layout).
    packed: upload every text that packs (core/textpack.h) 4-bit packed, the worker's default (the
    nibble-level kernels decode those; the rest stays raw).
    Returns (values [B, numel] f32, status [B] int32, ntok [B] int32) as torch tensors."""
    import torch

    B = len(texts)
    if text_cap is None:
        text_cap = max(4096, max(len(t) for t in texts if t is not None) + 64)
        text_cap = (text_cap + 4095) // 4096 * 4096
    slots = list(range(B)) if slot_order is None else list(slot_order)
    nslots = max(slots) + 1 if slots else 1
    host = np.zeros(nslots * text_cap, np.uint8)
    lens = np.full(B, -1, np.int64)
    offs = np.zeros(B, np.int64)
    for i, t in enumerate(texts):
        offs[i] = slots[i] * text_cap
        if t is None:
            continue
        assert len(t) <= text_cap
        host[offs[i]:offs[i] + len(t)] = np.frombuffer(t, np.uint8)
        lens[i] = len(t)
    L = native.kernels()
    d_text = torch.from_numpy(host).cuda()
    d_lens = torch.from_numpy(lens).cuda()
    d_offs = torch.from_numpy(offs).cuda() if slot_order is not None else None
    out = torch.full((B, numel), float("nan"), dtype=torch.float32, device="cuda")
    status = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    ntok = torch.zeros(B, dtype=torch.int32, device="cuda")
    scratch = torch.empty(int(L.die_decode_scratch_bytes(B, text_cap)), dtype=torch.uint8, device="cuda")
    d_packed = d_poffs = None
    if packed:
        hp = np.zeros(nslots * text_cap // 2, np.uint8)
        poffs = np.full(B, -1, np.int64)
        for i, t in enumerate(texts):
            pk = native.pack_nibbles(t) if t is not None else None
            if pk is not None:
                poffs[i] = slots[i] * (text_cap // 2)
                hp[poffs[i]:poffs[i] + len(pk)] = np.frombuffer(pk, np.uint8)
        d_packed = torch.from_numpy(hp).cuda()
        d_poffs = torch.from_numpy(poffs).cuda()
        if d_offs is None:
            d_offs = torch.from_numpy(offs).cuda()
    rc = L.die_kern_decode(_ptr(d_text), _ptr(d_offs), _ptr(d_packed), _ptr(d_poffs), text_cap, _ptr(d_lens), B, _ptr(out),
                           numel, _ptr(status), _ptr(ntok), _ptr(scratch), _stream())
    _check(rc, "decode_json_numbers")
    return out, status, ntok


def pack_stem_weight(w, split=False):
    """[64, C<=4, 7, 7] float -> [64][224] bf16 with k = ky*32 + kx*4 + c (kx padded to 8)
    (split: [2][64][224] hi, lo planes)."""
    import torch

    co, ci = w.shape[:2]
    wp = torch.zeros((co, 7, 8, 4), dtype=torch.float32, device=w.device)
    wp[:, :, :7, :ci] = w.float().permute(0, 2, 3, 1)
    wp = wp.reshape(co, 224)
    return split_planes(wp) if split else wp.to(torch.bfloat16).contiguous()


def conv_stem7x7(x_nhwc4, w, bias, relu=True, split=False):
    """ResNet stem on the LDS-patch kernel: x [B,H,W,4] bf16, w [64,C,7,7] -> [B,Ho,Wo,64] bf16.
    split (fp32 mode): x any float dtype, fp32 result."""
    import torch

    B, H, W, C = x_nhwc4.shape
    assert C == 4 and w.shape[0] == 64
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    out = torch.empty(((2,) if split else ()) + (B, Ho, Wo, 64), dtype=torch.bfloat16, device=x_nhwc4.device)
    b = bias.float().contiguous()
    xin, wp = _in(x_nhwc4, split), pack_stem_weight(w, split)
    rc = native.kernels().die_kern_stem(_ptr(xin), _ptr(wp), _ptr(b), _ptr(out),
                                        B, H, W, Ho, Wo, int(relu), _stream(), int(split))
    _check(rc, "conv_stem7x7")
    return _out(out, split)


def conv_stem7x7_nchw(x_nchw, w, bias, scale=None, shift=None, relu=True, split=False, max_blocks=0):
    """Persistent fused stem: x [B,C<=4,H,W] fp32 NCHW (the graph input, no input_prep pass), the
    per-channel input affine x*scale+shift applied on load, w [64,C,7,7] -> [B,Ho,Wo,64] (bf16, or the
    fp32 values of the split planes).  max_blocks > 0 caps the grid (tests: several tiles per block)."""
    import torch

    B, C, H, W = x_nchw.shape
    assert C <= 4 and w.shape[0] == 64
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    out = torch.empty(((2,) if split else ()) + (B, Ho, Wo, 64), dtype=torch.bfloat16, device=x_nchw.device)
    xin = x_nchw.float().contiguous()
    b = bias.float().contiguous()
    sc = None if scale is None else scale.float().contiguous()
    sh = None if shift is None else shift.float().contiguous()
    wp = pack_stem_weight(w, split)
    rc = native.kernels().die_kern_stem_nchw(_ptr(xin), C, _ptr(sc), _ptr(sh), _ptr(wp), _ptr(b), _ptr(out),
                                             B, H, W, Ho, Wo, int(relu), _stream(), int(split), int(max_blocks))
    _check(rc, "conv_stem7x7_nchw")
    return _out(out, split)


# ---- grouped conv / row softmax (csrc/kernels/gconv.hip, transformer.hip) ---------------------------

def grouped_conv(x_nhwc, w, bias=None, stride=1, pads=(0, 0, 0, 0), groups=1, clip=None, relu=False, split=False):
    """x [B,H,W,Cin] (bf16, or any float dtype with split), w [Cout, Cin/groups, k, k] float,
    pads [top, left, bottom, right] -> [B,Ho,Wo,Cout] (fp32 values of the split planes when split)."""
    import torch

    B, H, W, Cin = x_nhwc.shape
    Cout, cpg, KH, KW = w.shape
    Ho = (H + pads[0] + pads[2] - KH) // stride + 1
    Wo = (W + pads[1] + pads[3] - KW) // stride + 1
    xin = _in(x_nhwc, split) if split else x_nhwc.to(torch.bfloat16).contiguous()
    wp = w.float().permute(0, 2, 3, 1).contiguous()
    bp = None if bias is None else bias.float().contiguous()
    out = torch.empty(((2,) if split else ()) + (B, Ho, Wo, Cout), dtype=torch.bfloat16, device=x_nhwc.device)
    act = 3 if clip is not None else (1 if relu else 0)
    lo, hi = clip if clip is not None else (0.0, 0.0)
    geom = dict(B=B, H=H, W=W, Cin=Cin, Ho=Ho, Wo=Wo, Cout=Cout, groups=groups, KH=KH, KW=KW, stride=stride,
                pad_h=pads[0], pad_w=pads[1], act=act, clip_lo=float(lo), clip_hi=float(hi), split=int(split))
    rc = native.kernels().die_kern_gconv(json.dumps(geom).encode(), _ptr(xin), _ptr(wp), _ptr(bp), _ptr(out), _stream())
    _check(rc, "grouped_conv")
    return _out(out, split)


def depthwise_conv(x_nhwc, w, bias=None, pads=(0, 0, 0, 0), stride=1, dilation=1, clip=None, relu=False, residual=None,
                   split=False, want_f32=False, live=None, fill=None, tiled=True, groups=None):
    """Depthwise conv with the whole epilogue, on the tiled kernel (csrc/kernels/dwconv.hip; tiled=False:
    the same call on gconv_kernel, for comparison).  x [B,H,W,C] (bf16, or any float dtype with split),
    w [C,1,k,k] float, pads [top, left, bottom, right], residual [B,Ho,Wo,C] added after the activation,
    live: number of leading samples to compute (a device-side count; the others keep `fill`).
    Returns (stored planes: bf16 [B,Ho,Wo,C], or [2,B,Ho,Wo,C] hi / lo when split; f32 output or None).
    A geometry outside the tiled kernel's scope raises NativeError with hipError 1 and launches nothing."""
    import torch

    B, H, W, C = x_nhwc.shape
    Cout, cpg, KH, KW = w.shape
    Ho = (H + pads[0] + pads[2] - dilation * (KH - 1) - 1) // stride + 1
    Wo = (W + pads[1] + pads[3] - dilation * (KW - 1) - 1) // stride + 1
    dev = x_nhwc.device
    xin = _in(x_nhwc, split) if split else x_nhwc.to(torch.bfloat16).contiguous()
    if tiled:  # [tap][C]
        wp = w.float().reshape(Cout, cpg * KH * KW).t().contiguous()
    else:
        wp = w.float().permute(0, 2, 3, 1).contiguous()
    bp = None if bias is None else bias.float().contiguous()
    rp = None
    if residual is not None:
        rp = _in(residual, split) if split else residual.to(torch.bfloat16).contiguous()
    shape = ((2,) if split else ()) + (B, Ho, Wo, Cout)
    out = torch.empty(shape, dtype=torch.bfloat16, device=dev)
    of = torch.empty((B, Ho, Wo, Cout), dtype=torch.float32, device=dev) if want_f32 else None
    if fill is not None:
        out.fill_(fill)
        if of is not None:
            of.fill_(fill)
    lv = None if live is None else torch.tensor([int(live)], dtype=torch.int64, device=dev)
    act = 3 if clip is not None else (1 if relu else 0)
    lo, hi = clip if clip is not None else (0.0, 0.0)
    geom = dict(B=B, H=H, W=W, Cin=C, Ho=Ho, Wo=Wo, Cout=Cout, groups=C if groups is None else groups, KH=KH, KW=KW,
                stride=stride, dil=dilation, pad_h=pads[0], pad_w=pads[1], act=act, clip_lo=float(lo), clip_hi=float(hi),
                split=int(split))
    rc = native.kernels().die_kern_dwconv(json.dumps(geom).encode(), int(tiled), _ptr(xin), _ptr(wp), _ptr(bp), _ptr(rp),
                                          _ptr(out), _ptr(of), _ptr(lv), _stream())
    _check(rc, "depthwise_conv")
    return out, of


GN_ACTS = {None: 0, "none": 0, "relu": 1, "silu": 2}


def group_norm(x_nhwc, G, gamma=None, beta=None, eps=1e-5, act=None, split=False, live=None, fill=None, Cl=None,
               ws_bytes=None, out=None):
    """GroupNorm / InstanceNorm (csrc/kernels/groupnorm.hip) of x [B,H,W,C] (bf16, or any float dtype with
    split) over G groups of the first Cl (default C) channels; gamma / beta [Cl] float or None; act None,
    "relu" or "silu".  live: number of leading samples to compute (a device-side count; the others keep
    `fill`).  ws_bytes: the workspace size to allocate and declare (default: what the launcher asks for).
    out: a caller's buffer of the stored shape to write into (an error leaves it as it was).
    Returns the stored planes: bf16 [B,H,W,C], or [2,B,H,W,C] hi / lo when split.  Bad arguments raise
    NativeError with hipError 1 and launch nothing."""
    import torch

    B, H, W, C = x_nhwc.shape
    dev = x_nhwc.device
    xin = _in(x_nhwc, split) if split else x_nhwc.to(torch.bfloat16).contiguous()
    gp = None if gamma is None else gamma.float().contiguous()
    bp = None if beta is None else beta.float().contiguous()
    if out is None:
        out = torch.empty(((2,) if split else ()) + (B, H, W, C), dtype=torch.bfloat16, device=dev)
    assert out.shape == ((2,) if split else ()) + (B, H, W, C) and out.dtype == torch.bfloat16 and out.is_contiguous()
    if fill is not None:
        out.fill_(fill)
    need = int(native.kernels().die_groupnorm_workspace_bytes(B, H * W, C, int(G)))
    nbytes = need if ws_bytes is None else int(ws_bytes)
    ws = torch.empty((max(nbytes, 8) + 3) // 4, dtype=torch.float32, device=dev)
    lv = None if live is None else torch.tensor([int(live)], dtype=torch.int64, device=dev)
    geom = dict(B=B, HW=H * W, C=C, Cl=C if Cl is None else int(Cl), G=int(G), eps=float(eps), act=GN_ACTS[act],
                split=int(split), ws_bytes=nbytes)
    rc = native.kernels().die_kern_groupnorm(json.dumps(geom).encode(), _ptr(xin), _ptr(gp), _ptr(bp), _ptr(out),
                                             _ptr(ws), _ptr(lv), _stream())
    _check(rc, "group_norm")
    return out


def grn(x_nhwc, gamma=None, beta=None, eps=1e-6, split=False, live=None, fill=None, out=None, ws_bytes=None, form=0):
    """Global Response Normalization (csrc/kernels/grn.hip) of x [B,H,W,C] (any float dtype; a contiguous bf16
    tensor of the stored shape, [B,H,W,C] or split [2,B,H,W,C], is read where it is): y = gamma * (x * nx) + beta + x with nx = G / (mean_c G + eps), G[b,c] the L2 norm of channel c over
    the map; gamma / beta [C] float or None (0).  live: number of leading samples to compute (a device-side
    count; the others keep `fill`).  out: a caller's buffer of the stored shape to write into, which may be
    the stored planes of x themselves (in place); an error leaves it as it was.  ws_bytes: the workspace size
    to allocate and declare (default: what the launcher asks for); form: GrnArgs::form (measurements).
    Returns the stored planes: bf16 [B,H,W,C], or [2,B,H,W,C] hi / lo when split.  Bad arguments raise
    NativeError with hipError 1 and launch nothing."""
    import torch

    B, H, W, C = x_nhwc.shape[-4:]
    dev = x_nhwc.device
    stored = ((2,) if split else ()) + (B, H, W, C)
    if x_nhwc.dtype == torch.bfloat16 and tuple(x_nhwc.shape) == stored and x_nhwc.is_contiguous():
        xin = x_nhwc  # the stored planes themselves (bf16 [B,H,W,C], split: [2,B,H,W,C]): read in place, no copy
    else:
        assert x_nhwc.dim() == 4
        xin = _in(x_nhwc, split) if split else x_nhwc.to(torch.bfloat16).contiguous()
    gp = None if gamma is None else gamma.float().contiguous()
    bp = None if beta is None else beta.float().contiguous()
    if out is None:
        out = torch.empty(stored, dtype=torch.bfloat16, device=dev)
    assert tuple(out.shape) == stored and out.dtype == torch.bfloat16 and out.is_contiguous()
    if fill is not None:
        out.fill_(fill)
    need = int(native.kernels().die_grn_workspace_bytes(B, H * W, C))
    nbytes = need if ws_bytes is None else int(ws_bytes)
    ws = torch.empty((max(nbytes, 16) + 3) // 4, dtype=torch.float32, device=dev)
    lv = None if live is None else torch.tensor([int(live)], dtype=torch.int64, device=dev)
    geom = dict(B=B, HW=H * W, C=C, eps=float(eps), split=int(split), ws_bytes=nbytes, form=int(form))
    rc = native.kernels().die_kern_grn(json.dumps(geom).encode(), _ptr(xin), _ptr(gp), _ptr(bp), _ptr(out), _ptr(ws),
                                       _ptr(lv), _stream())
    _check(rc, "grn")
    return out


def softmax_rows(x, split=False):
    """x [rows, C] float -> (softmax stored bf16/split -> fp32 values, softmax fp32)."""
    import torch

    rows, C = x.shape
    xin = _in(x, split) if split else x.to(torch.bfloat16).contiguous()
    y = torch.empty(((2,) if split else ()) + (rows, C), dtype=torch.bfloat16, device=x.device)
    yf = torch.empty((rows, C), dtype=torch.float32, device=x.device)
    rc = native.kernels().die_kern_softmax(_ptr(xin), _ptr(y), _ptr(yf), rows, C, _stream(), int(split))
    _check(rc, "softmax_rows")
    return (join_planes(y) if split else y.float()), yf


# ---- generic row / image kernels and batched MatMul (csrc/kernels/generic.hip, bmm.hip) -------------
# Inputs are values (bf16 tensors, or any float dtype with split: converted to hi / lo planes).
# `out`: optional pre-filled raw storage (_storage) the kernel writes in place, so a caller can see
# what it left untouched; `live`: optional int, only the first `live` samples are computed.  Each
# returns the stored values (bf16, or the fp32 hi + lo with split).

def rows_prep(x, Fp, split=False, out=None):
    """fp32 [R, F] -> stored rows [R, Fp] (Fp % 8 == 0, pad columns 0)."""
    R, F = x.shape
    y = _storage(out, (R, Fp), split, x.device)
    xin = _f32(x)
    rc = native.kernels().die_kern_rows_prep(_ptr(xin), _ptr(y), R, F, int(Fp), _stream(), int(split))
    _check(rc, "rows_prep")
    return _out(y, split)


def input_prep_wide(x_nchw, Cp, scale=None, shift=None, split=False, out=None):
    """fp32 NCHW [B, C, H, W] -> x * scale[c] + shift[c] -> NHWC [B, H, W, Cp] (Cp % 8 == 0, pad channels 0)."""
    B, C, H, W = x_nchw.shape
    y = _storage(out, (B, H, W, Cp), split, x_nchw.device)
    xin, sc, sf = _f32(x_nchw), _f32(scale), _f32(shift)
    rc = native.kernels().die_kern_input_prep_wide(_ptr(xin), _ptr(sc), _ptr(sf), _ptr(y), B, C, H, W, int(Cp),
                                                   _stream(), int(split))
    _check(rc, "input_prep_wide")
    return _out(y, split)


def copy_cols(x, y, colx, coly, ncols, split=False):
    """y[r, coly + j] = x[r, colx + j], j < ncols.  x and y are raw storage: bf16 [R, ld], or the planes
    [2, R, ld] with split; either may be a row slice of a taller tensor (the plane distance is
    stride(0), the pitch stride(-2)).  y is written in place and returned."""
    R = x.shape[-2]
    for t in (x, y):
        if t.stride(-1) != 1 or t.shape[-2] != R or t.dim() != (3 if split else 2):
            raise ValueError("copy_cols takes raw rows [R, ld] (split: [2, R, ld]) with unit column stride")
    xp, yp = (int(x.stride(0)), int(y.stride(0))) if split else (0, 0)
    rc = native.kernels().die_kern_copy_cols(_ptr(x), xp, int(x.stride(-2)), int(colx), _ptr(y), yp, int(y.stride(-2)),
                                             int(coly), R, int(ncols), _stream(), int(split))
    _check(rc, "copy_cols")
    return y


def binary_rows(x, y, op, ymode=0, rows_per_sample=1, act=0, a=0.0, b=0.0, Cl=0, live=None, split=False, out=None):
    """act(x op y) over rows [R, C]; ymode 1: y [R / rows_per_sample, C], one row per sample.
    op / act codes and Cl: kernels.h binary_rows / unary_rows."""
    R, C = x.shape
    o = _storage(out, (R, C), split, x.device)
    xin, yin, lv = _in(x, split), _in(y, split), _live(live, x.device)
    rc = native.kernels().die_kern_binary_rows(_ptr(xin), _ptr(yin), _ptr(o), R, C, int(rows_per_sample), int(ymode),
                                               int(op), int(act), float(a), float(b), _stream(), _ptr(lv), int(split),
                                               int(Cl))
    _check(rc, "binary_rows")
    return _out(o, split)


def unary_rows(x, act, a=0.0, b=0.0, scale=None, shift=None, Cl=0, live=None, rows_per_sample=0, split=False,
               out=None):
    """act(x * scale[c] + shift[c]) over rows [R, C] (kernels.h unary_rows for the codes and Cl)."""
    R, C = x.shape
    y = _storage(out, (R, C), split, x.device)
    xin, sc, sf, lv = _in(x, split), _f32(scale), _f32(shift), _live(live, x.device)
    rc = native.kernels().die_kern_unary_rows(_ptr(xin), _ptr(sc), _ptr(sf), _ptr(y), R, C, int(act), float(a),
                                              float(b), _stream(), _ptr(lv), int(rows_per_sample), int(split), int(Cl))
    _check(rc, "unary_rows")
    return _out(y, split)


def where_rows(cond, a, b, Cl=0, live=None, rows_per_sample=1, split=False, out=None):
    """cond != 0 ? a : b over rows [R, C]; a / b: a tensor like cond, or a Python scalar."""
    import torch

    R, C = cond.shape
    o = _storage(out, (R, C), split, cond.device)
    cin, lv = _in(cond, split), _live(live, cond.device)
    ain = _in(a, split) if torch.is_tensor(a) else None
    bin_ = _in(b, split) if torch.is_tensor(b) else None
    rc = native.kernels().die_kern_where_rows(_ptr(cin), _ptr(ain), _ptr(bin_), 0.0 if ain is not None else float(a),
                                              0.0 if bin_ is not None else float(b), _ptr(o), R, C, _stream(),
                                              _ptr(lv), int(rows_per_sample), int(split), int(Cl))
    _check(rc, "where_rows")
    return _out(o, split)


def resize_nhwc(x, Ho, Wo, scale_h, scale_w, coord=0, mode=0, nearest=0, live=None, split=False, out=None):
    """ONNX Resize of NHWC [B, H, W, C] to [B, Ho, Wo, C] (kernels.h resize_nhwc for the codes)."""
    B, H, W, C = x.shape
    y = _storage(out, (B, Ho, Wo, C), split, x.device)
    xin, lv = _in(x, split), _live(live, x.device)
    rc = native.kernels().die_kern_resize_nhwc(_ptr(xin), _ptr(y), B, H, W, C, int(Ho), int(Wo), float(scale_h),
                                               float(scale_w), int(coord), int(mode), int(nearest), _stream(),
                                               _ptr(lv), int(split))
    _check(rc, "resize_nhwc")
    return _out(y, split)


def pad_nhwc(x, Ho, Wo, t, l, sy=1, sx=1, split=False, out=None):
    """NHWC [B, H, W, C] placed at (t, l) of zeros [B, Ho, Wo, C], input pixels sy / sx apart."""
    B, H, W, C = x.shape
    y = _storage(out, (B, Ho, Wo, C), split, x.device)
    xin = _in(x, split)
    rc = native.kernels().die_kern_pad_nhwc(_ptr(xin), _ptr(y), B, H, W, C, int(Ho), int(Wo), int(t), int(l),
                                            _stream(), int(split), int(sy), int(sx))
    _check(rc, "pad_nhwc")
    return _out(y, split)


def rows_to_f32(x, C, split=False):
    """Stored rows [R, ld] -> fp32 [R, C] (their first C columns)."""
    import torch

    R, ld = x.shape
    y = torch.empty((R, C), dtype=torch.float32, device=x.device)
    xin = _in(x, split)
    rc = native.kernels().die_kern_rows_to_f32(_ptr(xin), _ptr(y), R, int(C), ld, _stream(), int(split))
    _check(rc, "rows_to_f32")
    return y


def nhwc_to_nchw_f32_strided(x, C, split=False):
    """Stored NHWC [B, H, W, Cs] -> fp32 NCHW [B, C, H, W] (the first C channels)."""
    import torch

    B, H, W, Cs = x.shape
    y = torch.empty((B, C, H, W), dtype=torch.float32, device=x.device)
    xin = _in(x, split)
    rc = native.kernels().die_kern_nhwc_to_nchw_strided(_ptr(xin), _ptr(y), B, H, W, int(C), Cs, _stream(), int(split))
    _check(rc, "nhwc_to_nchw_f32_strided")
    return y


def bmm_rows(A, Bm, N, K, ldc, live=None, split=False, out=None):
    """C[b] = A[b][:, :K] @ Bm[b][:K, :N] for A [batch, M, lda], Bm [batch, K, ldb] -> [batch, M, ldc],
    the columns [N, ldc) written 0."""
    batch, M, lda = A.shape
    ldb = Bm.shape[2]
    if Bm.shape[0] != batch or Bm.shape[1] != K:
        raise ValueError("Bm must be [batch, K, ldb]")
    o = _storage(out, (batch, M, ldc), split, A.device)
    ain, bin_, lv = _in(A, split), _in(Bm, split), _live(live, A.device)
    rc = native.kernels().die_kern_bmm_rows(_ptr(ain), _ptr(bin_), _ptr(o), batch, M, int(N), int(K), lda, ldb, int(ldc),
                                            _stream(), _ptr(lv), int(split))
    _check(rc, "bmm_rows")
    return _out(o, split)
