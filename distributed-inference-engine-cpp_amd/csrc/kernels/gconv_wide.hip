// Grouped 3x3 convolution on the matrix cores for the wide group widths of gfx950 (NHWC): the grouped
// convs of RegNet (w = 24, 40, 48, 56) and of the last stage of ResNeXt-101 32x8d (w = 64), which
// gconv_mfma.hip leaves on gconv_kernel (gconv.hip: one scalar load per product).
//
// Scope: KH == KW == 3, dilation 1, stride 1 or 2, pads >= 0 (the four sides may differ: pad_h / pad_w
// are the top / left pads, the bottom / right ones follow from Ho / Wo), Cin == Cout == C = groups * w
// with w in {24, 40, 48, 56, 64} and any groups >= 1 (C = 72, 120, 168, 888 ...: no other
// divisibility), bf16 or split-fp32 planes, the whole GConvArgs epilogue (bias, act 0 / 1 / 3 / 4 / 5,
// residual after the activation, out and / or out_f32, the device-side live batch count).  Anything
// else returns hipErrorInvalidValue and launches nothing: widths 4 / 8 / 16 / 32 belong to
// gconv_mfma.hip; widths above 64 (112, 120, 128, 168, 232) stay on gconv_kernel, because a group's
// weights no longer fit a wave's registers there and a dense per-group GEMM is the right tool.
//
// One group per block.  blockIdx.y is the group, and the block grid-strides over (sample, 8x8 output
// tile).  The GEMM runs transposed as in gconv_mfma.hip (A = weights, B = pixels,
// v_mfma_f32_16x16x32_bf16): fragment f is 16 pixels, columns 0-7 of tile rows f and f + 4, and the
// tile's 64 pixels are 4 fragments.
//
// N axis.  The group's w output channels are NB = ceil(w / 16) bundles of 16; w % 16 is 0 or 8, so the
// last bundle of w = 24 / 40 / 56 is half real: its rows 8-15 are zero weights and never stored.  The
// four waves take (bundle, pixels) like this:
//   w = 56, 64 (NB = 4): wave v = bundle v, all 4 fragments;
//   w = 40, 48 (NB = 3): waves 0-2 = bundles 0-2, all 4 fragments; wave 3 only helps with the loads
//                        (splitting 12 (bundle, fragment) units evenly would make every wave hold all
//                        three bundles' weights, 3 x the registers);
//   w = 24     (NB = 2): wave v = bundle v >> 1, fragments 2 (v & 1) and 2 (v & 1) + 1: all four waves
//                        issue MFMAs and each keeps one bundle's weights.
//
// K axis, packed without per-tap padding.  k = tap * w + ci, K = 9 w rounded up to a multiple of 32
// with zero weights: NS = 7 / 12 / 14 / 16 / 18 K-steps for w = 24 / 40 / 48 / 56 / 64 (padding every
// tap to 32 or 64 channels would cost 9 / 18 / 18 / 18 / 18).  A lane's 8 k-values start at a multiple
// of 8 and w % 8 == 0, so they never straddle a tap: one 16-byte LDS read whose offset (tap pixel,
// channel slot) depends on (K-step, lane >> 4) only: four compile-time constants per step (gw_koff),
// picked by the lane's quarter -- no division in the loop.  The k-values of the last step past 9 w (w = 24,
// 40, 48, 56) have zero weights and are fed zeros.  The host packs [groups][NB * 16][Kp] bf16
// (gconv_wide_pack in kernels.h); fp32 mode appends the lo plane.
//
// Weights stationary.  A wave loads its bundle's A fragments once, NS x 4 VGPRs x 1-2 planes (144 at
// w = 64 in fp32 mode), and keeps them over its share of the tiles.  The halo is staged in rounds of
// at most 4 loads per thread and plane so that the staging registers stay below the accumulators and
// B fragments they alternate with; every instance fits 256 VGPRs (two blocks per CU) without scratch
// (profiles/gconv_wide.md has the compiler's figures).
//
// Activations through LDS, each pixel fetched once.  The tile's halo, 10 x 10 pixels at stride 1 and
// 17 x 17 at stride 2 (even columns first, then the odd ones, so that the 8 pixels of a tap are
// consecutive there too), is staged with the group's w channels only, w / 8 coalesced 16-byte loads
// per pixel and plane; pixels outside the image are zeros.  Sixteen lanes of a fragment read 16 bytes
// each at one channel slot of 16 pixels p0 .. p0 + 7 and p0 + D .. p0 + D + 7, where D = 4 * 10 = 40
// at stride 1 and 8 * 17 = 136 at stride 2, both 8 mod 16.  The 64 banks hold sixteen 16-byte slots:
//   pitch of U slots, U odd: the pixel's slot is p * U mod 16, and p -> p * U is a bijection mod 16
//     over p0 .. p0 + 15 (the second row counts as p0 + 8 .. p0 + 15): conflict-free.  U = w / 8 is odd
//     for w = 24, 40, 56 (no padding at all); w = 48 is padded from 6 to 7 slots (112 B);
//   w = 64: padding to 9 slots would make the fp32 stride-2 patch 81.3 KiB, more than half the LDS.
//     The pitch is 8.5 slots instead: slot(p, g) = 8 p + (p >> 1) + g, one spare slot per pair of pixels.
//     Eight consecutive pixels from an even p0 = 2 m land on slots m + {0, 8, 1, 9, 2, 10, 3, 11} mod 16
//     and the second row, D / 2 = 4 mod 8 pairs further, on the other eight: conflict-free.  From an odd
//     p0 the rows take m + {8, 1, 9, 2, 10, 3, 11, 4} and m + {12, 5, 13, 6, 14, 7, 15, 8}: one slot is
//     hit twice, a single 2-way conflict in the reads of the taps at an odd patch offset (3 of 9 taps at
//     stride 1, 5 of 9 at stride 2); no layout of 8.5 slots avoids it.  gconv_mfma.hip's XOR swizzle is
//     conflict-free in 8 slots, but it is not additive: the compiler then keeps all NS x 4 swizzled
//     addresses live across the tiles and spills the weights to scratch.
//   Either way a read's address is (lane and K-step part) + (fragment part), and the fragment part is a
//   compile-time constant (the fragments are 10 or 34 pixels apart, both even): the ds_read's immediate.
// Worst case 2 x 39,312 B = 76.8 KiB (w = 64, stride 2, fp32): two blocks per CU of 160 KiB.
// The patch is single-buffered (two barriers per tile); occupancy overlaps one block's loads with
// another's MFMAs.
//
// fp32 mode: three MFMAs per fragment pair (hi.hi + lo.hi + hi.lo, common.h), fp32 accumulation.
// Epilogue: a lane's accumulator is 4 consecutive channels of one pixel; lanes l and l ^ 16 swap one
// fragment of each pair so each ends with two runs of 8 channels: 16-byte residual loads and stores,
// in the order and meaning of gconv_kernel; the runs of a half bundle's missing rows are skipped.
// Samples >= *live are never touched.
#include "common.h"
#include "kernels.h"

namespace die {
namespace kern {

using namespace die::k;

namespace {

__device__ __forceinline__ float gw_act(float v, int act, float lo, float hi) {
  if (act == 1) return fmaxf(v, 0.f);
  if (act == 3) return fminf(fmaxf(v, lo), hi);
  if (act == 4) return v * __builtin_amdgcn_rcpf(1.f + __expf(-v));             // SiLU
  if (act == 5) return v * fminf(fmaxf(fmaf(v, 1.f / 6.f, 0.5f), 0.f), 1.f);  // HardSwish
  return v;
}

constexpr int gw_patch(int stride) { return stride == 1 ? 10 : 17; }  // halo rows = columns of an 8x8 tile
constexpr int gw_pitch(int w) { return w == 64 ? 8 : (w / 8) | 1; }   // 16-byte slots per patch pixel
// uint4 slots of one plane of the patch (w = 64: 8 slots per pixel and one more per pair of pixels)
constexpr int gw_plane(int w, int stride) {
  return gw_patch(stride) * gw_patch(stride) * gw_pitch(w) + (w == 64 ? (gw_patch(stride) * gw_patch(stride)) / 2 + 1 : 0);
}
constexpr size_t gw_lds_bytes(int w, int stride, bool split) {
  return static_cast<size_t>(gw_plane(w, stride)) * 16 * (split ? 2 : 1);
}

// 16-byte slot of channel group g (8 channels) of patch pixel p, in uint4 units
template <int W>
__device__ __forceinline__ int gw_slot(int p, int g) {
  if (W == 64) return p * 8 + (p >> 1) + g;
  return p * gw_pitch(W) + g;
}

// Where the 8 k-values from k0 on live, relative to a fragment pixel's tap (0, 0): the tap's patch pixel
// (stride 2: column parity 1 lives 9 pixels into the patch row) and the channel slot.  W != 64: one
// offset in uint4 units; W == 64: the pixel offset alone (the slot goes through gw_slot).
template <int W, int STRIDE>
__host__ __device__ constexpr int gw_koff(int k0) {
  if (k0 >= 9 * W) return 0;  // padding: fed zeros
  const int tap = k0 / W, ci8 = (k0 % W) >> 3, ky = tap / 3, kx = tap % 3;
  const int po = ky * gw_patch(STRIDE) + (STRIDE == 1 ? kx : (kx == 1 ? 9 : kx >> 1));
  return W == 64 ? po : po * gw_pitch(W) + ci8;
}

template <int W, int STRIDE, bool SPLIT>
__global__ __launch_bounds__(256, 2) void gconv_wide_kernel(const GConvArgs a) {
  constexpr int NB = (W + 15) / 16;          // bundles of 16 output channels
  constexpr int KP = (9 * W + 31) / 32 * 32; // packed row length
  constexpr int NS = KP / 32;                // K-steps of 32
  constexpr int PH = NB == 2 ? 2 : 1;        // waves sharing a bundle, each with 4 / PH fragments
  constexpr int NF = 4 / PH;
  constexpr int G8 = W / 8;                  // 16-byte channel slots of a pixel that hold data
  constexpr int U = gw_pitch(W);
  constexpr int PW = gw_patch(STRIDE);       // patch rows and pixels per patch row
  constexpr int NPIX = PW * PW;
  constexpr int PL = gw_plane(W, STRIDE);       // uint4 slots per plane
  constexpr int NLD = (NPIX * G8 + 255) / 256;  // 16-byte loads per thread and plane
  constexpr int RND = 4;                        // loads in flight per staging round
  extern __shared__ __attribute__((aligned(16))) uint4 gw_xs[];  // [plane][PL]
  const int C = a.Cout;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, li = lane & 15, q = lane >> 4;
  const int c0 = blockIdx.y * W;  // the group's first channel
  const int bundle = wv / PH, f0 = (wv % PH) * NF;
  const bool active = bundle < NB;
  const long long xplane = static_cast<long long>(a.B) * a.H * a.W * C;
  const long long oplane = static_cast<long long>(a.B) * a.Ho * a.Wo * C;

  // the bundle's weights, kept for every tile of this block
  bf16x8 wh[NS], wl[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    uint4 h = make_uint4(0, 0, 0, 0), l = h;
    if (active) {
      const uint16_t* wp = a.wp + ((static_cast<long long>(blockIdx.y) * (NB * 16) + bundle * 16 + li) * KP + s * 32 + q * 8);
      h = *reinterpret_cast<const uint4*>(wp);
      if (SPLIT) l = *reinterpret_cast<const uint4*>(wp + a.wplane);
    }
    wh[s] = __builtin_bit_cast(bf16x8, h);
    wl[s] = __builtin_bit_cast(bf16x8, l);
  }

  const bool tail = (NS - 1) * 32 + q * 8 >= 9 * W;  // the last K-step's k-values of this lane are padding
  // tap (0, 0) of this lane's pixel in fragment f0: tile row f0 + 4 * (li >> 3), column li & 7, as a
  // patch pixel (W == 64) or in uint4 units (times the pitch); fragment f0 + f is FOFF pixels further
  constexpr int FOFF = STRIDE * PW;
  const int lb0 = ((f0 + 4 * (li >> 3)) * FOFF + (li & 7)) * (W == 64 ? 1 : U);

  const int tiles_x = (a.Wo + 7) >> 3, tiles_y = (a.Ho + 7) >> 3, tiles = tiles_x * tiles_y;
  long long nb = a.B;
  if (a.live) nb = min(nb, max(*a.live, 0ll));
  const long long items = nb * tiles;

  for (long long it = blockIdx.x; it < items; it += gridDim.x) {
    const int b = static_cast<int>(it / tiles), t = static_cast<int>(it % tiles);
    const int ty0 = (t / tiles_x) * 8, tx0 = (t % tiles_x) * 8;
    const uint16_t* xb = a.x + static_cast<long long>(b) * a.H * a.W * C + c0;

    // ---- stage the halo in rounds: a round's global loads first, then its LDS writes
    __syncthreads();  // the previous tile's reads are done
#pragma unroll 1
    for (int u0 = 0; u0 < NLD; u0 += RND) {
      uint4 vh[RND], vl[RND];
#pragma unroll
      for (int u = 0; u < RND; ++u) {
        const int idx = tid + (u0 + u) * 256, p = idx / G8, cg = idx % G8;
        const int py = p / PW, pr = p % PW;
        const int px = STRIDE == 1 ? pr : (pr < 9 ? 2 * pr : 2 * (pr - 9) + 1);
        const int ih = ty0 * STRIDE - a.pad_h + py, iw = tx0 * STRIDE - a.pad_w + px;
        vh[u] = make_uint4(0, 0, 0, 0);
        vl[u] = vh[u];
        if (p < NPIX && ih >= 0 && ih < a.H && iw >= 0 && iw < a.W) {
          const uint16_t* src = xb + (static_cast<long long>(ih) * a.W + iw) * C + cg * 8;
          vh[u] = *reinterpret_cast<const uint4*>(src);
          if (SPLIT) vl[u] = *reinterpret_cast<const uint4*>(src + xplane);
        }
      }
#pragma unroll
      for (int u = 0; u < RND; ++u) {
        const int idx = tid + (u0 + u) * 256, p = idx / G8, cg = idx % G8;
        if (p < NPIX) {
          gw_xs[gw_slot<W>(p, cg)] = vh[u];
          if (SPLIT) gw_xs[PL + gw_slot<W>(p, cg)] = vl[u];
        }
      }
    }
    __syncthreads();
    if (!active) continue;  // uniform over the wave; it keeps taking part in the barriers above

    f32x4 acc[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) acc[f] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      // this lane's offset of the step: four compile-time constants, picked by the lane's quarter
      const int o0 = gw_koff<W, STRIDE>(s * 32), o1 = gw_koff<W, STRIDE>(s * 32 + 8),
                o2 = gw_koff<W, STRIDE>(s * 32 + 16), o3 = gw_koff<W, STRIDE>(s * 32 + 24);
      const int ko = lb0 + (q < 2 ? (q == 0 ? o0 : o1) : (q == 2 ? o2 : o3));
      const bool pad_k = s == NS - 1 && 9 * W % 32 != 0 && tail;
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        // the fragment's share of the address is a constant, the read's immediate offset (W == 64: FOFF is
        // even, so the half slot per pixel adds up too)
        const int sl = W == 64 ? gw_slot<W>(ko, (s & 1) * 4 + q) + f * (FOFF * 8 + FOFF / 2) : ko + f * FOFF * U;
        uint4 xh = gw_xs[sl], xl = make_uint4(0, 0, 0, 0);
        if (SPLIT) xl = gw_xs[PL + sl];
        if (pad_k) {
          xh = make_uint4(0, 0, 0, 0);
          xl = xh;
        }
        const bf16x8 bh = __builtin_bit_cast(bf16x8, xh), bl = __builtin_bit_cast(bf16x8, xl);
        if (SPLIT) {
          acc[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wl[s], bh, acc[f], 0, 0, 0);
          acc[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[s], bl, acc[f], 0, 0, 0);
        }
        acc[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[s], bh, acc[f], 0, 0, 0);
      }
    }

    // ---- epilogue: acc[f][r] = channel 4 q + r of the bundle, pixel (row f0 + f + 4 (li >> 3), column
    // li & 7).  Lanes l and l ^ 16 swap a fragment of each pair: the even q keeps fragment 2 h, the odd q
    // 2 h + 1.
    const bool oddq = (q & 1) != 0;
    const int cg0 = bundle * 16 + (q >> 1) * 8;  // this lane's 8 channels within the group
    const int co = c0 + cg0;
    const int ow = tx0 + (li & 7);
    float yy[NF / 2][8];
#pragma unroll
    for (int h = 0; h < NF / 2; ++h) {  // every lane takes part in the exchange, before any bound check
      const f32x4 keep = oddq ? acc[2 * h + 1] : acc[2 * h], send = oddq ? acc[2 * h] : acc[2 * h + 1];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float recv = __shfl_xor(send[r], 16);
        yy[h][r] = oddq ? recv : keep[r];
        yy[h][4 + r] = oddq ? keep[r] : recv;
      }
    }
    if (cg0 >= W) continue;  // the missing rows of a half bundle
#pragma unroll
    for (int h = 0; h < NF / 2; ++h) {
      float* y = yy[h];
      const int oh = ty0 + f0 + 2 * h + (oddq ? 1 : 0) + 4 * (li >> 3);
      if (oh >= a.Ho || ow >= a.Wo) continue;
      const long long o = ((static_cast<long long>(b) * a.Ho + oh) * a.Wo + ow) * C + co;
      float res[8];
      if (a.res) load8v(a.res + o, oplane, SPLIT, res);
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        float v = y[r] + (a.bias ? a.bias[co + r] : 0.f);
        v = gw_act(v, a.act, a.clip_lo, a.clip_hi);
        if (a.res) v += res[r];
        y[r] = v;
      }
      if (a.out) store8v(a.out + o, oplane, SPLIT, y);
      if (a.out_f32) {
        float4* of = reinterpret_cast<float4*>(a.out_f32 + o);
        of[0] = make_float4(y[0], y[1], y[2], y[3]);
        of[1] = make_float4(y[4], y[5], y[6], y[7]);
      }
    }
  }
}

template <int W, int STRIDE, bool SPLIT>
hipError_t launch_gconv_wide(const GConvArgs& a, hipStream_t s) {
  static const bool attr_set = [] {  // once, outside any graph capture's launches
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(gconv_wide_kernel<W, STRIDE, SPLIT>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    return true;
  }();
  (void)attr_set;
  const long long items = static_cast<long long>(a.B) * ((a.Ho + 7) / 8) * ((a.Wo + 7) / 8);
  // about four blocks per CU over the groups; a block keeps its weights over its share of the tiles
  const long long cap = (1024 + a.groups - 1) / a.groups;
  const dim3 grid(static_cast<unsigned>(items < cap ? items : cap), static_cast<unsigned>(a.groups));
  hipLaunchKernelGGL((gconv_wide_kernel<W, STRIDE, SPLIT>), grid, dim3(256), gw_lds_bytes(W, STRIDE, SPLIT), s, a);
  return hipGetLastError();
}

template <int W>
hipError_t dispatch_gconv_wide(const GConvArgs& a, hipStream_t s) {
  if (a.stride == 2) return a.split ? launch_gconv_wide<W, 2, true>(a, s) : launch_gconv_wide<W, 2, false>(a, s);
  return a.split ? launch_gconv_wide<W, 1, true>(a, s) : launch_gconv_wide<W, 1, false>(a, s);
}

}  // namespace

hipError_t grouped_conv_wide(const GConvArgs& a, hipStream_t s) {
  if (!grouped_conv_wide_supported(a) || !a.wp || !a.x || (!a.out && !a.out_f32) || a.B < 1 || a.H < 1 || a.W < 1 ||
      a.Ho < 1 || a.Wo < 1 || (a.split && a.wplane <= 0) || a.groups > 65535)
    return hipErrorInvalidValue;
  switch (a.Cout / a.groups) {
    case 24: return dispatch_gconv_wide<24>(a, s);
    case 40: return dispatch_gconv_wide<40>(a, s);
    case 48: return dispatch_gconv_wide<48>(a, s);
    case 56: return dispatch_gconv_wide<56>(a, s);
    default: return dispatch_gconv_wide<64>(a, s);
  }
}

}  // namespace kern
}  // namespace die
