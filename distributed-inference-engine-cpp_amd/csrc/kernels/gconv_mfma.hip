// Grouped 3x3 convolution on the matrix cores for gfx950 (NHWC): the grouped convs of ResNeXt / RegNet
// bottlenecks, which gconv_kernel (gconv.hip) walks with one scalar load per product.
//
// Scope: KH == KW == 3, dilation 1, stride 1 or 2, pads >= 0 (the four sides may differ: pad_h / pad_w
// are the top / left pads, the bottom / right ones follow from Ho / Wo), Cin == Cout == C with
// cpg == opg == w in {4, 8, 16, 32}, C % 16 == 0 (C % 64 == 0 is NOT needed), bf16 or split-fp32
// planes, the whole GConvArgs epilogue (bias, ReLU / Clip, residual after the activation, out and / or
// out_f32, the device-side live batch count).  Anything else -- w = 64, the other RegNet widths (24,
// 48, 56 ...), cpg != opg, dilation, other windows -- returns hipErrorInvalidValue, launches nothing
// and stays on gconv_kernel.
//
// Block-diagonal bundles.  The unit of N is a bundle of 16 consecutive output channels, one
// v_mfma_f32_16x16x32_bf16 fragment.  For w <= 16 a bundle is 16 / w whole groups whose inputs are the
// same 16 channels: a dense 16 -> 16 conv whose packed weights are zero off the block diagonal (the
// zeros add exact zeros; the MFMA waste is 4x at w = 4, 2x at w = 8, on a kernel that moves bytes).
// For w = 32 a bundle is half a group and reads the group's 32 channels.  Either way output channels
// [c0, c0 + 64) read input channels [c0, c0 + 64) only, so a block of four waves owns a 64-channel
// chunk (blockIdx.y), one bundle per wave; the waves of a trailing partial chunk past C only help
// with the loads.
//
// Weights stationary.  The host packs [C / 16][16][Kb] bf16 with k = tap * kc + ci (gconv_mfma_pack in
// kernels.h): kc = 16, Kb = 160 (tap 9 does not exist: zeros) or kc = 32, Kb = 288; fp32 mode appends
// the lo plane.  A wave loads its bundle's A fragments once, 5 or 9 K-steps x 4 VGPRs x 1-2 planes,
// and keeps them while the block grid-strides over (sample, 8x8 output tile).  At kc = 16 a K-step is
// two taps (lanes 0-31 the even tap, 32-63 the odd one), at kc = 32 one tap; a lane's 8 k-values are
// 8 consecutive channels of one tap, one 16-byte LDS read.
//
// Activations through LDS, each pixel fetched once.  The tile's halo, 10 x 10 pixels at stride 1 and
// 17 x 17 at stride 2, is staged with the chunk's 64 channels per pixel (128 B per plane, coalesced
// 16-byte loads; pixels outside the image and channels past C as zeros): 12.5 KiB per plane at stride
// 1, 36.1 KiB at stride 2, twice that in fp32 mode (two blocks per CU of 160 KiB at worst).
// The GEMM runs transposed (A = weights, B = pixels), so fragment f of a wave is 16 pixels: columns
// 0-7 of tile rows f and f + 4.  Sixteen lanes then read 16 bytes each at the same channel offset of
// 16 pixels; at a plain 128-byte pitch every second pixel lands on the same banks.  The pitch stays
// 128 B (no padding, which would push the fp32 stride-2 patch past half the LDS) and the eight 16-byte
// slots of pixel p are XOR-swizzled by (p >> 1) & 7: two pixels fill one 256-byte bank row, so the 16
// pixels of a read must differ in (p & 1, (p >> 1) & 7).  Eight consecutive p give four consecutive
// p >> 1 per parity, and the second row must shift p >> 1 by 4 mod 8, i.e. p by 8 mod 16: at stride 1
// the rows f and f + 4 are 4 * 10 = 40 pixels apart; at stride 2 the patch row holds its 9 even
// columns and then its 8 odd ones (so that the 8 pixels of a tap are consecutive there too) and the
// rows are 8 * 17 = 136 apart.  Both are 8 mod 16: conflict-free reads with no padding.
// The patch is single-buffered (two barriers per tile); occupancy, not a second buffer, overlaps one
// block's loads with another's MFMAs.
//
// fp32 mode: three MFMAs per fragment pair (hi.hi + lo.hi + hi.lo, common.h), fp32 accumulation.
// Epilogue: a lane's accumulator is 4 consecutive channels of one pixel; lanes l and l ^ 16 swap one
// fragment of each pair so each ends with two runs of 8 channels: 16-byte residual loads and stores,
// in the order and meaning of gconv_kernel.  Samples >= *live are never touched.
#include "common.h"
#include "kernels.h"

namespace die {
namespace kern {

using namespace die::k;

namespace {

__device__ __forceinline__ float gm_act(float v, int act, float lo, float hi) {
  if (act == 1) return fmaxf(v, 0.f);
  if (act == 3) return fminf(fmaxf(v, lo), hi);
  if (act == 4) return v * __builtin_amdgcn_rcpf(1.f + __expf(-v));             // SiLU
  if (act == 5) return v * fminf(fmaxf(fmaf(v, 1.f / 6.f, 0.5f), 0.f), 1.f);  // HardSwish
  return v;
}

// 16-byte slot of channel group g (8 channels) of patch pixel p, in uint4 units
__device__ __forceinline__ int gm_slot(int p, int g) { return (p << 3) | (g ^ ((p >> 1) & 7)); }

constexpr int gm_patch(int stride) { return stride == 1 ? 10 : 17; }  // halo rows = columns of an 8x8 tile
constexpr size_t gm_lds_bytes(int stride, bool split) {
  return static_cast<size_t>(gm_patch(stride)) * gm_patch(stride) * 128 * (split ? 2 : 1);
}

template <int KC, int STRIDE, bool SPLIT>
__global__ __launch_bounds__(256) void gconv_mfma_kernel(const GConvArgs a) {
  constexpr int NS = KC == 16 ? 5 : 9;       // K-steps of 32
  constexpr int KB = NS * 32;                // packed row length
  constexpr int PW = gm_patch(STRIDE);       // patch rows and pixels per patch row
  constexpr int NPIX = PW * PW;
  constexpr int NLD = (NPIX * 8 + 255) / 256;  // 16-byte loads per thread and plane
  extern __shared__ __attribute__((aligned(16))) uint4 gm_xs[];  // [plane][NPIX * 8]
  const int C = a.Cout;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, li = lane & 15, q = lane >> 4;
  const int c0 = blockIdx.y * 64;
  const int cw = min(64, C - c0);  // channels of this chunk, a multiple of 16
  const bool active = wv * 16 < cw;
  const long long xplane = static_cast<long long>(a.B) * a.H * a.W * C;
  const long long oplane = static_cast<long long>(a.B) * a.Ho * a.Wo * C;

  // the bundle's weights, kept for every tile of this block
  bf16x8 wh[NS], wl[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    uint4 h = make_uint4(0, 0, 0, 0), l = h;
    if (active) {
      const uint16_t* wp = a.wp + (static_cast<long long>(c0 + wv * 16 + li) * KB + s * 32 + q * 8);
      h = *reinterpret_cast<const uint4*>(wp);
      if (SPLIT) l = *reinterpret_cast<const uint4*>(wp + a.wplane);
    }
    wh[s] = __builtin_bit_cast(bf16x8, h);
    wl[s] = __builtin_bit_cast(bf16x8, l);
  }

  // channel group of the chunk this lane reads, and (kc = 16) which tap of a K-step's two
  const int g = KC == 16 ? wv * 2 + (q & 1) : (wv >> 1) * 4 + q;
  const bool odd_tap = KC == 16 && q >= 2;
  // patch pixel of tap (0, 0) of this lane's pixel in fragment f: tile row f + 4 * (li >> 3), column li & 7
  int pb[4];
#pragma unroll
  for (int f = 0; f < 4; ++f) pb[f] = (f + 4 * (li >> 3)) * STRIDE * PW + (li & 7);

  const int tiles_x = (a.Wo + 7) >> 3, tiles_y = (a.Ho + 7) >> 3, tiles = tiles_x * tiles_y;
  long long nb = a.B;
  if (a.live) nb = min(nb, max(*a.live, 0ll));
  const long long items = nb * tiles;

  for (long long it = blockIdx.x; it < items; it += gridDim.x) {
    const int b = static_cast<int>(it / tiles), t = static_cast<int>(it % tiles);
    const int ty0 = (t / tiles_x) * 8, tx0 = (t % tiles_x) * 8;
    const uint16_t* xb = a.x + static_cast<long long>(b) * a.H * a.W * C;

    // ---- stage the halo: all global loads first, then the LDS writes
    uint4 vh[NLD], vl[NLD];
#pragma unroll
    for (int u = 0; u < NLD; ++u) {
      const int idx = tid + u * 256, p = idx >> 3, cg = idx & 7;
      const int py = p / PW, pr = p % PW;
      const int px = STRIDE == 1 ? pr : (pr < 9 ? 2 * pr : 2 * (pr - 9) + 1);
      const int ih = ty0 * STRIDE - a.pad_h + py, iw = tx0 * STRIDE - a.pad_w + px;
      vh[u] = make_uint4(0, 0, 0, 0);
      vl[u] = vh[u];
      if (p < NPIX && cg * 8 < cw && ih >= 0 && ih < a.H && iw >= 0 && iw < a.W) {
        const uint16_t* src = xb + (static_cast<long long>(ih) * a.W + iw) * C + c0 + cg * 8;
        vh[u] = *reinterpret_cast<const uint4*>(src);
        if (SPLIT) vl[u] = *reinterpret_cast<const uint4*>(src + xplane);
      }
    }
    __syncthreads();  // the previous tile's reads are done
#pragma unroll
    for (int u = 0; u < NLD; ++u) {
      const int idx = tid + u * 256, p = idx >> 3, cg = idx & 7;
      if (p < NPIX) {
        gm_xs[gm_slot(p, cg)] = vh[u];
        if (SPLIT) gm_xs[NPIX * 8 + gm_slot(p, cg)] = vl[u];
      }
    }
    __syncthreads();
    if (!active) continue;  // uniform over the wave; it keeps taking part in the barriers above

    f32x4 acc[4];
#pragma unroll
    for (int f = 0; f < 4; ++f) acc[f] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      // offset of this lane's tap in the patch: (ky, kx) -> ky rows, and kx columns (stride 2: column
      // parity 1 lives 9 pixels into the patch row)
      const int t0 = KC == 16 ? 2 * s : s, t1 = t0 + 1;
      const int kx0 = t0 % 3, kx1 = t1 % 3;
      const int o0 = (t0 / 3) * PW + (STRIDE == 1 ? kx0 : (kx0 == 1 ? 9 : kx0 >> 1));
      const int o1 = t1 < 9 ? (t1 / 3) * PW + (STRIDE == 1 ? kx1 : (kx1 == 1 ? 9 : kx1 >> 1)) : o0;
      const int off = odd_tap ? o1 : o0;
      const bool phantom = KC == 16 && t1 >= 9 && odd_tap;  // tap 9: its weights are zero, feed zeros too
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        const int sl = gm_slot(pb[f] + off, g);
        uint4 xh = gm_xs[sl], xl = make_uint4(0, 0, 0, 0);
        if (SPLIT) xl = gm_xs[NPIX * 8 + sl];
        if (phantom) {
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

    // ---- epilogue: acc[f][r] = channel 4 q + r of pixel (row f + 4 (li >> 3), column li & 7).  Lanes
    // l and l ^ 16 swap a fragment of each pair: the even q keeps fragment 2 h, the odd q 2 h + 1.
    const bool oddq = (q & 1) != 0;
    const int co = c0 + wv * 16 + (q >> 1) * 8;
    const int ow = tx0 + (li & 7);
    float yy[2][8];
#pragma unroll
    for (int h = 0; h < 2; ++h) {  // every lane takes part in the exchange, before any bound check
      const f32x4 keep = oddq ? acc[2 * h + 1] : acc[2 * h], send = oddq ? acc[2 * h] : acc[2 * h + 1];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float recv = __shfl_xor(send[r], 16);
        yy[h][r] = oddq ? recv : keep[r];
        yy[h][4 + r] = oddq ? keep[r] : recv;
      }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      float* y = yy[h];
      const int oh = ty0 + 2 * h + (oddq ? 1 : 0) + 4 * (li >> 3);
      if (oh >= a.Ho || ow >= a.Wo) continue;
      const long long o = ((static_cast<long long>(b) * a.Ho + oh) * a.Wo + ow) * C + co;
      float res[8];
      if (a.res) load8v(a.res + o, oplane, SPLIT, res);
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        float v = y[r] + (a.bias ? a.bias[co + r] : 0.f);
        v = gm_act(v, a.act, a.clip_lo, a.clip_hi);
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

template <int KC, int STRIDE, bool SPLIT>
hipError_t launch_gconv_mfma(const GConvArgs& a, hipStream_t s) {
  static const bool attr_set = [] {  // once, outside any graph capture's launches
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(gconv_mfma_kernel<KC, STRIDE, SPLIT>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    return true;
  }();
  (void)attr_set;
  const int chunks = (a.Cout + 63) / 64;
  const long long items = static_cast<long long>(a.B) * ((a.Ho + 7) / 8) * ((a.Wo + 7) / 8);
  // about four blocks per CU over the chunks; a block keeps its weights over its share of the tiles
  const long long cap = (1024 + chunks - 1) / chunks;
  const dim3 grid(static_cast<unsigned>(items < cap ? items : cap), static_cast<unsigned>(chunks));
  hipLaunchKernelGGL((gconv_mfma_kernel<KC, STRIDE, SPLIT>), grid, dim3(256), gm_lds_bytes(STRIDE, SPLIT), s, a);
  return hipGetLastError();
}

}  // namespace

hipError_t grouped_conv_mfma(const GConvArgs& a, hipStream_t s) {
  if (!grouped_conv_mfma_supported(a) || !a.wp || !a.x || (!a.out && !a.out_f32) || a.B < 1 || a.H < 1 || a.W < 1 ||
      a.Ho < 1 || a.Wo < 1 || (a.split && a.wplane <= 0) || (a.Cout + 63) / 64 > 65535)
    return hipErrorInvalidValue;
  const bool k32 = a.Cout / a.groups == 32, s2 = a.stride == 2, sp = a.split != 0;
  if (k32) {
    if (s2) return sp ? launch_gconv_mfma<32, 2, true>(a, s) : launch_gconv_mfma<32, 2, false>(a, s);
    return sp ? launch_gconv_mfma<32, 1, true>(a, s) : launch_gconv_mfma<32, 1, false>(a, s);
  }
  if (s2) return sp ? launch_gconv_mfma<16, 2, true>(a, s) : launch_gconv_mfma<16, 2, false>(a, s);
  return sp ? launch_gconv_mfma<16, 1, true>(a, s) : launch_gconv_mfma<16, 1, false>(a, s);
}

}  // namespace kern
}  // namespace die
