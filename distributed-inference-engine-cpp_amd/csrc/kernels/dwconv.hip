// Tiled depthwise convolution for gfx950 (NHWC), for the large windows of ConvNeXt-style blocks:
// depthwise only (groups == Cin == Cout), stride 1, dilation 1, square 5x5 / 7x7 windows, any pads,
// C % 8 == 0, bf16 or split-fp32 planes, the epilogue of GConvArgs (bias, ReLU / Clip, residual,
// out / out_f32, the device-side live batch bound).  Everything else stays with gconv.hip.
//
// gconv_kernel<true> walks the window with one global load per tap: 49 loads per 8 outputs at 7x7,
// shared between neighbours only by the caches.  Here a block owns TH x TW output pixels of one
// sample times a slice of 32 channels and stages the input tile WITH its halo, (TH+K-1) x (TW+K-1)
// pixels, into LDS once (hi + lo joined to fp32, out-of-image pixels and channels past C as zeros),
// and the slice's K*K x 32 weights (fp32 [tap][C] in global memory) next to it.  A thread keeps 8
// channels of R vertically adjacent outputs: per tap two 16-byte reads of the weights, which every
// thread of a channel group shares, and two per output of the input.  Taps are accumulated in (ky, kx) order
// with the expression gconv_kernel uses, and a zero halo adds exact zeros, so the two kernels agree
// bit for bit.  Partial tiles and a partial last slice are masked on the store.
//
// LDS: a pixel is 32 fp32 = 128 B = 8 slots of 16 B, laid out [half][channel group][4] so that the
// four channel groups of a pixel read four neighbouring slots.  Lane l holds channel group l % 4 of
// column (l / 4) % TW.  ds_read_b128 serves a wave in four groups of 16 lanes, and each group holds
// four columns that are distinct mod 4 ({0,3,5,6} and {1,2,4,7}, then the same + 8).  The halo
// row pitch PW is a multiple of 4 pixels, so a pixel's index p is the column plus a constant mod 4;
// a pixel starts at slot 8 * (p & 1) of the 16-slot bank row and the two halves are swapped where
// p & 2 is set, so the four columns of a group start at slots 0, 4, 8 and 12: the 16 lanes read 16
// distinct slots, no conflict, with no padding between pixels.  The weight reads are four addresses
// per wave (broadcast).
// 7x7, TW = 16: (14 x 24 + 49) x 128 B = 48.1 KiB per block, three blocks per CU of 160 KiB;
// TW = 8 (maps up to 8 wide): 34.1 KiB.
#include "common.h"
#include "kernels.h"

namespace die {
namespace kern {

using namespace die::k;

namespace {

__device__ __forceinline__ float dw_act(float v, int act, float lo, float hi) {
  if (act == 1) return fmaxf(v, 0.f);
  if (act == 3) return fminf(fmaxf(v, lo), hi);
  return v;
}

constexpr int kDwTH = 8;      // output rows of a tile
constexpr int kDwR = 2;       // vertical run of one thread
constexpr int kDwSlice = 32;  // channels of a block (divides 96, 192, 384, 768)

template <int K, int TW>
__global__ __launch_bounds__(16 * TW) void dwconv_kernel(const GConvArgs a) {
  constexpr int TH = kDwTH, R = kDwR, HH = TH + K - 1, HW = TW + K - 1, PW = (HW + 3) / 4 * 4, NT = 16 * TW;
  static_assert(4 * TW * (TH / R) == NT, "one thread per (channel group, column, run)");
  __shared__ float4 xs[HH * PW * 8];
  __shared__ float4 ws[K * K * 8];
  const int b = blockIdx.z;
  if (a.live && b >= *a.live) return;  // uniform over the block
  const int tiles_x = (a.Wo + TW - 1) / TW;
  const int ty0 = (blockIdx.x / tiles_x) * TH, tx0 = (blockIdx.x % tiles_x) * TW;
  const int c0 = blockIdx.y * kDwSlice;
  const int C = a.Cout;
  const bool split = a.split != 0;
  const long long xplane = static_cast<long long>(a.B) * a.H * a.W * C;
  const long long oplane = static_cast<long long>(a.B) * a.Ho * a.Wo * C;
  const uint16_t* xb = a.x + static_cast<long long>(b) * a.H * a.W * C;

  for (int i = threadIdx.x; i < HH * PW * 4; i += NT) {
    const int g = i & 3, p = i >> 2, py = p / PW, px = p % PW;
    if (px >= HW) continue;  // pitch padding: never read
    const int ih = ty0 - a.pad_h + py, iw = tx0 - a.pad_w + px, c = c0 + g * 8;
    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (ih >= 0 && ih < a.H && iw >= 0 && iw < a.W && c < C)
      load8v(xb + (static_cast<long long>(ih) * a.W + iw) * C + c, xplane, split, v);
    const int s = (p >> 1) & 1;
    xs[p * 8 + s * 4 + g] = make_float4(v[0], v[1], v[2], v[3]);
    xs[p * 8 + (s ^ 1) * 4 + g] = make_float4(v[4], v[5], v[6], v[7]);
  }
  for (int i = threadIdx.x; i < K * K * 4; i += NT) {
    const int g = i & 3, tap = i >> 2, c = c0 + g * 8;
    float4 w0 = make_float4(0.f, 0.f, 0.f, 0.f), w1 = w0;
    if (c < C) {
      const float4* wp = reinterpret_cast<const float4*>(a.w + static_cast<long long>(tap) * C + c);
      w0 = wp[0];
      w1 = wp[1];
    }
    ws[tap * 8 + g] = w0;
    ws[tap * 8 + 4 + g] = w1;
  }
  __syncthreads();

  const int g = threadIdx.x & 3, col = (threadIdx.x >> 2) % TW, run = threadIdx.x / (4 * TW);
  float acc[R][8];
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int t = 0; t < 8; ++t) acc[r][t] = 0.f;
  // one window row per iteration: fully unrolled, the compiler hoists all K * K * (2 + 2 R) LDS reads
  // ahead of the arithmetic and spills (7x7: 512 registers and 1.6 KiB of scratch per lane)
#pragma unroll 1
  for (int ky = 0; ky < K; ++ky) {
#pragma unroll
    for (int kx = 0; kx < K; ++kx) {
      const float4 w0 = ws[(ky * K + kx) * 8 + g], w1 = ws[(ky * K + kx) * 8 + 4 + g];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int p = (run * R + r + ky) * PW + col + kx;
        const int s = (p >> 1) & 1;
        const float4 v0 = xs[p * 8 + s * 4 + g], v1 = xs[p * 8 + (s ^ 1) * 4 + g];
        acc[r][0] += v0.x * w0.x;
        acc[r][1] += v0.y * w0.y;
        acc[r][2] += v0.z * w0.z;
        acc[r][3] += v0.w * w0.w;
        acc[r][4] += v1.x * w1.x;
        acc[r][5] += v1.y * w1.y;
        acc[r][6] += v1.z * w1.z;
        acc[r][7] += v1.w * w1.w;
      }
    }
  }

  const int c = c0 + g * 8, ow = tx0 + col;
  if (c >= C || ow >= a.Wo) return;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int oh = ty0 + run * R + r;
    if (oh >= a.Ho) continue;
    const long long o = ((static_cast<long long>(b) * a.Ho + oh) * a.Wo + ow) * C + c;
    float res[8];
    if (a.res) load8v(a.res + o, oplane, split, res);
    float y[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      float v = acc[r][t] + (a.bias ? a.bias[c + t] : 0.f);
      v = dw_act(v, a.act, a.clip_lo, a.clip_hi);
      if (a.res) v += res[t];
      y[t] = v;
    }
    if (a.out) store8v(a.out + o, oplane, split, y);
    if (a.out_f32) {
#pragma unroll
      for (int t = 0; t < 8; ++t) a.out_f32[o + t] = y[t];
    }
  }
}

template <int K>
hipError_t launch_dwconv(const GConvArgs& a, hipStream_t s) {
  const int slices = (a.Cout + kDwSlice - 1) / kDwSlice;
  const int tiles_y = (a.Ho + kDwTH - 1) / kDwTH;
  if (a.Wo > 8) {
    const dim3 grid(static_cast<unsigned>(tiles_y * ((a.Wo + 15) / 16)), static_cast<unsigned>(slices), static_cast<unsigned>(a.B));
    hipLaunchKernelGGL((dwconv_kernel<K, 16>), grid, dim3(256), 0, s, a);
  } else {
    const dim3 grid(static_cast<unsigned>(tiles_y), static_cast<unsigned>(slices), static_cast<unsigned>(a.B));
    hipLaunchKernelGGL((dwconv_kernel<K, 8>), grid, dim3(128), 0, s, a);
  }
  return hipGetLastError();
}

}  // namespace

bool dwconv_tiled_supported(const GConvArgs& a) {
  return a.groups == a.Cin && a.groups == a.Cout && a.Cout % 8 == 0 && a.Cout >= 8 && a.stride == 1 && a.dil == 1 &&
         a.KH == a.KW && (a.KH == 5 || a.KH == 7);
}

hipError_t dwconv_tiled(const GConvArgs& a, hipStream_t s) {
  if (!dwconv_tiled_supported(a) || !a.w || !a.x || (!a.out && !a.out_f32) || a.B < 1 || a.B > 65535 || a.H < 1 ||
      a.W < 1 || a.Ho < 1 || a.Wo < 1 || a.pad_h < 0 || a.pad_w < 0 || a.Cout / kDwSlice >= 65535)
    return hipErrorInvalidValue;
  return a.KH == 5 ? launch_dwconv<5>(a, s) : launch_dwconv<7>(a, s);
}

}  // namespace kern
}  // namespace die
