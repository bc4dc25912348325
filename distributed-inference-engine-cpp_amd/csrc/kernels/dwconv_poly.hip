// Polyphase tiled depthwise convolution for gfx950 (NHWC), for the small and strided windows of the
// mobile families (MobileNetV2 / V3, EfficientNet(-Lite), MNASNet): depthwise only (groups == Cin ==
// Cout), dilation 1, (window, stride) in {(3x3, 1), (3x3, 2), (5x5, 2)}, any pads >= 0, C % 8 == 0,
// bf16 or split-fp32 planes, the epilogue of GConvArgs (bias, ReLU / Clip, residual, out / out_f32,
// the device-side live batch bound).  Stride-1 5x5 / 7x7 belong to dwconv.hip, the rest to gconv.hip.
//
// A block owns TH x TW output pixels of one sample times a slice of 32 channels.  It stages the input
// halo, HH x HW = ((TH-1)*S + K) x ((TW-1)*S + K) pixels, into LDS once (hi + lo joined to fp32,
// out-of-image pixels and channels past C as zeros) and the slice's K*K x 32 weights (fp32 [tap][C]
// in global memory) next to it.
//
// Polyphase columns.  At stride 2 the lane of output column `col` needs halo columns 2*col + kx.  A halo
// row is therefore stored de-interleaved: its even columns first (plane 0, PE = (HW + 1) / 2 pixels),
// then its odd columns (plane 1, HW / 2 pixels; HW = 2*TW + K - 2 is odd, so plane 1 is one pixel
// shorter and the row pitch is HW, with no padding).  Tap kx reads column col + kx / 2 of plane kx & 1:
// stored pixel index p = row * HW + (kx & 1) * PE + col + kx / 2.  At stride 1 there is one plane and
// p = row * HW + col + kx.
//
// LDS banks.  A pixel is 32 fp32 = 128 B = 8 slots of 16 B, laid out [half][channel group][4] as in
// dwconv.hip.  Lane l holds channel group l % 4 of column (l / 4) % TW and one vertical run.
// ds_read_b128 serves a wave in four groups of 16 lanes; each group is four channel groups of four
// columns that are distinct mod 4 and belong to one run (TW >= 8: a run is at least 32 lanes).  Within
// such a group and one tap, the row, the plane offset and kx / 2 are the same for all lanes, so p is
// the lane's column plus a constant: four values distinct mod 4 -- whatever the pitch HW and whichever
// plane, which is why the odd pitch and the shorter odd plane cost nothing.  Pixel p starts at slot
// 8 * (p & 1) of the 16-slot bank row, and its two halves are swapped where p & 2 is set, so the four
// pixels of a group start at slots 0, 4, 8 and 12: 16 lanes, 16 distinct slots, no conflict.  With raw
// columns 2*col + kx all four pixels would have the same parity and collide two by two.  The weight
// reads are four addresses per wave (broadcast).
//
// Input-stationary vertical window.  A thread keeps 8 channels of R vertically adjacent outputs of one
// column.  It walks the (R-1)*S + K input rows of its run from the top; each staged pixel is read
// once (two 16-byte reads) and applied to every output row r of the run with 0 <= ky = row - r*S < K:
// a 3x3 stride-1 run of 4 costs 6 x 3 pixel reads, not 36.  Every output still receives its taps in
// ascending (ky, kx) order with the expression gconv_kernel uses, and a zero halo adds exact zeros, so
// the result equals gconv_kernel<true> bit for bit.  3x3: the nine tap weights of the lane's 8
// channels stay in registers; 5x5: they are read from LDS where they are used.
//
// Tiles (static LDS, halo + weights):          wide, Wo > 8               narrow, Wo <= 8
//   3x3 s1   TH 8, R 4     10 x 18 px 23.6 KiB, 128 threads    10 x 10 px  13.6 KiB,  64 threads
//   3x3 s2   TH 4, R 2      9 x 33 px 38.3 KiB, 128 threads     9 x 17 px  20.3 KiB,  64 threads
//   5x5 s2   TH 4, R 2     11 x 35 px 51.3 KiB, 128 threads    11 x 19 px  29.3 KiB,  64 threads
// so at least three blocks fit in a CU's 160 KiB.  Partial tiles and a partial last slice are masked on
// the store.
#include "common.h"
#include "kernels.h"

namespace die {
namespace kern {

using namespace die::k;

namespace {

__device__ __forceinline__ float dwp_act(float v, int act, float lo, float hi) {
  if (act == 1) return fmaxf(v, 0.f);
  if (act == 3) return fminf(fmaxf(v, lo), hi);
  if (act == 4) return v * __builtin_amdgcn_rcpf(1.f + __expf(-v));             // SiLU
  if (act == 5) return v * fminf(fmaxf(fmaf(v, 1.f / 6.f, 0.5f), 0.f), 1.f);  // HardSwish
  return v;
}

__device__ __forceinline__ void dwp_fma8(float (&acc)[8], const float4& v0, const float4& v1, const float4& w0,
                                         const float4& w1) {
  acc[0] += v0.x * w0.x;
  acc[1] += v0.y * w0.y;
  acc[2] += v0.z * w0.z;
  acc[3] += v0.w * w0.w;
  acc[4] += v1.x * w1.x;
  acc[5] += v1.y * w1.y;
  acc[6] += v1.z * w1.z;
  acc[7] += v1.w * w1.w;
}

constexpr int kPolySlice = 32;  // channels of a block

template <int K, int S, int TW, int TH, int R>
__global__ __launch_bounds__(4 * TW * (TH / R), 3) void dwconv_poly_kernel(const GConvArgs a) {
  constexpr int HH = (TH - 1) * S + K, HW = (TW - 1) * S + K, RH = (R - 1) * S + K, NT = 4 * TW * (TH / R);
  constexpr int PE = S == 2 ? (HW + 1) / 2 : HW;  // pixels of plane 0 in a stored row
  constexpr bool WREG = K == 3;                   // tap weights in registers
  static_assert(S == 1 || S == 2, "one or two column phases");
  static_assert(TH % R == 0 && TW >= 8, "a 16-lane read group stays inside one run");
  static_assert(S == 1 || (TW - 1 + (K - 1) / 2 < PE && TW - 1 + (K - 2) / 2 < HW - PE), "taps stay inside their plane");
  static_assert((HH * HW * 8 + K * K * 8) * 16 <= 53 * 1024, "three blocks per CU");
  __shared__ float4 xs[HH * HW * 8];
  __shared__ float4 ws[K * K * 8];
  const int b = blockIdx.z;
  if (a.live && b >= *a.live) return;  // uniform over the block
  const int tiles_x = (a.Wo + TW - 1) / TW;
  const int ty0 = (blockIdx.x / tiles_x) * TH, tx0 = (blockIdx.x % tiles_x) * TW;
  const int c0 = blockIdx.y * kPolySlice;
  const int C = a.Cout;
  const bool split = a.split != 0;
  const long long xplane = static_cast<long long>(a.B) * a.H * a.W * C;
  const long long oplane = static_cast<long long>(a.B) * a.Ho * a.Wo * C;
  const uint16_t* xb = a.x + static_cast<long long>(b) * a.H * a.W * C;

#pragma unroll 4
  for (int i = threadIdx.x; i < HH * HW * 4; i += NT) {
    const int g = i & 3, hp = i >> 2, py = hp / HW, px = hp % HW;  // halo pixel (py, px)
    const int ih = ty0 * S - a.pad_h + py, iw = tx0 * S - a.pad_w + px, c = c0 + g * 8;
    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (ih >= 0 && ih < a.H && iw >= 0 && iw < a.W && c < C)
      load8v(xb + (static_cast<long long>(ih) * a.W + iw) * C + c, xplane, split, v);
    const int p = S == 2 ? py * HW + (px & 1) * PE + (px >> 1) : hp;  // de-interleaved by column parity
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
  float4 wr[WREG ? K * K : 1][2];
  if constexpr (WREG) {
#pragma unroll
    for (int tap = 0; tap < K * K; ++tap) {
      wr[tap][0] = ws[tap * 8 + g];
      wr[tap][1] = ws[tap * 8 + 4 + g];
    }
  }
  float acc[R][8];
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int t = 0; t < 8; ++t) acc[r][t] = 0.f;
  const int p0 = run * R * S * HW + col;  // the run's top row, the lane's column
#pragma unroll
  for (int j = 0; j < RH; ++j) {  // input rows of the run, top down
#pragma unroll
    for (int kx = 0; kx < K; ++kx) {
      const int p = p0 + j * HW + (S == 2 ? (kx & 1) * PE + (kx >> 1) : kx);
      const int s = (p >> 1) & 1;
      const float4 v0 = xs[p * 8 + s * 4 + g], v1 = xs[p * 8 + (s ^ 1) * 4 + g];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int ky = j - r * S;  // compile-time after unrolling
        if (ky < 0 || ky >= K) continue;
        if constexpr (WREG) {
          dwp_fma8(acc[r], v0, v1, wr[ky * K + kx][0], wr[ky * K + kx][1]);
        } else {
          const float4 w0 = ws[(ky * K + kx) * 8 + g], w1 = ws[(ky * K + kx) * 8 + 4 + g];
          dwp_fma8(acc[r], v0, v1, w0, w1);
        }
      }
    }
    // a row at a time: left alone, the compiler hoists every LDS read of the run ahead of the arithmetic
    // and keeps all 25 tap weights of a 5x5 live
    if constexpr (!WREG) asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
  }
  // the sums are needed here: without this the compiler sinks the whole accumulation into the masked
  // stores below and keeps every LDS read of the run alive until then (256 registers and scratch)
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int t = 0; t < 8; ++t) asm volatile("" : "+v"(acc[r][t]));

  const int c = c0 + g * 8, ow = tx0 + col;
  if (c >= C || ow >= a.Wo) return;
  float bs[8];
#pragma unroll
  for (int t = 0; t < 8; ++t) bs[t] = a.bias ? a.bias[c + t] : 0.f;
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
      float v = dwp_act(acc[r][t] + bs[t], a.act, a.clip_lo, a.clip_hi);
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

template <int K, int S, int TH, int R>
hipError_t launch_poly(const GConvArgs& a, hipStream_t s) {
  const unsigned slices = static_cast<unsigned>((a.Cout + kPolySlice - 1) / kPolySlice);
  const unsigned tiles_y = static_cast<unsigned>((a.Ho + TH - 1) / TH);
  if (a.Wo > 8) {
    const dim3 grid(tiles_y * static_cast<unsigned>((a.Wo + 15) / 16), slices, static_cast<unsigned>(a.B));
    hipLaunchKernelGGL((dwconv_poly_kernel<K, S, 16, TH, R>), grid, dim3(64 * (TH / R)), 0, s, a);
  } else {
    const dim3 grid(tiles_y, slices, static_cast<unsigned>(a.B));
    hipLaunchKernelGGL((dwconv_poly_kernel<K, S, 8, TH, R>), grid, dim3(32 * (TH / R)), 0, s, a);
  }
  return hipGetLastError();
}

}  // namespace

hipError_t dwconv_poly(const GConvArgs& a, hipStream_t s) {
  if (!dwconv_poly_supported(a) || !a.w || !a.x || (!a.out && !a.out_f32) || a.B < 1 || a.B > 65535 || a.H < 1 ||
      a.W < 1 || a.Ho < 1 || a.Wo < 1 || a.Cout / kPolySlice >= 65535)
    return hipErrorInvalidValue;
  if (a.KH == 5) return launch_poly<5, 2, 4, 2>(a, s);
  return a.stride == 1 ? launch_poly<3, 1, 8, 4>(a, s) : launch_poly<3, 2, 4, 2>(a, s);
}

}  // namespace kern
}  // namespace die
