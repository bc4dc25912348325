// Squeeze-excitation block of an NHWC map for gfx950 (kernels.h SeArgs): x [B][HW][C] bf16 or split planes,
//   g = act2(W2 act1(W1 mean_p(x) + b1) + b2),  y = x * g[c]
// in two launches: one pass over x for the pool with both FCs behind it in the same kernel, one pass for
// the scale.  The gate is fp32 from the stored x to the multiply (the unfused chain rounds the pooled
// vector, the hidden vector and the gate to the activation storage between its six or seven launches).
//
// Column layout (both kernels, grn.hip's): the C / 8 16-byte chunks of a pixel are cut into `nt` column
// tiles of `tw` <= 256 chunks; thread t holds the 8 channels of chunk tile * tw + t % tw and walks the
// pixels r, r + R, ... of its range (r = t / tw, R = 256 / tw): consecutive lanes read consecutive 16 bytes.
//
// 1. se_gate_kernel, grid (P, B): block (p, b) owns pixel slice p of sample b and loops over the column
//    tiles.  A thread sums its pixels in fp32 (split mode: the joined hi + lo), the R threads of a chunk
//    are merged by a tree in LDS (row r takes row r + s: a fixed pairing), and row 0 has the slice's sums.
//    P == 1: they go, times 1 / HW, straight into the pooled vector in LDS.  P > 1: they go to
//    ws[b][p][C]; every thread fences its stores, one lane takes the sample's ticket (agent-scope
//    fetch-add on counters[b] behind a release fence), and the block that draws the last ticket resets
//    the counter, acquires, and adds the P partials of every channel in slice order -- the same bits
//    whichever block comes last.  The other blocks are gone by then: nobody spins, no grid-wide sync.
//    The last block then runs the FCs on the pooled vector in LDS (16 KiB):
//     FC1: wave w takes rows w, w + 4, ...; its lanes stride over C (coalesced reads of w1), a butterfly
//          over the 64 lanes, + b1, act1; the hidden vector stays in LDS (4 KiB).
//     FC2: thread t takes channels t, t + 256, ...: reads w2t row by row (consecutive lanes, consecutive
//          channels -- hence the transposed weight), + b2, act2, g[b][c] in f32.
// 2. se_scale_kernel, grid (pixel blocks, nt, B): a thread loads its chunk's eight gate values once and
//    walks its pixels: 16-byte load, join, 8 multiplies, re-split, 16-byte store.
// Blocks of samples >= *live return at once (before any barrier).  out may be x: the gate kernel has read
// all of x when the scale kernel starts.  No MFMA: the FCs are M = 1 per sample, a few thousand MACs.
// LDS of the gate kernel: 8 KiB merge tree + 16 KiB pooled + 4 KiB hidden.
#include "common.h"
#include "kernels.h"

namespace die {
namespace kern {

using namespace die::k;

namespace {

constexpr int kSeThreads = 256;
constexpr int kSeMaxC = 4096;
constexpr int kSeMaxCr = 1024;
constexpr int kSeRowsPerThread = 4;  // pixels a thread of the scale kernel walks

struct SeGeom {
  int cv, nt, tw, R;
  int P, pps;     // gate kernel: slices of a sample, pixels per slice
  int ppb, nblk;  // scale kernel: pixels per block, blocks per (sample, column tile)
};

SeGeom se_geometry(int B, int HW, int C, int slices) {
  SeGeom g;
  g.cv = C / 8;
  g.nt = (g.cv + kSeThreads - 1) / kSeThreads;
  g.tw = (g.cv + g.nt - 1) / g.nt;
  g.R = kSeThreads / g.tw;
  const int want = std::max(1, std::min(std::min(slices > 0 ? slices : se_slices(B, HW), HW), kSeMaxSlices));
  g.pps = (HW + want - 1) / want;
  g.P = (HW + g.pps - 1) / g.pps;  // no empty slice
  g.ppb = g.R * kSeRowsPerThread;
  g.nblk = (HW + g.ppb - 1) / g.ppb;
  return g;
}

__device__ __forceinline__ float se_sigmoid(float v) { return __builtin_amdgcn_rcpf(1.f + __expf(-v)); }

__device__ __forceinline__ float se_act1(float v, int act) {
  if (act == 4) return v * se_sigmoid(v);
  if (act == 5) return v * fminf(fmaxf(fmaf(v, 1.f / 6.f, 0.5f), 0.f), 1.f);
  return fmaxf(v, 0.f);
}

__device__ __forceinline__ float se_act2(float v, int act, float alpha, float beta) {
  return act == 1 ? fminf(fmaxf(fmaf(alpha, v, beta), 0.f), 1.f) : se_sigmoid(v);
}

__global__ __launch_bounds__(kSeThreads) void se_gate_kernel(const SeArgs a, const SeGeom gm) {
  __shared__ float sm[8][kSeThreads];
  __shared__ float pooled[kSeMaxC];
  __shared__ float hidden[kSeMaxCr];
  __shared__ int last;
  const int b = blockIdx.y;
  if (a.live && b >= *a.live) return;  // uniform over the block (and over the sample's blocks)
  const int p = blockIdx.x, tid = threadIdx.x;
  const int j = tid % gm.tw, r = tid / gm.tw;
  const int p0 = p * gm.pps, p1 = min(a.HW, p0 + gm.pps);
  const long long plane = static_cast<long long>(a.B) * a.HW * a.C;
  const uint16_t* xs = a.x + static_cast<long long>(b) * a.HW * a.C;
  const float inv_hw = 1.f / static_cast<float>(a.HW);
  float* part = gm.P > 1 ? a.ws + (static_cast<size_t>(b) * gm.P + p) * a.C : nullptr;

  for (int tile = 0; tile < gm.nt; ++tile) {  // uniform trip count: every thread reaches the barriers
    const int jc = tile * gm.tw + j;
    const bool on = r < gm.R && jc < gm.cv;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (on) {
#pragma unroll 4
      for (int q = p0 + r; q < p1; q += gm.R) {
        float v[8];
        load8v(xs + static_cast<long long>(q) * a.C + jc * 8, plane, a.split != 0, v);
#pragma unroll
        for (int t = 0; t < 8; ++t) acc[t] += v[t];
      }
    }
#pragma unroll
    for (int t = 0; t < 8; ++t) sm[t][tid] = acc[t];
    __syncthreads();
    int s = 1;
    while (s < gm.R) s <<= 1;
    for (s >>= 1; s >= 1; s >>= 1) {  // row r takes row r + s; a row < s is read by nobody in its step
      if (on && r < s && r + s < gm.R) {
#pragma unroll
        for (int t = 0; t < 8; ++t) {
          acc[t] += sm[t][tid + s * gm.tw];
          sm[t][tid] = acc[t];
        }
      }
      __syncthreads();
    }
    if (on && r == 0) {
      if (part) {
        float4* dst = reinterpret_cast<float4*>(part + jc * 8);
        dst[0] = make_float4(acc[0], acc[1], acc[2], acc[3]);
        dst[1] = make_float4(acc[4], acc[5], acc[6], acc[7]);
      } else {
#pragma unroll
        for (int t = 0; t < 8; ++t) pooled[jc * 8 + t] = acc[t] * inv_hw;
      }
    }
  }

  if (part) {
    // hand-off: the partials are out before the ticket is drawn; the last block reads them behind an acquire
    __threadfence();
    __syncthreads();
    if (tid == 0) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      const int prev = __hip_atomic_fetch_add(a.counters + b, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const int is_last = prev == gm.P - 1;
      if (is_last) __hip_atomic_store(a.counters + b, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // ready for the next launch
      last = is_last;
    }
    __syncthreads();
    if (!last) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    const float* all = a.ws + static_cast<size_t>(b) * gm.P * a.C;
    for (int c = tid; c < a.C; c += kSeThreads) {
      float s = 0.f;
      for (int q = 0; q < gm.P; ++q) s += all[static_cast<size_t>(q) * a.C + c];  // slice order
      pooled[c] = s * inv_hw;
    }
  }
  __syncthreads();

  const int wave = tid >> 6, lane = tid & 63;
  for (int row = wave; row < a.Cr; row += kSeThreads / 64) {
    const float* w = a.w1 + static_cast<size_t>(row) * a.C;
    float s = 0.f;
    for (int c = lane; c < a.C; c += 64) s = fmaf(w[c], pooled[c], s);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
    if (lane == 0) hidden[row] = se_act1(s + (a.b1 ? a.b1[row] : 0.f), a.act1);
  }
  __syncthreads();
  for (int c = tid; c < a.C; c += kSeThreads) {
    float s = 0.f;
#pragma unroll 4
    for (int row = 0; row < a.Cr; ++row) s = fmaf(a.w2t[static_cast<size_t>(row) * a.C + c], hidden[row], s);
    a.gate[static_cast<size_t>(b) * a.C + c] = se_act2(s + (a.b2 ? a.b2[c] : 0.f), a.act2, a.alpha, a.beta);
  }
}

__global__ __launch_bounds__(kSeThreads) void se_scale_kernel(const SeArgs a, const SeGeom gm) {
  const int b = blockIdx.z;
  if (a.live && b >= *a.live) return;
  const int j = threadIdx.x % gm.tw, r = threadIdx.x / gm.tw, jc = blockIdx.y * gm.tw + j;
  if (r >= gm.R || jc >= gm.cv) return;
  const int p0 = blockIdx.x * gm.ppb, p1 = min(a.HW, p0 + gm.ppb);
  const float4* gp = reinterpret_cast<const float4*>(a.gate + static_cast<size_t>(b) * a.C + jc * 8);
  const float4 g0 = gp[0], g1 = gp[1];
  const float g[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
  const long long plane = static_cast<long long>(a.B) * a.HW * a.C;
  const long long off = static_cast<long long>(b) * a.HW * a.C + jc * 8;
#pragma unroll
  for (int q = 0; q < kSeRowsPerThread; ++q) {
    const int px = p0 + r + q * gm.R;
    if (px >= p1) break;
    const long long o = off + static_cast<long long>(px) * a.C;
    float v[8];
    load8v(a.x + o, plane, a.split != 0, v);
#pragma unroll
    for (int t = 0; t < 8; ++t) v[t] *= g[t];
    store8v(a.out + o, plane, a.split != 0, v);
  }
}

bool aligned(const void* p, uintptr_t n) { return reinterpret_cast<uintptr_t>(p) % n == 0; }

}  // namespace

hipError_t se_block(const SeArgs& a, hipStream_t s) {
  if (!a.x || !a.out || !a.w1 || !a.w2t || !a.gate || a.B < 1 || a.B > 65535 || a.HW < 1 || a.C < 8 || a.C > kSeMaxC ||
      a.C % 8 || a.Cr < 1 || a.Cr > kSeMaxCr || a.slices < 0)
    return hipErrorInvalidValue;
  if (!(a.act1 == 1 || a.act1 == 4 || a.act1 == 5) || a.act2 < 0 || a.act2 > 1) return hipErrorInvalidValue;
  if (static_cast<long long>(a.HW) * a.C > 0x7fffffffLL) return hipErrorInvalidValue;  // a sample's offsets are ints
  if (!aligned(a.x, 16) || !aligned(a.out, 16) || !aligned(a.gate, 16) || !aligned(a.ws, 16) || !aligned(a.w1, 4) ||
      !aligned(a.w2t, 4) || !aligned(a.b1, 4) || !aligned(a.b2, 4) || !aligned(a.counters, 4))
    return hipErrorInvalidValue;
  const SeGeom gm = se_geometry(a.B, a.HW, a.C, a.slices);
  if (gm.P > 1 && (!a.ws || a.ws_bytes < se_workspace_bytes(a.B, gm.P, a.C) || !a.counters || a.counters_n < a.B))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(se_gate_kernel, dim3(static_cast<unsigned>(gm.P), static_cast<unsigned>(a.B)), dim3(kSeThreads), 0, s, a, gm);
  hipLaunchKernelGGL(se_scale_kernel, dim3(static_cast<unsigned>(gm.nblk), static_cast<unsigned>(gm.nt), static_cast<unsigned>(a.B)),
                     dim3(kSeThreads), 0, s, a, gm);
  return hipGetLastError();
}

}  // namespace kern
}  // namespace die
