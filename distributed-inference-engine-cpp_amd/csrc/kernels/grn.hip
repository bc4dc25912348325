// Global Response Normalization (ConvNeXt-V2) of an NHWC map for gfx950 (kernels.h GrnArgs): x [B][HW][C]
// bf16 or split planes, per sample
//   G[c] = sqrt(sum_p x[p][c]^2),  a[c] = 1 + gamma[c] * G[c] / (mean_c G + eps),  y = x * a[c] + beta[c]
// which is the exported gamma * (x * nx) + beta + x with the trailing "+ x" folded into the coefficient.
//
// The C / 8 16-byte chunks of a pixel are cut into `nt` column tiles of `tw` <= 256 chunks (any C: 11264
// channels are 6 tiles of 235), and thread t of a block holds the 8 channels of chunk tile * tw + t % tw
// and walks the pixels r, r + R, ... of its block (r = t / tw, R = 256 / tw pixel rows per pass;
// consecutive lanes read consecutive 16 bytes).  Which form runs depends on (HW, C) alone
// (grn_geometry), never on the batch:
//  * one launch (grn_fused_kernel, grid (1, 1, B)) where a sample has at most kGrnFusedChunks 16-byte
//    chunks and at most 4096 channels: one block takes the whole sample, tile by tile, keeps G and then a
//    in LDS, and reads x a second time (from the L2) to apply them.  Measured against the three launches
//    on maps of 32 and 128 chunks per pixel at B = 1, 8 and 32 (us per call, fp32 / bf16 storage; B changes
//    neither by more than 0.7): 5.7 - 6.2 against 8.4 - 9.5 at 256 chunks per sample, 8.0 - 8.5 / 6.9 - 7.4
//    against 10.9 - 11.8 / 9.7 - 10.5 at 1024, 11.0 - 11.7 / 8.8 - 9.4 against 11.7 - 12.8 / 10.5 - 11.6 at
//    2048, and slower from 4096 on (16.8 - 18.1 / 12.6 - 13.3 against 12.1 - 13.6 / 11.0 - 12.3; 7 x 7 x 3072
//    takes 76 against 16): one block per sample streams too little.  Hence the bound of 2048.
//  * three launches otherwise:
//  1. grn_sumsq_kernel, grid (nblk, nt, B): a block owns `ppb` consecutive pixels of one column tile of
//     one sample.  A thread accumulates the squares of the joined values of its 8 channels in fp32, the R
//     threads of a chunk are merged by a tree in LDS (row r takes row r + s, fixed pairing), and row 0
//     writes the block's sums: ws[b][blk][c].
//  2. grn_coef_kernel, grid (1, B), 1024 threads: thread t takes channels t, t + 1024, ...: adds the nblk
//     partials of a channel in block order, G = sqrt of it; the threads' sums of G (channel order) are
//     merged by a tree in LDS into the mean; a[c] goes to ws[b][nblk][c].  One block per sample, because
//     the mean needs every channel; its loads are the launch's serial part, hence the 1024 threads.
//  3. grn_apply_kernel, the grid and thread layout of 1: a thread loads its chunk's a and beta once and
//     the inner loop is one FMA per value between a 16-byte load and a 16-byte store.
// Every order above depends on (HW, C) only, nothing is accumulated by atomics and a block never reads
// another sample: a sample's bits do not depend on B, on its place in the batch or on *live.  Blocks of
// samples >= *live return at once.  out may be x: in the three-launch form every read of the statistics
// pass is over before the apply pass starts, in the one-launch form the block that writes a sample is the
// only one that reads it and has passed a barrier behind its last statistics read.
// ppb gives every thread at least 4 pixels and a sample at most 64 blocks per column tile, which bounds
// the coefficient kernel's reads (64 * C floats per sample).
// LDS: 8 KiB of the merge tree (+ 1 KiB and the 16 KiB of coefficients in the one-launch form), 4 KiB in the
// coefficient kernel.  Measurements: tools/grn_bench.py, profiles/convnextv2.md.
#include "common.h"
#include "kernels.h"

namespace die {
namespace kern {

using namespace die::k;

namespace {

constexpr int kGrnThreads = 256;
constexpr int kGrnMaxBlocks = 64;     // statistics blocks per (sample, column tile)
constexpr int kGrnRowsPerThread = 4;
constexpr int kGrnCoefThreads = 1024;
constexpr int kGrnFusedMaxC = 4096;   // the fused form keeps a sample's coefficients in 16 KiB of LDS
// 16-byte chunks of a sample (HW * C / 8) up to which one block takes it whole
constexpr int kGrnFusedChunks = 2048;

struct GrnGeom {
  int cv, nt, tw, R, ppb, nblk, fused;
};

// Depends on (HW, C) only: the merge order of a sample's sums must not change with the batch.
GrnGeom grn_geometry(int HW, int C, int form) {
  GrnGeom g;
  g.cv = C / 8;
  g.nt = (g.cv + kGrnThreads - 1) / kGrnThreads;
  g.tw = (g.cv + g.nt - 1) / g.nt;
  g.R = kGrnThreads / g.tw;
  const bool can_fuse = C <= kGrnFusedMaxC;
  g.fused = form == 1 ? can_fuse : form == 2 ? 0 : can_fuse && static_cast<long long>(HW) * g.cv <= kGrnFusedChunks;
  const int want = std::max(g.R * kGrnRowsPerThread, (HW + kGrnMaxBlocks - 1) / kGrnMaxBlocks);
  g.ppb = (want + g.R - 1) / g.R * g.R;
  g.nblk = g.fused ? 1 : (HW + g.ppb - 1) / g.ppb;
  return g;
}

// The sums of squares of one thread: pixels p0 + r, p0 + r + R, ... < p1 of the 8 channels at xb
__device__ __forceinline__ void grn_sumsq(const uint16_t* xb, const int C, const long long plane, const bool split,
                                          const int r, const int R, const int p0, const int p1, float* acc) {
#pragma unroll
  for (int t = 0; t < 8; ++t) acc[t] = 0.f;
  for (int p = p0 + r; p < p1; p += R) {
    float v[8];
    load8v(xb + static_cast<long long>(p) * C, plane, split, v);
#pragma unroll
    for (int t = 0; t < 8; ++t) acc[t] = fmaf(v[t], v[t], acc[t]);
  }
}

// Tree over the R pixel rows of a chunk in sm[8][256]: row r takes row r + s.  A row < s is read by
// nobody in its step, so it writes its own slot back at once: one barrier per step.  Every thread of
// the block calls it; the sums of a chunk end in its row-0 thread's acc.
__device__ __forceinline__ void grn_tree(float (*sm)[kGrnThreads], const int tid, const int r, const int R, const int tw,
                                         const bool on, float* acc) {
#pragma unroll
  for (int t = 0; t < 8; ++t) sm[t][tid] = acc[t];
  __syncthreads();
  int s = 1;
  while (s < R) s <<= 1;
  for (s >>= 1; s >= 1; s >>= 1) {
    if (on && r < s && r + s < R) {
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        acc[t] += sm[t][tid + s * tw];
        sm[t][tid] = acc[t];
      }
    }
    __syncthreads();
  }
}

// The apply pass of one thread with its chunk's coefficients at a8 (global memory or LDS)
__device__ __forceinline__ void grn_apply(const GrnArgs& a, const float* a8, const int b, const int jc, const int r,
                                          const int R, const int p0, const int p1) {
  float sc[8], sh[8];
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    sc[t] = a8[t];
    sh[t] = a.beta ? a.beta[jc * 8 + t] : 0.f;
  }
  const long long plane = static_cast<long long>(a.B) * a.HW * a.C;
  const long long off = static_cast<long long>(b) * a.HW * a.C + jc * 8;
  for (int p = p0 + r; p < p1; p += R) {
    const long long o = off + static_cast<long long>(p) * a.C;
    float v[8], y[8];
    load8v(a.x + o, plane, a.split != 0, v);
#pragma unroll
    for (int t = 0; t < 8; ++t) y[t] = fmaf(v[t], sc[t], sh[t]);
    store8v(a.out + o, plane, a.split != 0, y);
  }
}

// The sum over the block's T threads of v, in a fixed tree; every thread gets it.  red[T] in LDS.
template <int T>
__device__ __forceinline__ float grn_block_sum(float* red, const int tid, float v) {
  red[tid] = v;
  __syncthreads();
  for (int s = T / 2; s >= 1; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  return red[0];
}

__global__ __launch_bounds__(kGrnThreads) void grn_sumsq_kernel(const GrnArgs a, const GrnGeom gm) {
  __shared__ float sm[8][kGrnThreads];
  const int b = blockIdx.z;
  if (a.live && b >= *a.live) return;  // uniform over the block
  const int blk = blockIdx.x, tid = threadIdx.x;
  const int j = tid % gm.tw, r = tid / gm.tw, jc = blockIdx.y * gm.tw + j;
  const bool on = r < gm.R && jc < gm.cv;
  const int p0 = blk * gm.ppb, p1 = min(a.HW, p0 + gm.ppb);
  const long long plane = static_cast<long long>(a.B) * a.HW * a.C;
  float acc[8];
  if (on) {
    grn_sumsq(a.x + static_cast<long long>(b) * a.HW * a.C + jc * 8, a.C, plane, a.split != 0, r, gm.R, p0, p1, acc);
  } else {
#pragma unroll
    for (int t = 0; t < 8; ++t) acc[t] = 0.f;
  }
  grn_tree(sm, tid, r, gm.R, gm.tw, on, acc);
  if (on && r == 0) {
    float4* dst = reinterpret_cast<float4*>(a.ws + (static_cast<size_t>(b) * (gm.nblk + 1) + blk) * a.C + jc * 8);
    dst[0] = make_float4(acc[0], acc[1], acc[2], acc[3]);
    dst[1] = make_float4(acc[4], acc[5], acc[6], acc[7]);
  }
}

__global__ __launch_bounds__(kGrnCoefThreads) void grn_coef_kernel(const GrnArgs a, const GrnGeom gm) {
  __shared__ float red[kGrnCoefThreads];
  const int b = blockIdx.y;
  if (a.live && b >= *a.live) return;
  const int tid = threadIdx.x;
  const float* part = a.ws + static_cast<size_t>(b) * (gm.nblk + 1) * a.C;
  float* coef = a.ws + (static_cast<size_t>(b) * (gm.nblk + 1) + gm.nblk) * a.C;
  float gsum = 0.f;
  for (int c = tid; c < a.C; c += kGrnCoefThreads) {
    float s = 0.f;
#pragma unroll 8
    for (int blk = 0; blk < gm.nblk; ++blk) s += part[static_cast<size_t>(blk) * a.C + c];
    const float g = sqrtf(s);
    coef[c] = g;  // read back below by the thread that wrote it
    gsum += g;
  }
  const float inv = 1.f / (grn_block_sum<kGrnCoefThreads>(red, tid, gsum) / static_cast<float>(a.C) + a.eps);
  for (int c = tid; c < a.C; c += kGrnCoefThreads) coef[c] = a.gamma ? fmaf(a.gamma[c], coef[c] * inv, 1.f) : 1.f;
}

__global__ __launch_bounds__(kGrnThreads) void grn_apply_kernel(const GrnArgs a, const GrnGeom gm) {
  const int b = blockIdx.z;
  if (a.live && b >= *a.live) return;
  const int j = threadIdx.x % gm.tw, r = threadIdx.x / gm.tw, jc = blockIdx.y * gm.tw + j;
  if (r >= gm.R || jc >= gm.cv) return;
  const int p0 = blockIdx.x * gm.ppb, p1 = min(a.HW, p0 + gm.ppb);
  const float* coef = a.ws + (static_cast<size_t>(b) * (gm.nblk + 1) + gm.nblk) * a.C;
  grn_apply(a, coef + jc * 8, b, jc, r, gm.R, p0, p1);
}

// The one-launch form, grid (1, 1, B): the block owns the whole sample.
__global__ __launch_bounds__(kGrnThreads) void grn_fused_kernel(const GrnArgs a, const GrnGeom gm) {
  __shared__ float sm[8][kGrnThreads];
  __shared__ float red[kGrnThreads];
  __shared__ float coef[kGrnFusedMaxC];
  const int b = blockIdx.z;
  if (a.live && b >= *a.live) return;
  const int tid = threadIdx.x;
  const int j = tid % gm.tw, r = tid / gm.tw;
  const long long plane = static_cast<long long>(a.B) * a.HW * a.C;
  for (int tile = 0; tile < gm.nt; ++tile) {  // uniform trip count: the tree's barriers are reached by all
    const int jc = tile * gm.tw + j;
    const bool on = r < gm.R && jc < gm.cv;
    float acc[8];
    if (on) {
      grn_sumsq(a.x + static_cast<long long>(b) * a.HW * a.C + jc * 8, a.C, plane, a.split != 0, r, gm.R, 0, a.HW, acc);
    } else {
#pragma unroll
      for (int t = 0; t < 8; ++t) acc[t] = 0.f;
    }
    grn_tree(sm, tid, r, gm.R, gm.tw, on, acc);
    if (on && r == 0) {
#pragma unroll
      for (int t = 0; t < 8; ++t) coef[jc * 8 + t] = sqrtf(acc[t]);
    }
    __syncthreads();  // sm is written again by the next tile
  }
  float gsum = 0.f;
  for (int c = tid; c < a.C; c += kGrnThreads) gsum += coef[c];
  const float inv = 1.f / (grn_block_sum<kGrnThreads>(red, tid, gsum) / static_cast<float>(a.C) + a.eps);
  for (int c = tid; c < a.C; c += kGrnThreads) coef[c] = a.gamma ? fmaf(a.gamma[c], coef[c] * inv, 1.f) : 1.f;
  __syncthreads();
  for (int tile = 0; tile < gm.nt; ++tile) {
    const int jc = tile * gm.tw + j;
    if (r < gm.R && jc < gm.cv) grn_apply(a, coef + jc * 8, b, jc, r, gm.R, 0, a.HW);
  }
}

bool aligned(const void* p, uintptr_t n) { return reinterpret_cast<uintptr_t>(p) % n == 0; }

}  // namespace

size_t grn_workspace_bytes(int B, int HW, int C) {
  if (B < 1 || HW < 1 || C < 8 || C % 8) return 0;
  // the three-launch geometry's size also where the fused form runs: a forced form (GrnArgs::form) fits
  const GrnGeom g = grn_geometry(HW, C, 2);
  return static_cast<size_t>(B) * (g.nblk + 1) * C * sizeof(float);
}

hipError_t grn(const GrnArgs& a, hipStream_t s) {
  if (!a.x || !a.out || a.B < 1 || a.B > 65535 || a.HW < 1 || a.C < 8 || a.C % 8 || !(a.eps >= 0.f) || a.form < 0 || a.form > 2)
    return hipErrorInvalidValue;
  if (static_cast<long long>(a.HW) * a.C > 0x7fffffffLL) return hipErrorInvalidValue;  // a sample's offsets are ints
  if (!aligned(a.x, 16) || !aligned(a.out, 16) || !aligned(a.gamma, 4) || !aligned(a.beta, 4) || !aligned(a.ws, 16))
    return hipErrorInvalidValue;
  const size_t need = grn_workspace_bytes(a.B, a.HW, a.C);
  if (!a.ws || need == 0 || a.ws_bytes < need) return hipErrorInvalidValue;
  const GrnGeom gm = grn_geometry(a.HW, a.C, a.form);
  if (gm.fused) {
    hipLaunchKernelGGL(grn_fused_kernel, dim3(1, 1, static_cast<unsigned>(a.B)), dim3(kGrnThreads), 0, s, a, gm);
    return hipGetLastError();
  }
  const dim3 grid(static_cast<unsigned>(gm.nblk), static_cast<unsigned>(gm.nt), static_cast<unsigned>(a.B));
  hipLaunchKernelGGL(grn_sumsq_kernel, grid, dim3(kGrnThreads), 0, s, a, gm);
  hipLaunchKernelGGL(grn_coef_kernel, dim3(1, static_cast<unsigned>(a.B)), dim3(kGrnCoefThreads), 0, s, a, gm);
  hipLaunchKernelGGL(grn_apply_kernel, grid, dim3(kGrnThreads), 0, s, a, gm);
  return hipGetLastError();
}

}  // namespace kern
}  // namespace die
