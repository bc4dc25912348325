// GroupNorm / InstanceNorm of an NHWC image for gfx950 (kernels.h GroupNormArgs): x [B][HW][C] bf16 or
// split planes, G groups of Cg = Cl / G consecutive logical channels, any Cg >= 1.
//
// Which form runs depends on (HW, C) alone (gn_geometry), never on the batch:
//  * one launch (gn_stats_kernel<true>, grid (1, B)) where a sample has at most 1024 16-byte chunks
//    (HW * C / 8: 4 per thread -- an 8 x 8 x 96 or 16 x 16 x 32 map): one block takes the whole sample,
//    so every (sample, group) fits it.  Steps 1 and 3 below in one kernel, the groups' (mean, rstd) in
//    LDS between them; the second read of x is served by the L2.  Measured per op inside gn_resnet at
//    B = 8 against the three launches: 16 us against 21 - 26 at 768 - 1024 chunks, equal at 2048, slower
//    from 3072 on (one block per sample streams too little): hence the bound.
//  * three launches otherwise:
//  1. gn_stats_kernel<false>, grid (nblk, B): a block owns `ppb` consecutive pixels of one sample and ALL
//     C channels.  Thread t holds the 8 channels of 16-byte chunk j = t % (C / 8) and walks the pixels
//     r, r + R, ... of the block (r = t / (C / 8), R = 256 / (C / 8) pixel rows per pass; consecutive
//     lanes read consecutive 16 bytes).  Per CHANNEL it keeps (count, mean, M2) by Welford's update, so
//     a chunk that straddles two groups needs no special case.  The R threads of a chunk are merged by
//     a tree in LDS (Chan et al., fixed pairing), then one thread per group merges the group's Cg
//     channels in channel order and writes the block's (mean, M2) of the group: ws[b][blk][g].  The
//     count is (pixels of the block) * Cg, known from the geometry.
//  2. gn_merge_kernel: L = min(64, nblk rounded up to a power of two) lanes per group merge the nblk
//     partials -- lane l takes blocks l, l + L, ... in order, then a shuffle tree -- into (mean, rstd) of
//     the group: ws[b][nblk * G + g].
//  3. gn_apply_kernel, grid (nblk, B), the same thread layout: a thread folds its 8 channels'
//     (mean, rstd, gamma, beta) into (mean, a = rstd * gamma, beta) once and the inner loop is
//     y = act((x - mean) * a + beta): one subtract and one FMA.  Folding the mean in as well
//     (b = beta - mean * a) would leave the rounding of mean * a, up to 2^-24 |mean| rstd, in every
//     output: the whole error where the variance is tiny (a 1x1 map with G = C must give act(beta)
//     exactly) and visible for a map with a large mean.
// The geometry (R, ppb, nblk) depends on (HW, C) only and every merge order on (HW, C, G) only, nothing
// is accumulated by atomics, and a block never reads another sample: a sample's bits do not depend on B,
// on its place in the batch or on *live.  Blocks of samples >= *live return at once.
// In the three-launch form ppb gives every thread two pixels and at most 256 blocks per sample: 128
// blocks for one 64 x 64 x 128 map.  LDS: the 17 KiB of the merge tree, + 16 KiB of group statistics in
// the one-launch form.  Measurements: profiles/groupnorm.md.
#include "common.h"
#include "kernels.h"

namespace die {
namespace kern {

using namespace die::k;

namespace {

constexpr int kGnThreads = 256;
constexpr int kGnMaxC = 2048;       // one 16-byte chunk per thread: C / 8 <= 256
constexpr int kGnMaxBlocks = 256;   // statistics blocks per sample
constexpr int kGnRowsPerThread = 2;
constexpr int kGnFusedChunks = 1024;  // 16-byte chunks of a sample (4 per thread) up to which one block takes it whole

struct GnGeom {
  int cv, R, ppb, nblk;  // nblk == 1: the one-launch form
};

// Depends on (HW, C) only: the merge order of a sample's statistics must not change with the batch.
GnGeom gn_geometry(int HW, int C) {
  GnGeom g;
  g.cv = C / 8;
  g.R = kGnThreads / g.cv;
  const int want = std::max(g.R * kGnRowsPerThread, (HW + kGnMaxBlocks - 1) / kGnMaxBlocks);
  g.ppb = (want + g.R - 1) / g.R * g.R;
  if (static_cast<long long>(HW) * g.cv <= kGnFusedChunks) g.ppb = (HW + g.R - 1) / g.R * g.R;  // one block: the fused form
  g.nblk = (HW + g.ppb - 1) / g.ppb;
  return g;
}

// Floats of workspace per sample: the blocks' partials [nblk][G] float2, then (mean, rstd) [G] float2.
size_t gn_ws_floats(const GnGeom& g, int G) { return (static_cast<size_t>(g.nblk) + 1) * G * 2; }

// (count, mean, M2) a <- a merged with b (Chan et al.); an empty side leaves the other as it is.
__device__ __forceinline__ void chan_merge(float& na, float& ma, float& qa, float nb, float mb, float qb) {
  if (nb == 0.f) return;
  if (na == 0.f) {
    na = nb;
    ma = mb;
    qa = qb;
    return;
  }
  const float n = na + nb, d = mb - ma, f = nb / n;
  ma = fmaf(d, f, ma);
  qa = (qa + qb) + d * d * (na * f);
  na = n;
}

__device__ __forceinline__ float gn_act(float v, int act) {
  if (act == 1) return fmaxf(v, 0.f);
  if (act == 2) return v * __builtin_amdgcn_rcpf(1.f + __expf(-v));
  return v;
}

// The apply pass of one thread: pixels p0 + r, p0 + r + R, ... < p1 of sample b, the 8 channels of chunk j,
// with the groups' (mean, rstd) at st[g] (global memory or LDS).
template <typename Stats>
__device__ __forceinline__ void gn_apply(const GroupNormArgs& a, const int Cl, const Stats st, const int b, const int j,
                                         const int r, const int R, const int p0, const int p1) {
  const int Cg = Cl / a.G;
  float mu[8], sc[8], sh[8];
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    const int c = j * 8 + t;
    mu[t] = sc[t] = sh[t] = 0.f;
    if (c < Cl) {
      const float2 ms = st[c / Cg];
      mu[t] = ms.x;
      sc[t] = a.gamma ? ms.y * a.gamma[c] : ms.y;
      sh[t] = a.beta ? a.beta[c] : 0.f;
    }
  }
  const long long plane = static_cast<long long>(a.B) * a.HW * a.C;
  const long long off = static_cast<long long>(b) * a.HW * a.C + j * 8;
  for (int p = p0 + r; p < p1; p += R) {
    const long long o = off + static_cast<long long>(p) * a.C;
    float v[8], y[8];
    load8v(a.x + o, plane, a.split != 0, v);
#pragma unroll
    for (int t = 0; t < 8; ++t) y[t] = j * 8 + t < Cl ? gn_act(fmaf(v[t] - mu[t], sc[t], sh[t]), a.act) : 0.f;
    store8v(a.out + o, plane, a.split != 0, y);
  }
}

// FUSED: the one-launch form, grid (1, B) -- the block owns the whole sample (gm.ppb >= HW), keeps the
// groups' (mean, rstd) in LDS and applies them itself.
template <bool FUSED>
__global__ __launch_bounds__(kGnThreads) void gn_stats_kernel(const GroupNormArgs a, const GnGeom gm, const int Cl) {
  __shared__ float sm[17][kGnThreads];  // [0] count, [1..8] mean, [9..16] M2 of a thread's 8 channels
  __shared__ float2 sstat[FUSED ? kGnMaxC : 1];  // FUSED: (mean, rstd) of the groups (G <= C)
  const int b = blockIdx.y;
  if (a.live && b >= *a.live) return;  // uniform over the block
  const int blk = blockIdx.x, tid = threadIdx.x;
  const int cv = gm.cv, R = gm.R;
  const int j = tid % cv, r = tid / cv;
  const int p0 = blk * gm.ppb, p1 = min(a.HW, p0 + gm.ppb);
  const long long plane = static_cast<long long>(a.B) * a.HW * a.C;
  const uint16_t* xb = a.x + static_cast<long long>(b) * a.HW * a.C + j * 8;

  float n = 0.f, mu[8], m2[8];
#pragma unroll
  for (int t = 0; t < 8; ++t) mu[t] = m2[t] = 0.f;
  if (r < R) {
    for (int p = p0 + r; p < p1; p += R) {
      float v[8];
      load8v(xb + static_cast<long long>(p) * a.C, plane, a.split != 0, v);
      n += 1.f;
      const float inv = 1.f / n;
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        const float d = v[t] - mu[t];
        mu[t] = fmaf(d, inv, mu[t]);
        m2[t] = fmaf(d, v[t] - mu[t], m2[t]);
      }
    }
  }
  sm[0][tid] = n;
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    sm[1 + t][tid] = mu[t];
    sm[9 + t][tid] = m2[t];
  }
  __syncthreads();
  // tree over the R pixel rows of a chunk: row r takes row r + s.  A row < s is read by nobody in
  // its step, so it writes its own slot back at once: one barrier per step.
  int s = 1;
  while (s < R) s <<= 1;
  for (s >>= 1; s >= 1; s >>= 1) {
    if (r < s && r + s < R) {
      const int o = tid + s * cv;
      const float nb = sm[0][o];
      if (nb != 0.f) {
        const float nn = n + nb, f = nb / nn, w = n * f;
#pragma unroll
        for (int t = 0; t < 8; ++t) {
          const float mb = sm[1 + t][o], qb = sm[9 + t][o];
          if (n == 0.f) {
            mu[t] = mb;
            m2[t] = qb;
          } else {
            const float d = mb - mu[t];
            mu[t] = fmaf(d, f, mu[t]);
            m2[t] = (m2[t] + qb) + d * d * w;
          }
        }
        n = nn;
      }
      sm[0][tid] = n;
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        sm[1 + t][tid] = mu[t];
        sm[9 + t][tid] = m2[t];
      }
    }
    __syncthreads();
  }
  // channel c of the block: slot c / 8 (row 0), lane value c % 8.  One thread per group merges its Cg
  // channels in channel order; every channel holds the block's p1 - p0 pixels.
  const int Cg = Cl / a.G;
  const float npix = static_cast<float>(p1 - p0);
  float2* part = FUSED ? nullptr : reinterpret_cast<float2*>(a.ws) + (static_cast<size_t>(b) * (gm.nblk + 1) + blk) * a.G;
  for (int g = tid; g < a.G; g += kGnThreads) {
    float na = 0.f, ma = 0.f, qa = 0.f;
    for (int c = g * Cg; c < (g + 1) * Cg; ++c) chan_merge(na, ma, qa, npix, sm[1 + (c & 7)][c >> 3], sm[9 + (c & 7)][c >> 3]);
    if (FUSED) sstat[g] = make_float2(ma, 1.f / sqrtf(qa / na + a.eps));
    else part[g] = make_float2(ma, qa);
  }
  if (FUSED) {
    __syncthreads();
    if (r < R) gn_apply(a, Cl, sstat, b, j, r, R, p0, p1);
  }
}

// L (a power of two, <= 64) consecutive lanes per group: lane l of them takes blocks l, l + L, ... in order,
// then a shuffle tree in which lane l takes lane l + s; grid (groups / (256 / L), B).
__global__ __launch_bounds__(kGnThreads) void gn_merge_kernel(const GroupNormArgs a, const GnGeom gm, const int Cl, const int L) {
  const int b = blockIdx.y;
  if (a.live && b >= *a.live) return;
  const int t = blockIdx.x * kGnThreads + threadIdx.x;
  const int g = t / L, lane = t % L;
  const bool on = g < a.G;  // every lane of a wave takes part in the shuffles
  const int Cg = Cl / a.G;
  float2* base = reinterpret_cast<float2*>(a.ws) + static_cast<size_t>(b) * (gm.nblk + 1) * a.G;
  float n = 0.f, mu = 0.f, m2 = 0.f;
  for (int blk = lane; on && blk < gm.nblk; blk += L) {
    const float2 p = base[static_cast<size_t>(blk) * a.G + g];
    const int pix = min(a.HW, (blk + 1) * gm.ppb) - blk * gm.ppb;
    chan_merge(n, mu, m2, static_cast<float>(pix) * Cg, p.x, p.y);
  }
  for (int s = L >> 1; s >= 1; s >>= 1) {
    const float nb = __shfl_down(n, s, L), mb = __shfl_down(mu, s, L), qb = __shfl_down(m2, s, L);
    if (lane < s) chan_merge(n, mu, m2, nb, mb, qb);
  }
  if (on && lane == 0) base[static_cast<size_t>(gm.nblk) * a.G + g] = make_float2(mu, 1.f / sqrtf(m2 / n + a.eps));
}

__global__ __launch_bounds__(kGnThreads) void gn_apply_kernel(const GroupNormArgs a, const GnGeom gm, const int Cl) {
  const int b = blockIdx.y;
  if (a.live && b >= *a.live) return;
  const int j = threadIdx.x % gm.cv, r = threadIdx.x / gm.cv;
  if (r >= gm.R) return;
  const int p0 = blockIdx.x * gm.ppb, p1 = min(a.HW, p0 + gm.ppb);
  const float2* st = reinterpret_cast<const float2*>(a.ws) + (static_cast<size_t>(b) * (gm.nblk + 1) + gm.nblk) * a.G;
  gn_apply(a, Cl, st, b, j, r, gm.R, p0, p1);
}

bool aligned(const void* p, uintptr_t n) { return reinterpret_cast<uintptr_t>(p) % n == 0; }

}  // namespace

size_t group_norm_workspace_bytes(int B, int HW, int C, int G) {
  if (B < 1 || HW < 1 || C < 8 || C % 8 || C > kGnMaxC || G < 1) return 0;
  return static_cast<size_t>(B) * gn_ws_floats(gn_geometry(HW, C), G) * sizeof(float);
}

hipError_t group_norm(const GroupNormArgs& a, hipStream_t s) {
  const int Cl = a.Cl ? a.Cl : a.C;
  if (!a.x || !a.out || a.B < 1 || a.B > 65535 || a.HW < 1 || a.C < 8 || a.C % 8 || a.C > kGnMaxC || Cl < 1 || Cl > a.C ||
      a.G < 1 || Cl % a.G || a.act < 0 || a.act > 2 || !(a.eps >= 0.f))
    return hipErrorInvalidValue;
  if (!aligned(a.x, 16) || !aligned(a.out, 16) || !aligned(a.gamma, 4) || !aligned(a.beta, 4) || !aligned(a.ws, 8))
    return hipErrorInvalidValue;
  const size_t need = group_norm_workspace_bytes(a.B, a.HW, a.C, a.G);
  if (!a.ws || need == 0 || a.ws_bytes < need) return hipErrorInvalidValue;
  const GnGeom gm = gn_geometry(a.HW, a.C);
  const dim3 grid(static_cast<unsigned>(gm.nblk), static_cast<unsigned>(a.B));
  if (gm.nblk == 1) {
    hipLaunchKernelGGL(gn_stats_kernel<true>, grid, dim3(kGnThreads), 0, s, a, gm, Cl);
    return hipGetLastError();
  }
  int L = 1;
  while (L < gm.nblk && L < 64) L <<= 1;
  const dim3 mgrid(static_cast<unsigned>((static_cast<long long>(a.G) * L + kGnThreads - 1) / kGnThreads), static_cast<unsigned>(a.B));
  hipLaunchKernelGGL(gn_stats_kernel<false>, grid, dim3(kGnThreads), 0, s, a, gm, Cl);
  hipLaunchKernelGGL(gn_merge_kernel, mgrid, dim3(kGnThreads), 0, s, a, gm, Cl, L);
  hipLaunchKernelGGL(gn_apply_kernel, grid, dim3(kGnThreads), 0, s, a, gm, Cl);
  return hipGetLastError();
}

}  // namespace kern
}  // namespace die
