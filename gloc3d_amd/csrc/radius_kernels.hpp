// radius_kernels.hpp -- the exact fixed-radius, capped neighbour search of a resident scan within itself (R1 of
// include/gloc3d.h; tests/fpfh_radius_ref.py restates it): the lists behind the radius-support normals and FPFH features.
// Compiled in ground.hip, after ground_kernels.hpp, whose chunks, boxes and un-fused distance it shares.
//
// radius_self_kernel is knn_culled_kernel with a metric bound: a wave owns one chunk of 64 sorted sources, ballots over the
// chunk boxes and evaluates every chunk whose box comes within r of its own.  Two things differ.
//   * A lane's list holds up to 128 entries, too many for registers: it is a column of 64-bit keys
//     (bits(d2) << 32 | original index) in LDS, entry s of lane l at [s * 64 + l] -- a wave-wide access at one s touches every
//     bank once.  The width is a launch parameter that sizes the dynamic LDS (512 B x max_nn per wave, 64 KiB at 128): a
//     32-wide normal search runs four times the waves per CU of a 128-wide feature search.  d2 is never negative nor NaN
//     where it is kept, so the keys order as (d2, index) does.  The column is NOT kept sorted: a wave pays for an insert
//     whenever any of its lanes makes one, and a sorted insert is a chain of dependent LDS reads and writes (the first form
//     of this kernel: 2.8 ms for the 100-wide search of a 13 k scan, now 2.1).  Instead a list fills by appending, a full
//     list replaces its largest key and looks for the new largest -- max_nn independent reads -- and the order is made once
//     at the end, each key written to the output slot of its rank.
//   * count(i) is the size of the WHOLE neighbourhood, so every chunk within r is visited whether a lane's list is full or
//     not: the cull is on r2 throughout, and a full list only spares the insertion (its bound tightens to its largest key).
// The candidates of a chunk are not staged: each lane holds one and the wave reads them lane by lane (v_readlane), which
// leaves all of the LDS to the lists.  No atomics: a lane owns its column and its output row.
#pragma once
#include "ground_kernels.hpp"

namespace gloc {
namespace ground {

constexpr int RADIUS_MAX_NN = 128;

__device__ __forceinline__ float lane_f(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

// One wave per work-group, one chunk of sources per wave.  idx / d2 [m][W] and count [m] by ORIGINAL index (each may be null).
__global__ __launch_bounds__(64) void radius_self_kernel(const f32x4* __restrict__ spts, uint32_t m, const f32x4* __restrict__ box_lo,
                                                         const f32x4* __restrict__ box_hi, uint32_t nchunks, float r2, int W,
                                                         uint32_t* __restrict__ idx, float* __restrict__ d2, uint32_t* __restrict__ count) {
  extern __shared__ unsigned long long rad_list[];  // [W][64]
  const int lane = threadIdx.x;
  const uint32_t own = blockIdx.x;
  if (own >= nchunks) return;
  const uint32_t si = own * KCH + lane;
  const bool valid = si < m;
  const f32x4 p = spts[valid ? si : m - 1];
  unsigned long long* L = rad_list + lane;
  int len = 0;
  uint32_t cnt = 0;
  // a candidate within r2 enters the list iff its key < worst: all ones while there is room, then the list's largest key
  unsigned long long worst = ~0ull;
  int wpos = 0;  // a full list: the slot of its largest key
  auto insert = [&](unsigned long long key) {
    L[(len < W ? len : wpos) * 64] = key;
    if (len < W) ++len;
    if (len == W) {
      unsigned long long mx = 0;
      for (int s = 0; s < W; ++s) {
        const unsigned long long kk = L[s * 64];
        if (kk >= mx) { mx = kk; wpos = s; }
      }
      worst = mx;
    }
  };
  auto eval_chunk = [&](uint32_t c) {
    const uint32_t j = c * KCH + lane;
    f32x4 v = {NN_FAR_, NN_FAR_, NN_FAR_, __uint_as_float(0xFFFFFFFFu)};
    if (j < m) v = spts[j];
    const int lim = (int)((m - c * KCH) < (uint32_t)KCH ? (m - c * KCH) : (uint32_t)KCH);
    for (int t = 0; t < KCH; t += 8) {
      float d[8];
      uint32_t o[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        d[u] = reg::dist2(p.x, p.y, p.z, lane_f(v.x, t + u), lane_f(v.y, t + u), lane_f(v.z, t + u));
        o[u] = __float_as_uint(lane_f(v.w, t + u));
      }
      const float dm = fminf(fminf(fminf(d[0], d[1]), fminf(d[2], d[3])), fminf(fminf(d[4], d[5]), fminf(d[6], d[7])));
      if (valid && dm <= r2) {
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (t + u < lim && d[u] <= r2) {  // (a NaN distance is never inside)
            ++cnt;
            const unsigned long long key = ((unsigned long long)__float_as_uint(d[u]) << 32) | (unsigned long long)o[u];
            if (key < worst) insert(key);
          }
      }
    }
  };
  eval_chunk(own);
  const f32x4 olo = box_lo[own], ohi = box_hi[own];
  for (uint32_t c0 = 0; c0 < nchunks; c0 += 64) {
    const uint32_t cl = c0 + lane;
    const bool other = cl < nchunks && cl != own;
    float lbw = __builtin_inff();
    f32x4 blo = {0.f, 0.f, 0.f, 0.f}, bhi = {0.f, 0.f, 0.f, 0.f};
    if (other) {
      blo = box_lo[cl]; bhi = box_hi[cl];
      const float ex = fmaxf(fmaxf(blo.x - ohi.x, olo.x - bhi.x), 0.f);
      const float ey = fmaxf(fmaxf(blo.y - ohi.y, olo.y - bhi.y), 0.f);
      const float ez = fmaxf(fmaxf(blo.z - ohi.z, olo.z - bhi.z), 0.f);
      lbw = ((ex * ex + ey * ey) + ez * ez) * 0.99999905f;
    }
    unsigned long long mask = __ballot(other && lbw <= r2);  // (`other` on its own: r2 may be infinite)
    while (mask) {
      const int b = __ffsll((long long)mask) - 1;
      mask &= mask - 1;
      f32x4 lo, hi;
      lo.x = lane_f(blo.x, b); lo.y = lane_f(blo.y, b); lo.z = lane_f(blo.z, b);
      hi.x = lane_f(bhi.x, b); hi.y = lane_f(bhi.y, b); hi.z = lane_f(bhi.z, b);
      const bool need = valid && reg::box_lb(p.x, p.y, p.z, lo, hi) <= r2;  // <=: a point at exactly r is inside
      if (!__any(need)) continue;
      eval_chunk(c0 + b);
    }
  }
  if (valid) {
    const uint32_t orig = __float_as_uint(p.w);
    if (orig < m) {
      for (int s = 0; s < len; ++s) {  // ascending (d2, index): a key goes to the slot of its rank
        const unsigned long long key = L[s * 64];
        int rank = 0;
        for (int t = 0; t < len; ++t) rank += L[t * 64] < key ? 1 : 0;
        if (idx) idx[(size_t)orig * W + rank] = (uint32_t)(key & 0xFFFFFFFFull);
        if (d2) d2[(size_t)orig * W + rank] = __uint_as_float((uint32_t)(key >> 32));
      }
      for (int s = len; s < W; ++s) {
        if (idx) idx[(size_t)orig * W + s] = 0xFFFFFFFFu;
        if (d2) d2[(size_t)orig * W + s] = FLT_MAX;
      }
      if (count) count[orig] = cnt;
    }
  }
}

// R2's minimum: the normal of a point whose list holds fewer than min_nn entries (count capped at the list width) is none.
// Runs behind normals_kernel on the radius lists, so the arithmetic of every normal that stays is that kernel's.
__global__ __launch_bounds__(256) void normals_min_nn_kernel(uint32_t m, const uint32_t* __restrict__ count, uint32_t max_nn, uint32_t min_nn,
                                                              float* __restrict__ normals) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  if (min(count[i], max_nn) < min_nn) {
    normals[3 * (size_t)i + 0] = 0.f;
    normals[3 * (size_t)i + 1] = 0.f;
    normals[3 * (size_t)i + 2] = 0.f;
  }
}

}  // namespace ground
}  // namespace gloc
