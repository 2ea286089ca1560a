// iss_kernels.hpp -- Intrinsic Shape Signatures keypoints of a resident scan (I1 - I3 of include/gloc3d.h; tests/iss_ref.py
// restates them) and the gather of the keypoints' feature rows the keypoint-restricted matcher reads (I4).  Compiled in
// iss.hip.
//
//   I1 iss_saliency_kernel   one thread per point over the radius lists ground::scan_lists leaves (original order): fp64
//                            mean and covariance in list order, the sums formed as normals_kernel forms them, the
//                            eigenvalues by a values-only cyclic Jacobi whose arithmetic on A is jacobi_eig3's
//   I2 iss_nms_kernel        radius_self_kernel's cull without lists and without LDS: the store's sorted copy in chunks of
//                            64 with their boxes, a wave per chunk of sources, a ballot over the chunk boxes against r2;
//                            a lane keeps one bit, "beaten", and a wave leaves as soon as no lane is still in the running
//   I3 iss_compact_kernel    the flags to the ascending index list and K (ballot prefix sums, as fpfh_pairs_kernel)
//      iss_gather_rows_kernel  the keypoints' rows out of the features (kept in the order of the sorted points)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ground_normals.hpp"
#include "math3.hpp"

namespace gloc {
namespace iss {

using reg::f32x4;

constexpr int CHUNK = ground::LIST_CHUNK;  // points per chunk of the sorted copy (one box each; not reg::CH, the 1-NN index's)
constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr int ROW = 33;                  // floats per feature row

__device__ __forceinline__ float lane_f(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

// reg::jacobi_eig3 without the eigenvectors: every operation on A is that function's, in its order (V never feeds back
// into A there), so the diagonal left is the same to the bit.
__device__ inline void jacobi_eigvals3(double A[9]) {
  for (int sweep = 0; sweep < 16; ++sweep) {
    const double off = A[1] * A[1] + A[2] * A[2] + A[5] * A[5];
    const double diag = A[0] * A[0] + A[4] * A[4] + A[8] * A[8];
    if (off <= 1e-32 * diag || off == 0.0) break;
    for (int e = 0; e < 3; ++e) {
      const int p = (e == 2) ? 1 : 0, q = (e == 0) ? 1 : 2;
      const double apq = A[3 * p + q];
      if (apq == 0.0) continue;
      const double app = A[3 * p + p], aqq = A[3 * q + q];
      const double theta = (aqq - app) / (2.0 * apq);
      const double at = theta < 0 ? -theta : theta;
      double t = 1.0 / (at + sqrt(theta * theta + 1.0));
      if (theta < 0) t = -t;
      const double c = 1.0 / sqrt(t * t + 1.0);
      const double s = t * c;
      for (int k = 0; k < 3; ++k) {
        const double akp = A[3 * k + p], akq = A[3 * k + q];
        A[3 * k + p] = c * akp - s * akq;
        A[3 * k + q] = s * akp + c * akq;
      }
      for (int k = 0; k < 3; ++k) {
        const double apk = A[3 * p + k], aqk = A[3 * q + k];
        A[3 * p + k] = c * apk - s * aqk;
        A[3 * q + k] = s * apk + c * aqk;
      }
    }
  }
}

// I1.  pts [m] in original order, nb [m][W] the radius lists by original index (padding NONE).  saliency [m] and
// eig [m][3] (sorted, zeros where the list holds fewer than min_nn entries) in original order; either may be null.
__global__ __launch_bounds__(256) void iss_saliency_kernel(const f32x4* __restrict__ pts, uint32_t m, const uint32_t* __restrict__ nb, int W,
                                                            uint32_t min_nn, float g21, float g32, float* __restrict__ saliency,
                                                            double* __restrict__ eig) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  double mean[3] = {0, 0, 0};
  uint32_t cnt = 0;
  for (int s = 0; s < W; ++s) {
    const uint32_t j = nb[(size_t)i * W + s];
    if (j >= m) continue;  // (padding)
    const f32x4 q = pts[j];
    mean[0] += (double)q.x; mean[1] += (double)q.y; mean[2] += (double)q.z;
    ++cnt;
  }
  double l1 = 0.0, l2 = 0.0, l3 = 0.0;
  float sal = 0.f;
  if (cnt >= min_nn) {
    for (int a = 0; a < 3; ++a) mean[a] = mean[a] / (double)cnt;
    double C[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int s = 0; s < W; ++s) {
      const uint32_t j = nb[(size_t)i * W + s];
      if (j >= m) continue;
      const f32x4 q = pts[j];
      const double d[3] = {(double)q.x - mean[0], (double)q.y - mean[1], (double)q.z - mean[2]};
      C[0] += d[0] * d[0]; C[1] += d[0] * d[1]; C[2] += d[0] * d[2];
      C[4] += d[1] * d[1]; C[5] += d[1] * d[2];
      C[8] += d[2] * d[2];
    }
    C[3] = C[1]; C[6] = C[2]; C[7] = C[5];
    jacobi_eigvals3(C);
    l1 = C[0]; l2 = C[4]; l3 = C[8];
    double t;
    if (l1 < l2) { t = l1; l1 = l2; l2 = t; }
    if (l2 < l3) { t = l2; l2 = l3; l3 = t; }
    if (l1 < l2) { t = l1; l1 = l2; l2 = t; }
    if (l3 > 0.0 && l2 < (double)g21 * l1 && l3 < (double)g32 * l2) sal = (float)l3;
  }
  if (saliency) saliency[i] = sal;
  if (eig) {
    eig[3 * (size_t)i + 0] = l1;
    eig[3 * (size_t)i + 1] = l2;
    eig[3 * (size_t)i + 2] = l3;
  }
}

// the saliencies in the order of the sorted points (spts[s].w = original index of sorted position s)
__global__ __launch_bounds__(256) void iss_sort_saliency_kernel(const f32x4* __restrict__ spts, uint32_t m, const float* __restrict__ sal,
                                                                 float* __restrict__ sal_sorted) {
  const uint32_t s = blockIdx.x * 256 + threadIdx.x;
  if (s >= m) return;
  const uint32_t o = __float_as_uint(spts[s].w);
  sal_sorted[s] = o < m ? sal[o] : 0.f;
}

// I2.  Four independent waves per work-group, one chunk of sources each (no LDS, no barrier).  sal [m] in sorted order;
// keypoint [m] by ORIGINAL index: 1 iff the point's saliency is positive and nothing within r2 beats it.
__global__ __launch_bounds__(256) void iss_nms_kernel(const f32x4* __restrict__ spts, uint32_t m, const float* __restrict__ sal,
                                                       const f32x4* __restrict__ box_lo, const f32x4* __restrict__ box_hi, uint32_t nchunks,
                                                       float r2, uint8_t* __restrict__ keypoint) {
  const int lane = threadIdx.x & 63;
  const uint32_t own = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (own >= nchunks) return;  // (the whole wave)
  const uint32_t si = own * CHUNK + lane;
  const bool valid = si < m;
  const f32x4 p = spts[valid ? si : m - 1];
  const float ps = valid ? sal[si] : 0.f;
  const uint32_t po = __float_as_uint(p.w);
  const bool live = valid && po < m && ps > 0.f;
  bool beaten = false;
  auto eval_chunk = [&](uint32_t c) {
    const uint32_t j = c * CHUNK + lane;
    f32x4 v = {reg::NN_FAR, reg::NN_FAR, reg::NN_FAR, __uint_as_float(NONE)};
    float vs = 0.f;
    if (j < m) {
      v = spts[j];
      vs = sal[j];
    }
    unsigned long long cand = __ballot(vs > 0.f);  // (a point of saliency 0 beats nobody who is in the running)
    while (cand) {
      const int t = __ffsll((long long)cand) - 1;
      cand &= cand - 1;
      const float d = reg::dist2(p.x, p.y, p.z, lane_f(v.x, t), lane_f(v.y, t), lane_f(v.z, t));
      const float qs = lane_f(vs, t);
      const uint32_t qo = __float_as_uint(lane_f(v.w, t));
      if (d <= r2 && qo != po && (qs > ps || (qs == ps && qo < po))) beaten = true;  // (a NaN distance is never inside)
    }
  };
  if (__any(live)) {
    eval_chunk(own);
    const f32x4 olo = box_lo[own], ohi = box_hi[own];
    for (uint32_t c0 = 0; c0 < nchunks && __any(live && !beaten); c0 += 64) {
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
        const bool need = live && !beaten && reg::box_lb(p.x, p.y, p.z, lo, hi) <= r2;  // <=: a point at exactly r is inside
        if (!__any(need)) {
          if (!__any(live && !beaten)) break;
          continue;
        }
        eval_chunk(c0 + b);
      }
    }
  }
  if (valid && po < m) keypoint[po] = (live && !beaten) ? 1 : 0;
}

// I3.  One work-group: out[rank] = i for the flagged points in ascending i, *count = K.
__global__ __launch_bounds__(1024) void iss_compact_kernel(const uint8_t* __restrict__ flag, uint32_t m, uint32_t* __restrict__ out,
                                                            uint32_t* __restrict__ count) {
  __shared__ uint32_t wave_cnt[16], base_s;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (tid == 0) base_s = 0;
  __syncthreads();
  for (uint32_t i0 = 0; i0 < m; i0 += 1024) {
    const uint32_t i = i0 + (uint32_t)tid;
    const bool keep = i < m && flag[i] != 0;
    const unsigned long long mk = __ballot(keep);
    if (lane == 0) wave_cnt[w] = (uint32_t)__popcll(mk);
    __syncthreads();
    uint32_t off = base_s, tot = 0;
    for (int q = 0; q < 16; ++q) {
      if (q < w) off += wave_cnt[q];
      tot += wave_cnt[q];
    }
    if (keep) out[off + (uint32_t)__popcll(mk & ((1ull << lane) - 1ull))] = i;
    __syncthreads();
    if (tid == 0) base_s += tot;
    __syncthreads();
  }
  if (tid == 0) *count = base_s;
}

// out[r] = the feature row of keypoint r: feat is in the order of the sorted points, inv maps an original index to it.
__global__ __launch_bounds__(256) void iss_gather_rows_kernel(const uint32_t* __restrict__ kp, uint32_t K, uint32_t n,
                                                               const uint32_t* __restrict__ inv, const float* __restrict__ feat,
                                                               float* __restrict__ out) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)K * ROW) return;
  const uint32_t r = (uint32_t)(e / ROW), c = (uint32_t)(e % ROW);
  const uint32_t o = kp[r];
  const uint32_t s = o < n ? inv[o] : NONE;
  out[e] = s < n ? feat[(size_t)s * ROW + c] : 0.f;
}

}  // namespace iss
}  // namespace gloc
