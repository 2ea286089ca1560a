// fgr_kernels.hpp -- device kernels of the Fast Global Registration on a match list (gfx950; include/gloc3d.h R1 - R4,
// tests/fgr_ref.py is the contract).
//
//   tuple_kernel   R1's test, one thread per (job, h): the keyed sample of F4 (ransac_sample.hpp), the three edge lengths
//                  on both sides in fp64, a pass bit; a wave's 64 bits go out as one ballot word
//   gnc_kernel     one work-group per job, everything else in ONE launch: the ranking of the pass bits (popcount prefix,
//                  the first max_tuples in h order) into the multiplicities, the gather of the active pairs, the centroids
//                  and D^2, ALL max_iters graduated-non-convexity updates, the inlier count of the final pose
//
// The correspondences are fixed, so an update needs nothing from outside the work-group: lane l sums the 27 fp64
// contributions (H's upper triangle 21, g 6) of the active entries l, l + 256, ... in that order, gn6::reduce_store
// reduces them over the wave and the four waves into LDS, one lane runs gn6::chol_rodrigues on the fp64 pose in LDS, a
// barrier ends the update.  The scale mu is stepped in registers by R2's rule, the same value in every lane.  A job's
// arithmetic touches its own rows only: nothing depends on the batch around it.  No floating-point atomics; the
// multiplicities are integer atomics, whose sum does not depend on order.
//
// LDS: the active pairs -- x, y, z of both sides and the multiplicity, 28 B an entry, structure of arrays -- stay in
// dynamic LDS when they fit.  Capacity LDS_CAP = 4096 entries (112 KiB of the CU's 160; the default 3 x 1000 tuple members
// need at most 3000); the launch asks only for what its longest list can need.  A job with more active pairs streams them
// from the pair list through its index list every update.
//
// Visibility inside the work-group: the multiplicities and the index list are written to global memory and read back by
// other lanes of the same work-group behind a fence and a barrier, with device-scope loads that do not stop at the
// CU's vector cache.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fgr.hpp"            // JobIn, Result
#include "gn6_kernels.hpp"    // reduce_store, chol_rodrigues
#include "math3.hpp"          // f32x4, xform, dist2
#include "ransac_sample.hpp"
#include "robust.hpp"

namespace gloc {
namespace fgr {

using reg::f32x4;

constexpr int THREADS = gn6::ACC_THREADS;  // reduce_store's work-group
constexpr uint32_t LDS_CAP = 4096;         // active entries that stay in LDS
constexpr uint32_t ENTRY_BYTES = 28;
struct Rule {
  uint32_t tuple_tries, max_tuples, max_iters, anneal_every;
  double tuple_scale, anneal_div, delta2;
  float thr2;
  uint64_t seed;
};

__device__ __forceinline__ uint32_t ld_dev_u32(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ double edge_len(const f32x4& a, const f32x4& b) {
  const double dx = (double)a.x - (double)b.x, dy = (double)a.y - (double)b.y, dz = (double)a.z - (double)b.z;
  return sqrt((dx * dx + dy * dy) + dz * dz);
}

// grid (ceil(tries / THREADS), jobs); bits [job][words], words = ceil(tries / 64)
static __global__ __launch_bounds__(THREADS) void tuple_kernel(const f32x4* __restrict__ pairs, size_t ld, const JobIn* __restrict__ jobs,
                                                               Rule r, unsigned long long* __restrict__ bits, uint32_t words) {
  const uint32_t job = blockIdx.y, h = blockIdx.x * THREADS + threadIdx.x;
  const uint32_t m = jobs[job].m;
  bool pass = false;
  uint32_t t[3];
  if (h < r.tuple_tries && m >= 3 && reg::ransac_sample(r.seed, jobs[job].stream, h, m, t)) {
    f32x4 p[3], q[3];
    for (int k = 0; k < 3; ++k) {
      p[k] = pairs[((size_t)job * ld + t[k]) * 2 + 0];
      q[k] = pairs[((size_t)job * ld + t[k]) * 2 + 1];
    }
    pass = true;
    for (int k = 0; k < 3; ++k) {
      const int j = k == 2 ? 0 : k + 1;
      const double lp = edge_len(p[k], p[j]), lq = edge_len(q[k], q[j]);
      pass = pass && (r.tuple_scale * lp < lq) && (r.tuple_scale * lq < lp);  // (a NaN or infinite length, or a zero one, fails)
    }
  }
  const unsigned long long b = __builtin_amdgcn_ballot_w64(pass);
  const uint32_t word = h >> 6;
  if ((threadIdx.x & 63) == 0 && word < words) bits[(size_t)job * words + word] = b;
}

// the work-group's sum of one count per lane, and this lane's exclusive prefix of it in lane order; two barriers
__device__ __forceinline__ uint32_t block_prefix(uint32_t c, uint32_t* wsum /* LDS [THREADS / 64] */, uint32_t* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t incl = c;
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t up = __shfl_up(incl, o);
    if (lane >= o) incl += up;
  }
  if (lane == 63) wsum[w] = incl;
  __syncthreads();
  uint32_t off = 0, tot = 0;
  for (int ww = 0; ww < THREADS / 64; ++ww) {
    const uint32_t s = wsum[ww];
    off += ww < w ? s : 0u;
    tot += s;
  }
  __syncthreads();
  *total = tot;
  return off + incl - c;
}

// grid (jobs), THREADS lanes, dynamic LDS ENTRY_BYTES x cap.  mult [job][ld] (zero on entry), act [job][ld].
static __global__ __launch_bounds__(THREADS) void gnc_kernel(const f32x4* __restrict__ pairs, size_t ld, const JobIn* __restrict__ jobs, Rule r,
                                                             const unsigned long long* __restrict__ bits, uint32_t words, uint32_t cap,
                                                             uint32_t* __restrict__ mult, uint32_t* __restrict__ act, Result* __restrict__ results) {
  extern __shared__ __attribute__((aligned(16))) float ent[];  // [7][cap]: px py pz qx qy qz, the multiplicity (uint32)
  __shared__ double red[THREADS / 64][gn6::NSLOT];
  __shared__ double tot[gn6::NSLOT];
  __shared__ double Tsh[12];
  __shared__ double dmax_sh[THREADS / 64];
  __shared__ float Tf_sh[12];
  __shared__ uint32_t wsum[THREADS / 64];
  __shared__ uint32_t inl_sh, upd_sh;
  __shared__ int status_sh;
  const uint32_t job = blockIdx.x, tid = threadIdx.x;
  const int lane = tid & 63;
  const uint32_t m = jobs[job].m;
  uint32_t* ent_mu = reinterpret_cast<uint32_t*>(ent) + 6 * (size_t)cap;
  Result& out = results[job];
  const f32x4* __restrict__ pr = pairs + (size_t)job * ld * 2;
  uint32_t* __restrict__ mu_row = mult + (size_t)job * ld;
  uint32_t* __restrict__ act_row = act + (size_t)job * ld;
  if (tid == 0) {
    for (int k = 0; k < 12; ++k) Tsh[k] = (k == 0 || k == 4 || k == 8) ? 1.0 : 0.0;
    inl_sh = 0u;
    upd_sh = 0u;
    status_sh = 0;
  }
  if (tid < gn6::NSLOT) tot[tid] = 0.0;
  __syncthreads();

  uint32_t n_tuples = 0, n_act = 0;
  double d2 = 0.0;
  if (m >= 3) {  // (uniform)
    // ---- R1: the first max_tuples passing samples in h order -> multiplicities
    if (r.tuple_tries) {
      uint32_t base = 0;
      for (uint32_t w0 = 0; w0 < words && base < r.max_tuples; w0 += THREADS) {
        const uint32_t wi = w0 + tid;
        unsigned long long word = wi < words ? bits[(size_t)job * words + wi] : 0ull;
        uint32_t total;
        uint32_t rank = base + block_prefix((uint32_t)__popcll(word), wsum, &total);
        while (word && rank < r.max_tuples) {
          const uint32_t h = wi * 64u + (uint32_t)__builtin_ctzll(word);
          word &= word - 1ull;
          uint32_t t[3];
          reg::ransac_sample(r.seed, jobs[job].stream, h, m, t);
          for (int k = 0; k < 3; ++k) atomicAdd(&mu_row[t[k]], 1u);
          ++rank;
        }
        base += total;
      }
      n_tuples = base < r.max_tuples ? base : r.max_tuples;
      __threadfence();
      __syncthreads();
    }
    // ---- the active pairs, in ascending position
    for (uint32_t i0 = 0; i0 < m; i0 += THREADS) {
      const uint32_t i = i0 + tid;
      uint32_t mu = 0;
      f32x4 pv = {0.f, 0.f, 0.f, 0.f}, qv = {0.f, 0.f, 0.f, 0.f};
      if (i < m) {
        pv = pr[(size_t)i * 2 + 0];
        qv = pr[(size_t)i * 2 + 1];
        if (r.tuple_tries) mu = ld_dev_u32(&mu_row[i]);
        else {
          const bool fin = isfinite(pv.x) && isfinite(pv.y) && isfinite(pv.z) && isfinite(qv.x) && isfinite(qv.y) && isfinite(qv.z);
          mu = fin ? 1u : 0u;
          mu_row[i] = mu;
        }
      }
      uint32_t total;
      const uint32_t pos = n_act + block_prefix(mu ? 1u : 0u, wsum, &total);
      if (mu) {
        act_row[pos] = i;
        if (pos < cap) {
          ent[0 * (size_t)cap + pos] = pv.x;
          ent[1 * (size_t)cap + pos] = pv.y;
          ent[2 * (size_t)cap + pos] = pv.z;
          ent[3 * (size_t)cap + pos] = qv.x;
          ent[4 * (size_t)cap + pos] = qv.y;
          ent[5 * (size_t)cap + pos] = qv.z;
          ent_mu[pos] = mu;
        }
      }
      n_act += total;
    }
    __threadfence();
    __syncthreads();
  }
  const bool in_lds = n_act <= cap;
  auto fetch = [&](uint32_t e, double* p, double* q, double* wm) {
    if (in_lds) {
      for (int a = 0; a < 3; ++a) {
        p[a] = (double)ent[a * (size_t)cap + e];
        q[a] = (double)ent[(3 + a) * (size_t)cap + e];
      }
      *wm = (double)ent_mu[e];
    } else {
      const uint32_t i = ld_dev_u32(&act_row[e]);
      const f32x4 pv = pr[(size_t)i * 2 + 0], qv = pr[(size_t)i * 2 + 1];
      p[0] = (double)pv.x; p[1] = (double)pv.y; p[2] = (double)pv.z;
      q[0] = (double)qv.x; q[1] = (double)qv.y; q[2] = (double)qv.z;
      *wm = (double)ld_dev_u32(&mu_row[i]);
    }
  };

  double v[gn6::NSLOT];
  // ---- R2: centroids and D^2
  if (n_act) {  // (uniform)
#pragma unroll
    for (int k = 0; k < gn6::NSLOT; ++k) v[k] = 0.0;
    for (uint32_t e = tid; e < n_act; e += THREADS) {
      double p[3], q[3], wm;
      fetch(e, p, q, &wm);
      for (int a = 0; a < 3; ++a) {
        v[a] += wm * p[a];
        v[3 + a] += wm * q[a];
      }
      v[6] += wm;
    }
    gn6::reduce_store(v, red, tot);
    __syncthreads();
    double cp[3], cq[3];
    for (int a = 0; a < 3; ++a) {
      cp[a] = tot[a] / tot[6];
      cq[a] = tot[3 + a] / tot[6];
    }
    double dm = 0.0;
    for (uint32_t e = tid; e < n_act; e += THREADS) {
      double p[3], q[3], wm;
      fetch(e, p, q, &wm);
      const double ax = p[0] - cp[0], ay = p[1] - cp[1], az = p[2] - cp[2];
      const double bx = q[0] - cq[0], by = q[1] - cq[1], bz = q[2] - cq[2];
      const double a2 = (ax * ax + ay * ay) + az * az, b2 = (bx * bx + by * by) + bz * bz;
      const double mx = a2 > b2 ? a2 : b2;
      dm = mx > dm ? mx : dm;
    }
    for (int o = 32; o > 0; o >>= 1) {
      const double other = __shfl_xor(dm, o);
      dm = other > dm ? other : dm;
    }
    if (lane == 0) dmax_sh[tid >> 6] = dm;
    __syncthreads();  // (every lane has read tot)
    for (int w = 0; w < THREADS / 64; ++w) d2 = dmax_sh[w] > d2 ? dmax_sh[w] : d2;
    if (tid < gn6::NSLOT) tot[tid] = 0.0;
    __syncthreads();
  }

  // ---- R3: the updates
  if (m >= 3) {
    double mu_k = d2 > r.delta2 ? d2 : r.delta2;
    for (uint32_t k = 0; k < r.max_iters; ++k) {
      if (k > 0 && k % r.anneal_every == 0) {
        const double nx = mu_k / r.anneal_div;
        mu_k = nx > r.delta2 ? nx : r.delta2;
      }
      double T[12];
#pragma unroll
      for (int a = 0; a < 12; ++a) T[a] = Tsh[a];
#pragma unroll
      for (int a = 0; a < gn6::NSLOT; ++a) v[a] = 0.0;
      for (uint32_t e = tid; e < n_act; e += THREADS) {
        double p[3], q[3], wm;
        fetch(e, p, q, &wm);
        const double x = ((T[0] * p[0] + T[1] * p[1]) + T[2] * p[2]) + T[9];
        const double y = ((T[3] * p[0] + T[4] * p[1]) + T[5] * p[2]) + T[10];
        const double z = ((T[6] * p[0] + T[7] * p[1]) + T[8] * p[2]) + T[11];
        const double rx = x - q[0], ry = y - q[1], rz = z - q[2];
        const double s2 = (rx * rx + ry * ry) + rz * rz;
        const double w = wm * robust::weight<GLOC_ROBUST_GEMAN_MCCLURE>(s2, mu_k);
        // J = [-[x]x | I]: columns (0, -z, y), (z, 0, -x), (-y, x, 0), e0, e1, e2
        v[0] += w * (z * z + y * y);
        v[1] += w * (-(x * y));
        v[2] += w * (-(x * z));
        v[4] += w * (-z);
        v[5] += w * y;
        v[6] += w * (z * z + x * x);
        v[7] += w * (-(y * z));
        v[8] += w * z;
        v[10] += w * (-x);
        v[11] += w * (y * y + x * x);
        v[12] += w * (-y);
        v[13] += w * x;
        v[15] += w;
        v[21] += w * (y * rz - z * ry);
        v[22] += w * (z * rx - x * rz);
        v[23] += w * (x * ry - y * rx);
        v[24] += w * rx;
        v[25] += w * ry;
        v[26] += w * rz;
      }
      v[18] = v[15];
      v[20] = v[15];
      gn6::reduce_store(v, red, tot);
      __syncthreads();
      if (tid == 0) {
        double Tn[12], xi[6], th;
        if (n_act >= 3 && gn6::chol_rodrigues(tot, Tsh, Tn, xi, &th)) {
          for (int a = 0; a < 12; ++a) Tsh[a] = Tn[a];
          upd_sh = k + 1;
        } else {
          status_sh = 2;
        }
      }
      __syncthreads();
      if (status_sh) break;  // (uniform)
    }
  }

  // ---- R4: the verdict's numbers
  const uint32_t updates = upd_sh;
  if (tid < 12) Tf_sh[tid] = (float)Tsh[tid];
  __syncthreads();
  if (updates) {
    float Tf[12];
#pragma unroll
    for (int a = 0; a < 12; ++a) Tf[a] = Tf_sh[a];
    uint32_t cnt = 0;
    for (uint32_t i0 = 0; i0 < m; i0 += THREADS) {
      const uint32_t i = i0 + tid;
      bool in = false;
      if (i < m) {
        const f32x4 pv = pr[(size_t)i * 2 + 0], qv = pr[(size_t)i * 2 + 1];
        float x, y, z;
        reg::xform(Tf, pv.x, pv.y, pv.z, x, y, z);
        in = reg::dist2(x, y, z, qv.x, qv.y, qv.z) < r.thr2;
      }
      cnt += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(in));
    }
    if (lane == 0 && cnt) atomicAdd(&inl_sh, cnt);
    __syncthreads();
  }
  if (tid < 12) {
    out.Td[tid] = Tsh[tid];
    out.Tf[tid] = Tf_sh[tid];
  }
  if (tid < NSYS) out.system[tid] = tot[tid];
  if (tid == 0) {
    out.d2 = d2;
    out.inliers = inl_sh;
    out.n_tuples = n_tuples;
    out.updates = updates;
    out.status = (m >= 3 && status_sh == 0) ? 0 : 2;
  }
}

}  // namespace fgr
}  // namespace gloc
