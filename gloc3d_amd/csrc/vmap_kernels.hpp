// vmap_kernels.hpp -- the device half of the resident voxel maps (gfx950; include/gloc3d.h: M1 - M8).  tests/vmap_ref.py
// is the contract.  A map is the voxelized generalized ICP's target (vgicp::Voxel[], one open-addressing table) that
// outlives the call: scans are merged into it, voxels are pruned from it, and vgicp_accum_kernel probes it through the
// vgicp::Target view it takes every target by.
//
//   insert   move_kernel (T given: p = R s + t in fp32, reg::xform)  ->  the voxel map builder of voxel_map_kernels.hpp
//            over the moved points with contrib_stats_kernel as its statistics kernel: voxel_stats_kernel's sums, left as
//            SUMS (n, s1, s2), the normal rotated by T  ->  count_new_kernel: one lane per contribution voxel probes the
//            resident table, flags the keys it lacks and keeps the index of the ones it has  ->  flag scan  ->  the host
//            reads the count of new keys and refuses an insert that does not fit  ->  merge_kernel: one lane per
//            contribution voxel; a new key claims a slot by a 64-bit atomicCAS and becomes voxel n_voxels + its rank, an
//            old one adds its sums to the voxel's; mean and Nbar are formed again from the running sums
//   prune    prune_flags_kernel (1: the voxel stays)  ->  flag scan  ->  compact_kernel into scratch, copied back  ->  the
//            table cleared and rebuilt by voxmap::cell_hash_kernel
//
// Keys within a launch are unique (the builder makes one contribution voxel per key), so no two lanes of merge_kernel
// touch one voxel and nothing here adds floating-point numbers atomically.  The table holds at most `capacity` keys in
// >= 2 x capacity slots: every probe ends at an empty slot; all the same every probe loop here is bounded by the table's
// size and leaves a word in `err` instead of spinning should the table ever be broken.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "math3.hpp"
#include "vgicp_kernels.hpp"
#include "voxel_map_kernels.hpp"

namespace gloc {
namespace vmap {

using vgicp::TgtAux;
using vgicp::Voxel;
using voxmap::KEY_BIAS;
using voxmap::KEY_NONE;

constexpr uint32_t NO_VOXEL = 0xFFFFFFFFu;

struct Contrib {  // what one insert adds to one voxel; the builder's cell type (a key and a valid flag, as Voxel)
  unsigned long long key;
  uint32_t count, valid;
  double s1[3];  // sum (p - corner)
  double s2[6];  // sum m m^T: xx xy xz yy yz zz
};

struct Sums {  // beside every resident voxel: what its mean and Nbar are the quotients of
  double s1[3];
  double s2[6];
};

struct Pose {  // scan -> map as the kernels take it: R row-major 9, t 3 (reg::xform's layout); on = 0: the scan as it is
  float T[12];
  uint32_t on;
};

struct Counters {  // of one insert or prune, zeroed before it
  unsigned long long points;  // insert: points of the contribution; prune: points of the voxels removed
  uint32_t err;               // a probe ran the length of the table, or a voxel index beyond the capacity
  uint32_t pad_;
};

__device__ __forceinline__ void corner_of(unsigned long long k, double res, double* c) {
  c[0] = (double)((long long)((k >> 42) & 0x1FFFFF) - KEY_BIAS) * res;
  c[1] = (double)((long long)((k >> 21) & 0x1FFFFF) - KEY_BIAS) * res;
  c[2] = (double)((long long)(k & 0x1FFFFF) - KEY_BIAS) * res;
}

// the sum of v over the wave in lane 0
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

static __global__ void move_kernel(const float* __restrict__ xyz, uint32_t n, Pose P, float* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  reg::xform(P.T, xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2], out[3 * (size_t)i], out[3 * (size_t)i + 1],
             out[3 * (size_t)i + 2]);
}

// vgicp::voxel_stats_kernel's sums of one scan (tg[0]: its points already moved), one thread per voxel, in the scan's
// upload order; the normal is rotated in fp64 from the fp32 values by the accumulate kernel's expression
static __global__ void contrib_stats_kernel(const voxmap::TgtDesc* __restrict__ tg, const TgtAux* __restrict__ aux,
                                            const unsigned long long* __restrict__ key, const uint32_t* __restrict__ val,
                                            const uint32_t* __restrict__ flag, const uint32_t* __restrict__ pos, double res, Pose P,
                                            Contrib* __restrict__ out) {
  const voxmap::TgtDesc d = tg[blockIdx.y];
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= d.n || !flag[d.begin + i]) return;
  const TgtAux a = aux[blockIdx.y];
  const unsigned long long k = key[d.begin + i];
  double c[3];
  corner_of(k, res, c);
  Contrib o;
  o.key = k;
  o.valid = 1u;
  for (int q = 0; q < 3; ++q) o.s1[q] = 0.0;
  for (int q = 0; q < 6; ++q) o.s2[q] = 0.0;
  uint32_t n = 0;
  for (uint32_t t = i; t < d.n && key[d.begin + t] == k; ++t) {
    const uint32_t j = val[d.begin + t];  // (the sort is stable: ascending original index inside a voxel)
    o.s1[0] += (double)d.xyz[3 * (size_t)j] - c[0];
    o.s1[1] += (double)d.xyz[3 * (size_t)j + 1] - c[1];
    o.s1[2] += (double)d.xyz[3 * (size_t)j + 2] - c[2];
    const size_t at = 3 * (size_t)a.inv[j];
    double u[3] = {(double)a.nrm[at], (double)a.nrm[at + 1], (double)a.nrm[at + 2]};
    if (P.on) {
      const double ns[3] = {u[0], u[1], u[2]};
#pragma unroll
      for (int r = 0; r < 3; ++r) u[r] = ((double)P.T[3 * r] * ns[0] + (double)P.T[3 * r + 1] * ns[1]) + (double)P.T[3 * r + 2] * ns[2];
    }
    o.s2[0] += u[0] * u[0]; o.s2[1] += u[0] * u[1]; o.s2[2] += u[0] * u[2];
    o.s2[3] += u[1] * u[1]; o.s2[4] += u[1] * u[2]; o.s2[5] += u[2] * u[2];
    ++n;
  }
  o.count = n;
  out[pos[d.begin + i]] = o;
}

// one lane per contribution voxel: is its key in the resident table?  is_new for the flag scan, at = its voxel if not
static __global__ __launch_bounds__(256) void count_new_kernel(const Contrib* __restrict__ con, uint32_t nc,
                                                               const unsigned long long* __restrict__ hkey,
                                                               const uint32_t* __restrict__ hval, uint32_t mask,
                                                               uint32_t* __restrict__ is_new, uint32_t* __restrict__ at,
                                                               Counters* __restrict__ ctr) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t pts = 0;
  if (c < nc) {
    const unsigned long long k = con[c].key;
    pts = con[c].count;
    uint32_t s = voxmap::hash_slot(k, mask), found = NO_VOXEL, fresh = 0u, step = 0;
    for (; step <= mask; ++step) {
      const unsigned long long hk = hkey[s];
      if (hk == k) {
        found = hval[s];
        break;
      }
      if (hk == KEY_NONE) {
        fresh = 1u;
        break;
      }
      s = (s + 1) & mask;
    }
    if (step > mask) ctr->err = 1u;
    is_new[c] = fresh;
    at[c] = found;
  }
  const uint32_t w = wave_sum(pts);
  if ((threadIdx.x & 63) == 0 && w) atomicAdd(&ctr->points, (unsigned long long)w);
}

// one lane per contribution voxel; rank[c]: how many new keys stand before c (the flag scan of is_new)
static __global__ __launch_bounds__(256) void merge_kernel(const Contrib* __restrict__ con, uint32_t nc, const uint32_t* __restrict__ is_new,
                                                           const uint32_t* __restrict__ rank, const uint32_t* __restrict__ at,
                                                           uint32_t n_voxels, uint32_t capacity, uint32_t stamp, double res,
                                                           unsigned long long* __restrict__ hkey, uint32_t* __restrict__ hval, uint32_t mask,
                                                           Voxel* __restrict__ vox, Sums* __restrict__ sums, uint32_t* __restrict__ stamps,
                                                           Counters* __restrict__ ctr) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nc) return;
  const Contrib in = con[c];
  uint32_t v;
  Sums S;
  uint32_t N = in.count;
  if (is_new[c]) {
    v = n_voxels + rank[c];
    if (v >= capacity) {
      ctr->err = 1u;
      return;
    }
    uint32_t s = voxmap::hash_slot(in.key, mask), step = 0;
    for (; step <= mask; ++step) {
      if (atomicCAS(&hkey[s], KEY_NONE, in.key) == KEY_NONE) break;
      s = (s + 1) & mask;
    }
    if (step > mask) {
      ctr->err = 1u;
      return;
    }
    hval[s] = v;
#pragma unroll
    for (int q = 0; q < 3; ++q) S.s1[q] = in.s1[q];
#pragma unroll
    for (int q = 0; q < 6; ++q) S.s2[q] = in.s2[q];
  } else {
    v = at[c];
    if (v >= n_voxels) {
      ctr->err = 1u;
      return;
    }
    S = sums[v];
    N += vox[v].count;
#pragma unroll
    for (int q = 0; q < 3; ++q) S.s1[q] += in.s1[q];
#pragma unroll
    for (int q = 0; q < 6; ++q) S.s2[q] += in.s2[q];
  }
  double corner[3];
  corner_of(in.key, res, corner);
  const double nd = (double)N;
  Voxel out;
  out.key = in.key;
  out.count = N;
  out.valid = 1u;
#pragma unroll
  for (int q = 0; q < 3; ++q) out.mean[q] = corner[q] + S.s1[q] / nd;
#pragma unroll
  for (int q = 0; q < 6; ++q) out.nn[q] = S.s2[q] / nd;
  vox[v] = out;
  sums[v] = S;
  stamps[v] = stamp;
}

// keep[v] = 1 for a voxel neither rule removes.  center / max_dist: the fp32 values widened; dist_on, age_on: the rules
static __global__ __launch_bounds__(256) void prune_flags_kernel(const Voxel* __restrict__ vox, const uint32_t* __restrict__ stamps,
                                                                 uint32_t n_voxels, bool dist_on, double cx, double cy, double cz,
                                                                 double max_d2, uint32_t max_age /* 0: off */, uint32_t n_inserts,
                                                                 uint32_t* __restrict__ keep, Counters* __restrict__ ctr) {
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t gone_pts = 0;
  if (v < n_voxels) {
    bool gone = false;
    if (dist_on) {
      const double dx = vox[v].mean[0] - cx, dy = vox[v].mean[1] - cy, dz = vox[v].mean[2] - cz;
      gone = (dx * dx + dy * dy) + dz * dz > max_d2;
    }
    if (max_age > 0u && n_inserts - stamps[v] > max_age) gone = true;
    keep[v] = gone ? 0u : 1u;
    if (gone) gone_pts = vox[v].count;
  }
  // (a voxel's count can pass 2^32 / 64 only in a map of more than 2^26 points per voxel: the wave's sum is taken in 64 bits)
  unsigned long long w = gone_pts;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) w += __shfl_down(w, o, 64);
  if ((threadIdx.x & 63) == 0 && w) atomicAdd(&ctr->points, w);
}

// survivors to their rank among the survivors, values and stamps as they are
static __global__ __launch_bounds__(256) void compact_kernel(const Voxel* __restrict__ vox, const Sums* __restrict__ sums,
                                                             const uint32_t* __restrict__ stamps, uint32_t n_voxels,
                                                             const uint32_t* __restrict__ keep, const uint32_t* __restrict__ rank,
                                                             Voxel* __restrict__ vox_out, Sums* __restrict__ sums_out,
                                                             uint32_t* __restrict__ stamps_out) {
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n_voxels || !keep[v]) return;
  const uint32_t r = rank[v];
  vox_out[r] = vox[v];
  sums_out[r] = sums[v];
  stamps_out[r] = stamps[v];
}

}  // namespace vmap
}  // namespace gloc
