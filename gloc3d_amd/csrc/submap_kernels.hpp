// submap_kernels.hpp -- local submaps on gfx950 (gloc_scan_store_add_submap[s]): resident scans brought into one frame by
// their poses and thinned by an exact voxel grid.  The executable contract is tests/submap_ref.py, bit for bit.
//
//   member_keys_kernel   (member, point): transform in the fixed un-fused fp32 order, voxel key, the point's place in the
//                        concatenation of the group's members -- every member's 12 B/point read once --, and the bounds of
//                        the work-group's cells
//   bounds_reduce_kernel one work-group: the bounds of the group's cells from those partials
//   narrow_keys_kernel   the keys again, in place, relative to those bounds with just the bits each axis needs: the same
//                        (kx, ky, kz) order in about 30 bits for lidar submaps where the 3 x 21-bit key has 63: half the radix passes
//   segmented radix sort by that key (seg_sort.hpp, stable), one segment per submap
//   voxmap::cell_flags_kernel, voxmap::scan_flags (voxel_map*.hpp): a run of equal keys = a cell, cells numbered
//   run_stats_kernel     one thread per run: the fp64 sum in (member position, point index) order -- the order the stable
//                        sort leaves a run in --, the centroid, the members seen, the keep flag
//   voxmap::scan_flags over the keep flags, voxmap::cell_first_kernel twice (cells and kept cells of every submap)
//   compact_kernel       the kept centroids into per-submap packed xyz
//
// Every kernel takes the member or the submap from blockIdx.y and a descriptor table: the launch count does not depend
// on how many submaps a group holds.  Nothing here depends on the order work-groups run in, and no float is ever added
// by an atomic: the bits are those of the ordered sum whatever the batch a submap is built in.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "voxel_map_kernels.hpp"

namespace gloc {
namespace submap {

struct Member {  // one member scan of one submap of the group
  const float* xyz;  // the scan's original-order packed xyz
  uint32_t n;
  uint32_t begin;  // its slice of the group's concatenated arrays
  float T[12];     // rows 0..2 of the 4x4 pose, row-major: member frame -> submap frame
  uint32_t pad_[2];
};

__device__ __forceinline__ bool finite3(float x, float y, float z) {
  return fabsf(x) <= 3.4028234e38f && fabsf(y) <= 3.4028234e38f && fabsf(z) <= 3.4028234e38f;  // (false for NaN)
}

// q = T p with every product and sum rounded on its own, k = floor(q / leaf) as voxmap::cell_keys_kernel computes it; a
// point that is skipped (non-finite, beyond max_range of its own sensor, outside the key range) gets KEY_NONE, which
// sorts behind every cell.  mr2 < 0: no range limit.  part[work-group]: [min kx, ky, kz, max kx, ky, kz] of its cells, biased
// as in the key (~0 / 0: none) -- partials and no atomics: six of them per work-group on one cache line took longer than
// everything else the kernel does, as they did in pack_bbox_kernel (scan_store.hip).
static __global__ __launch_bounds__(256) void member_keys_kernel(const Member* __restrict__ mem, float inv, float mr2,
                                                                 float* __restrict__ q, unsigned long long* __restrict__ key,
                                                                 uint32_t* __restrict__ val, uint32_t* __restrict__ part) {
  __shared__ uint32_t red[4][6];
  const Member& m = mem[blockIdx.y];
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  const bool in = i < m.n;
  bool ok = in;
  long long k[3] = {0, 0, 0};
  if (in) {
    const float x = m.xyz[3 * (size_t)i], y = m.xyz[3 * (size_t)i + 1], z = m.xyz[3 * (size_t)i + 2];
    ok = finite3(x, y, z);
    if (mr2 >= 0.f) {
      const float r2 = __fadd_rn(__fadd_rn(__fmul_rn(x, x), __fmul_rn(y, y)), __fmul_rn(z, z));
      ok = ok && !(r2 > mr2);
    }
    float p[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float* T = m.T + 4 * a;
      p[a] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(T[0], x), __fmul_rn(T[1], y)), __fmul_rn(T[2], z)), T[3]);
      const float f = floorf(__fmul_rn(p[a], inv));
      ok = ok && fabsf(f) < (float)voxmap::KEY_BIAS;  // (false for NaN; an infinite q gives an infinite or NaN f)
      k[a] = ok ? (long long)f : 0;
    }
    const size_t g = (size_t)m.begin + i;
    q[3 * g] = p[0];
    q[3 * g + 1] = p[1];
    q[3 * g + 2] = p[2];
    key[g] = ok ? voxmap::pack_key(k[0], k[1], k[2]) : voxmap::KEY_NONE;
    val[g] = (uint32_t)g;
  }
  // the work-group's cell bounds: lanes, then waves
  uint32_t lo[3], hi[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    lo[a] = ok ? (uint32_t)(k[a] + voxmap::KEY_BIAS) : 0xFFFFFFFFu;
    hi[a] = ok ? (uint32_t)(k[a] + voxmap::KEY_BIAS) : 0u;
    for (int o = 32; o > 0; o >>= 1) {
      const uint32_t l2 = __shfl_xor(lo[a], o), h2 = __shfl_xor(hi[a], o);
      lo[a] = l2 < lo[a] ? l2 : lo[a];
      hi[a] = h2 > hi[a] ? h2 : hi[a];
    }
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      red[threadIdx.x >> 6][a] = lo[a];
      red[threadIdx.x >> 6][3 + a] = hi[a];
    }
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    uint32_t v = red[0][threadIdx.x];
    for (int w = 1; w < 4; ++w) {
      const uint32_t x = red[w][threadIdx.x];
      v = threadIdx.x < 3 ? (x < v ? x : v) : (x > v ? x : v);
    }
    part[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 6 + threadIdx.x] = v;
  }
}

static __global__ __launch_bounds__(1024) void bounds_reduce_kernel(const uint32_t* __restrict__ part, uint32_t n_part,
                                                                    uint32_t* __restrict__ bounds) {
  __shared__ uint32_t red[16][6];
  uint32_t lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0u, 0u, 0u};
  for (uint32_t b = threadIdx.x; b < n_part; b += 1024)
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const uint32_t l = part[6 * (size_t)b + a], h = part[6 * (size_t)b + 3 + a];
      lo[a] = l < lo[a] ? l : lo[a];
      hi[a] = h > hi[a] ? h : hi[a];
    }
#pragma unroll
  for (int a = 0; a < 3; ++a)
    for (int o = 32; o > 0; o >>= 1) {
      const uint32_t l2 = __shfl_xor(lo[a], o), h2 = __shfl_xor(hi[a], o);
      lo[a] = l2 < lo[a] ? l2 : lo[a];
      hi[a] = h2 > hi[a] ? h2 : hi[a];
    }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      red[threadIdx.x >> 6][a] = lo[a];
      red[threadIdx.x >> 6][3 + a] = hi[a];
    }
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    uint32_t v = red[0][threadIdx.x];
    for (int w = 1; w < 16; ++w) {
      const uint32_t x = red[w][threadIdx.x];
      v = threadIdx.x < 3 ? (x < v ? x : v) : (x > v ? x : v);
    }
    bounds[threadIdx.x] = v;
  }
}

// The keys of the group again, in place: (kx - min kx, ky - min ky, kz - min kz) packed with by + bz, bz and 0 bits to
// the right of them, where b? is the number of bits the group's extent along that axis needs.  Ascending keys are still
// ascending (kx, ky, kz); KEY_NONE stays all ones, above every cell in the bits the sort looks at (bx + by + bz + 1).
static __global__ __launch_bounds__(256) void narrow_keys_kernel(unsigned long long* __restrict__ key, uint32_t n, uint32_t ox, uint32_t oy,
                                                                 uint32_t oz, uint32_t by, uint32_t bz) {
  const uint32_t g = blockIdx.x * 256 + threadIdx.x;
  if (g >= n) return;
  const unsigned long long k = key[g];
  if (k == voxmap::KEY_NONE) return;
  const unsigned long long kx = (k >> 42) & 0x1FFFFFull, ky = (k >> 21) & 0x1FFFFFull, kz = k & 0x1FFFFFull;
  key[g] = ((kx - ox) << (by + bz)) | ((ky - oy) << bz) | (kz - oz);
}

// One thread per run of equal keys (flag = 1 at its first element, pos = the cell's number within the group).  The stable
// sort left the run in ascending order of the concatenated index = (member position, point index): the fp64 sum walks it
// in that order, and the members seen are counted by the slices the indices fall into (mbegin: the group's member slices,
// ascending, n_mem + 1 entries; an empty member shares its begin with the next one and is never found).  keep[g] = 1
// where the run starts a cell that stays.  used[submap] = points of the submap with a key (they sort in front of the rest).
static __global__ __launch_bounds__(256) void run_stats_kernel(const voxmap::TgtDesc* __restrict__ seg,
                                                               const unsigned long long* __restrict__ key,
                                                               const uint32_t* __restrict__ val, const uint32_t* __restrict__ flag,
                                                               const uint32_t* __restrict__ pos, const float* __restrict__ q,
                                                               const uint32_t* __restrict__ mbegin, uint32_t n_mem,
                                                               uint32_t min_points, uint32_t min_scans, float* __restrict__ cent,
                                                               uint32_t* __restrict__ keep, uint32_t* __restrict__ used) {
  const voxmap::TgtDesc d = seg[blockIdx.y];
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= d.n) return;
  const size_t g = (size_t)d.begin + i;
  const unsigned long long k = key[g];
  if (k == voxmap::KEY_NONE) {
    if (i == 0 || key[g - 1] != voxmap::KEY_NONE) used[blockIdx.y] = i;
  } else if (i + 1 == d.n) {
    used[blockIdx.y] = d.n;
  }
  if (!flag[g]) {
    keep[g] = 0u;
    return;
  }
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  uint32_t count = 0, scans = 0, mend = 0;
  for (uint32_t j = i; j < d.n && key[(size_t)d.begin + j] == k; ++j) {
    const uint32_t v = val[(size_t)d.begin + j];
    if (v >= mend) {  // the run has moved on to another member: the last slice that begins at or before v
      uint32_t lo = 0, hi = n_mem;
      while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (mbegin[mid] <= v) lo = mid; else hi = mid;
      }
      mend = mbegin[lo + 1];
      ++scans;
    }
    s0 += (double)q[3 * (size_t)v];
    s1 += (double)q[3 * (size_t)v + 1];
    s2 += (double)q[3 * (size_t)v + 2];
    ++count;
  }
  const size_t c = pos[g];
  const double cn = (double)count;
  cent[3 * c] = (float)(s0 / cn);
  cent[3 * c + 1] = (float)(s1 / cn);
  cent[3 * c + 2] = (float)(s2 / cn);
  keep[g] = (count >= min_points && scans >= min_scans) ? 1u : 0u;
}

// kept cell -> its place among the kept cells of the group (kpos: the scanned keep flags); a submap's kept cells are
// consecutive there, in cell order: its packed xyz
static __global__ __launch_bounds__(256) void compact_kernel(const uint32_t* __restrict__ keep, const uint32_t* __restrict__ pos,
                                                             const uint32_t* __restrict__ kpos, const float* __restrict__ cent,
                                                             uint32_t n, float* __restrict__ out) {
  const uint32_t g = blockIdx.x * 256 + threadIdx.x;
  if (g >= n || !keep[g]) return;
  const size_t c = pos[g], o = kpos[g];
  out[3 * o] = cent[3 * c];
  out[3 * o + 1] = cent[3 * c + 1];
  out[3 * o + 2] = cent[3 * c + 2];
}

}  // namespace submap
}  // namespace gloc
