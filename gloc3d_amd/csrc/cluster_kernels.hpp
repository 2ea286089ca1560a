// cluster_kernels.hpp -- Euclidean clusters and outlier filters of a resident scan (E1 - E7 of include/gloc3d.h;
// tests/cluster_ref.py restates them).  Compiled in cluster.hip.
//
//   cluster_link_kernel     radius_self_kernel's traversal without lists and without LDS (the shape of iss_nms_kernel): the
//                           store's sorted copy in chunks of 64 with their boxes, a wave per chunk of sources, a ballot over
//                           the chunk boxes against r2, candidates read lane by lane.  Every pair within r2 whose other
//                           ORIGINAL index is the smaller one is united in parent[] (by original index), so each edge is
//                           united once, from its larger end.
//   union-find              lock-free, after ECL-CC (Jaiganesh, Burtscher, HPDC 2018): find with pointer halving, the larger
//                           root hooked under the smaller by atomicCAS, a failed hook goes on from the value the CAS
//                           returned.  Invariant: parent[x] <= x always, and a vertex that has once had a smaller parent
//                           never is a root again.  Hence
//                             - every walk descends strictly, so find ends whatever it reads and a failed hook moves its
//                               end strictly down: the retries are bounded by the index, not by another wave's progress.
//                               No lane waits for anything: no spin, no barrier across waves.
//                             - the smallest index of a component can only be a root, a tree has one root and a component
//                               ends as one tree: the final root is the minimum (E2) whatever the schedule.
//                           All of parent[] is read and written with device-scope atomics inside the link kernel -- relaxed
//                           loads, atomicCAS, and the halving as an atomicMin, which can only move a pointer down to another
//                           vertex of the same tree: nothing depends on a cache being fresh, a stale value is an older
//                           ancestor and the CAS, which decides, sees the truth.  A lane carries the last root it reached
//                           for its own point from edge to edge, and the roots of a chunk's 64 candidates are found once
//                           per chunk, side by side: an edge whose ends show the same root touches no memory.
//   cluster_flatten_kernel  root[i] = find(i) (plain loads: a launch of its own), NONE for a non-finite point; the sizes by
//                           integer atomicAdd on the root.
//   cluster_keys_kernel, segmented radix sort (seg_sort.hpp, stable), cluster_run_sums_kernel, cluster_figures_kernel:
//                           E4's sums in (cluster, upload index) order -- a thread per run of 64 points, then a wave per
//                           kept cluster over its runs' sums (wave_seq_add), every addition in the stated order, never
//                           by an atomic.
//   *_flags_kernel          a filter stage's survivors (E5 - E7) as byte flags; ground::select_flagged makes their ascending
//                           index list (stable, tiled); gather_rows_kernel the rows of a list.
//   sor_mean_kernel, sor_run_sums_kernel, sor_total_kernel  E6: m_i per point, then mu and sigma in the same two levels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ground_normals.hpp"
#include "math3.hpp"
#include "scan_index.hpp"

namespace gloc {
namespace cluster {

using reg::f32x4;

constexpr int CHUNK = ground::LIST_CHUNK;  // points per chunk of the sorted copy (one box each)
constexpr uint32_t NONE = 0xFFFFFFFFu;

__device__ __forceinline__ float lane_f(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

__device__ __forceinline__ bool finite3(float x, float y, float z) {
  return fabsf(x) <= 3.4028234e38f && fabsf(y) <= 3.4028234e38f && fabsf(z) <= 3.4028234e38f;  // (false for NaN)
}

__device__ __forceinline__ uint32_t parent_of(const uint32_t* parent, uint32_t x) {
  return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// From x down to a vertex that read as its own parent; on the way every vertex passed is pointed at its grandparent.
__device__ inline uint32_t find_root(uint32_t* parent, uint32_t x) {
  uint32_t p = parent_of(parent, x);
  while (p < x) {
    const uint32_t g = parent_of(parent, p);
    if (g < p) atomicMin(parent + x, g);
    x = p;
    p = g;
  }
  return x;
}

// Unites the trees of a and b; returns a vertex both are now under (their root at the time of the hook).
__device__ inline uint32_t unite(uint32_t* parent, uint32_t a, uint32_t b) {
  for (;;) {
    a = find_root(parent, a);
    b = find_root(parent, b);
    if (a == b) return a;
    const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
    const uint32_t old = atomicCAS(parent + hi, hi, lo);
    if (old == hi) return lo;
    a = old;  // (hi has a parent by now, below it: on from there)
    b = lo;
  }
}

__global__ __launch_bounds__(256) void cluster_init_kernel(uint32_t* __restrict__ parent, uint32_t* __restrict__ csize, uint32_t n) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  parent[i] = i;
  csize[i] = 0u;
}

// Four independent waves per work-group, one chunk of sources each (no LDS, no barrier).  parent [m] by ORIGINAL index.
__global__ __launch_bounds__(256) void cluster_link_kernel(const f32x4* __restrict__ spts, uint32_t m, const f32x4* __restrict__ box_lo,
                                                            const f32x4* __restrict__ box_hi, uint32_t nchunks, float r2,
                                                            uint32_t* __restrict__ parent) {
  const int lane = threadIdx.x & 63;
  const uint32_t own = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (own >= nchunks) return;  // (the whole wave)
  const uint32_t si = own * CHUNK + lane;
  const bool valid = si < m;
  const f32x4 p = spts[valid ? si : m - 1];
  const uint32_t po = __float_as_uint(p.w);
  const bool live = valid && po < m && finite3(p.x, p.y, p.z);  // (a non-finite point is a vertex of nothing)
  uint32_t mine = po;  // the last root reached for this lane's point
  auto eval_chunk = [&](uint32_t c) {
    const uint32_t j = c * CHUNK + lane;
    f32x4 v = {reg::NN_FAR, reg::NN_FAR, reg::NN_FAR, __uint_as_float(NONE)};
    if (j < m) {
      v = spts[j];
      if (!finite3(v.x, v.y, v.z)) v.x = __builtin_nanf("");  // its distance to anything is a NaN, inside no r2
    }
    // The roots of the chunk's 64 candidates, found once per chunk with the lanes side by side, and this lane's own again:
    // an edge whose two ends show the same root costs no memory access at all, and in a dense scan that is nearly every
    // edge (a point has hundreds of neighbours and needs one link).  An edge that is united starts from the candidate's
    // root as found here: a vertex of the candidate's tree, whatever has happened since.
    const uint32_t vo = __float_as_uint(v.w);
    uint32_t vr = NONE;
    if (vo < m && v.x == v.x) vr = find_root(parent, vo);
    if (live) mine = find_root(parent, mine);
    const int lim = (int)((m - c * CHUNK) < (uint32_t)CHUNK ? (m - c * CHUNK) : (uint32_t)CHUNK);
    for (int t = 0; t < CHUNK; t += 8) {
      float d[8];
      uint32_t o[8], ro[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        d[u] = reg::dist2(p.x, p.y, p.z, lane_f(v.x, t + u), lane_f(v.y, t + u), lane_f(v.z, t + u));
        o[u] = __float_as_uint(lane_f(v.w, t + u));
        ro[u] = (uint32_t)__builtin_amdgcn_readlane((int)vr, t + u);
      }
      const float dm = fminf(fminf(fminf(d[0], d[1]), fminf(d[2], d[3])), fminf(fminf(d[4], d[5]), fminf(d[6], d[7])));
      if (live && dm <= r2) {
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (t + u < lim && d[u] <= r2 && o[u] < po && ro[u] != mine) mine = unite(parent, mine, ro[u]);
      }
    }
  };
  if (!__any(live)) return;
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
      const bool need = live && reg::box_lb(p.x, p.y, p.z, lo, hi) <= r2;  // <=: a point at exactly r is inside
      if (!__any(need)) continue;
      eval_chunk(c0 + b);
    }
  }
}

// xyz [n][3] in upload order.  root [n]; csize [n], zeroed: the size of a component at its root.  The lanes of a wave that
// reached the same root add once between them: upload order is ray order, a wave's 64 points mostly share a component,
// and 78 000 single adds to one word took 0.89 ms of a 1.9-ms call on a bench-sized scan where these take 0.02.
__global__ __launch_bounds__(256) void cluster_flatten_kernel(const float* __restrict__ xyz, uint32_t n, const uint32_t* __restrict__ parent,
                                                               uint32_t* __restrict__ root, uint32_t* __restrict__ csize) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  uint32_t r = NONE;
  if (i < n && finite3(xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2])) {
    r = i;
    for (uint32_t p = parent[r]; p < r; p = parent[r]) r = p;
  }
  if (i < n) root[i] = r;
  unsigned long long todo = __ballot(r != NONE);
  while (todo) {  // (every lane of the wave is here)
    const int l = __ffsll((long long)todo) - 1;
    const uint32_t rl = (uint32_t)__builtin_amdgcn_readlane((int)r, l);
    const unsigned long long same = __ballot(r == rl) & todo;
    if (lane == l) atomicAdd(csize + rl, (uint32_t)__popcll(same));
    todo &= ~same;
  }
}

// sort keys of E4: the cluster of a point, n_kept for a point of no kept cluster (behind every cluster)
__global__ __launch_bounds__(256) void cluster_keys_kernel(const uint32_t* __restrict__ label, uint32_t n, uint32_t n_kept,
                                                            uint32_t* __restrict__ key, uint32_t* __restrict__ val) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t c = label[i];
  key[i] = c < n_kept ? c : n_kept;
  val[i] = i;
}

// ---- ordered fp64 sums ----------------------------------------------------------------------------------------------------------
// E4 and E6 state their sums in two levels: the terms, in ascending upload index, are cut into RUNS of 64; a run's terms
// are added one by one from +0.0, and the runs' sums are added one by one, in run order, from +0.0.  A thread adds one run
// (the runs side by side), then one wave adds the runs' sums: a chain of n / 64 additions instead of n.  A term that is
// left out (past the end, a non-finite point) is added as +0.0, which changes no sum that started from +0.0.
constexpr int RUN = 64;

__device__ __forceinline__ double lane_d(double v, int l) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(v);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)u, l), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(u >> 32), l);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// s + v(lane 0) + v(lane 1) + ... + v(lane 63), added one by one in that order; the same in every lane
__device__ __forceinline__ double wave_seq_add(double s, double v) {
#pragma unroll
  for (int l = 0; l < 64; ++l) s += lane_d(v, l);
  return s;
}

// E4, first level.  The points of kept cluster c are val[first[c] .. first[c + 1]), ascending upload index (the stable
// sort by cluster left them so); its runs are runs [runfirst[c], runfirst[c + 1]) of the launch.  One thread per run:
// psum [runs][3] the run's sums, pmin / pmax [runs][3] its corners as order-preserving integers (f2ord: -0 below +0).
__global__ __launch_bounds__(256) void cluster_run_sums_kernel(const float* __restrict__ xyz, const uint32_t* __restrict__ val,
                                                                const uint32_t* __restrict__ first, const uint32_t* __restrict__ runfirst,
                                                                uint32_t n_kept, double* __restrict__ psum, uint32_t* __restrict__ pmin,
                                                                uint32_t* __restrict__ pmax) {
  const uint32_t g = blockIdx.x * 256 + threadIdx.x;
  if (g >= runfirst[n_kept]) return;
  uint32_t c = 0, hi = n_kept;  // the last cluster whose first run is at or before g
  while (hi - c > 1) {
    const uint32_t mid = (c + hi) >> 1;
    if (runfirst[mid] <= g) c = mid; else hi = mid;
  }
  const uint32_t b = first[c] + (g - runfirst[c]) * RUN, e = min(b + (uint32_t)RUN, first[c + 1]);
  double s[3] = {0.0, 0.0, 0.0};
  uint32_t mn[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, mx[3] = {0u, 0u, 0u};
  for (uint32_t k = b; k < e; ++k) {
    const size_t i = val[k];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float q = xyz[3 * i + a];
      s[a] += (double)q;
      const uint32_t u = reg::f2ord(q);
      mn[a] = u < mn[a] ? u : mn[a];
      mx[a] = u > mx[a] ? u : mx[a];
    }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    psum[3 * (size_t)g + a] = s[a];
    pmin[3 * (size_t)g + a] = mn[a];
    pmax[3 * (size_t)g + a] = mx[a];
  }
}

// E4, second level.  One wave per kept cluster, four per work-group.  cent [K][3], lo / hi [K][3].
__global__ __launch_bounds__(256) void cluster_figures_kernel(const uint32_t* __restrict__ first, const uint32_t* __restrict__ runfirst,
                                                               uint32_t n_kept, const double* __restrict__ psum, const uint32_t* __restrict__ pmin,
                                                               const uint32_t* __restrict__ pmax, double* __restrict__ cent, float* __restrict__ lo,
                                                               float* __restrict__ hi) {
  const int lane = threadIdx.x & 63;
  const uint32_t c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= n_kept) return;  // (the whole wave)
  const uint32_t b = runfirst[c], e = runfirst[c + 1];
  double s[3] = {0.0, 0.0, 0.0};
  uint32_t mn[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, mx[3] = {0u, 0u, 0u};
  for (uint32_t g0 = b; g0 < e; g0 += 64) {
    const uint32_t g = g0 + lane;
    const bool ok = g < e;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      s[a] = wave_seq_add(s[a], ok ? psum[3 * (size_t)g + a] : 0.0);
      const uint32_t l = ok ? pmin[3 * (size_t)g + a] : 0xFFFFFFFFu, h = ok ? pmax[3 * (size_t)g + a] : 0u;
      mn[a] = l < mn[a] ? l : mn[a];
      mx[a] = h > mx[a] ? h : mx[a];
    }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a)
    for (int o = 32; o > 0; o >>= 1) {
      const uint32_t l2 = __shfl_xor(mn[a], o), h2 = __shfl_xor(mx[a], o);
      mn[a] = l2 < mn[a] ? l2 : mn[a];
      mx[a] = h2 > mx[a] ? h2 : mx[a];
    }
  if (lane < 3) {
    const double cn = (double)(first[c + 1] - first[c]);
    const double sum = lane == 0 ? s[0] : lane == 1 ? s[1] : s[2];
    const uint32_t l = lane == 0 ? mn[0] : lane == 1 ? mn[1] : mn[2], h = lane == 0 ? mx[0] : lane == 1 ? mx[1] : mx[2];
    cent[3 * (size_t)c + lane] = sum / cn;
    lo[3 * (size_t)c + lane] = reg::ord2f(l);
    hi[3 * (size_t)c + lane] = reg::ord2f(h);
  }
}

// ---- the filter stages: byte flags of the survivors, in upload order ---------------------------------------------------------

// E7's range crop.  min2 / max2: the fp32 squares, negative = off.
__global__ __launch_bounds__(256) void range_flags_kernel(const float* __restrict__ xyz, uint32_t n, float min2, float max2,
                                                           uint8_t* __restrict__ flag) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float x = xyz[3 * (size_t)i], y = xyz[3 * (size_t)i + 1], z = xyz[3 * (size_t)i + 2];
  const float r2 = __fadd_rn(__fadd_rn(__fmul_rn(x, x), __fmul_rn(y, y)), __fmul_rn(z, z));
  bool ok = finite3(x, y, z);
  if (max2 >= 0.f) ok = ok && !(r2 > max2);
  if (min2 >= 0.f) ok = ok && !(r2 < min2);
  flag[i] = ok ? 1 : 0;
}

// E5.  count [n]: R1's whole-neighbourhood counts, self included, by upload index.
__global__ __launch_bounds__(256) void ror_flags_kernel(const float* __restrict__ xyz, uint32_t n, const uint32_t* __restrict__ count,
                                                         uint32_t min_neighbors, uint8_t* __restrict__ flag) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t c = count[i];
  flag[i] = (finite3(xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2]) && c >= 1u && c - 1u >= min_neighbors) ? 1 : 0;
}

// E6's m_i.  nb / nd2 [n][W]: the k-NN lists by upload index, of which the first mean_k + 1 entries are looked at
// (W >= mean_k + 1; a longer list begins with the shorter one).  mean [n], 0 and fin = 0 for a non-finite point.
__global__ __launch_bounds__(256) void sor_mean_kernel(const float* __restrict__ xyz, uint32_t n, const uint32_t* __restrict__ nb,
                                                        const float* __restrict__ nd2, int W, int mean_k, double* __restrict__ mean,
                                                        uint8_t* __restrict__ fin) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const bool f = finite3(xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2]);
  double s = 0.0;
  int taken = 0;
  if (f)
    for (int e = 0; e <= mean_k; ++e) {
      if (taken == mean_k || nb[(size_t)i * W + e] == i) continue;
      s += sqrt((double)nd2[(size_t)i * W + e]);
      ++taken;
    }
  mean[i] = f ? s / (double)mean_k : 0.0;
  fin[i] = f ? 1 : 0;
}

// E6's sums, first level: one thread per run of 64 consecutive upload indices.  mu null: the run's sum of m_i and its
// count of finite points; else its sum of (m_i - *mu)^2.
__global__ __launch_bounds__(256) void sor_run_sums_kernel(const double* __restrict__ mean, const uint8_t* __restrict__ fin, uint32_t n,
                                                            const double* __restrict__ mu, double* __restrict__ psum, uint32_t* __restrict__ pcnt) {
  const uint32_t g = blockIdx.x * 256 + threadIdx.x;
  if (g >= (n + RUN - 1) / RUN) return;
  const uint32_t b = g * RUN, e = min(b + (uint32_t)RUN, n);
  const double m0 = mu ? *mu : 0.0;
  double s = 0.0;
  uint32_t cnt = 0;
  for (uint32_t i = b; i < e; ++i) {
    if (!fin[i]) continue;
    const double d = mean[i] - m0;
    s += mu ? d * d : mean[i];
    ++cnt;
  }
  psum[g] = s;
  if (!mu) pcnt[g] = cnt;
}

// ... second level: ONE wave adds the runs' sums in run order.  pass 0: stats[0] = mu, stats[2] = (double)N; pass 1:
// stats[1] = sigma = sqrt(sum / N).
__global__ __launch_bounds__(64) void sor_total_kernel(const double* __restrict__ psum, const uint32_t* __restrict__ pcnt, uint32_t runs, int pass,
                                                        double* __restrict__ stats) {
  const uint32_t lane = threadIdx.x;
  double s = 0.0;
  uint32_t N = 0;
  for (uint32_t g0 = 0; g0 < runs; g0 += 64) {
    const bool ok = g0 + lane < runs;
    s = wave_seq_add(s, ok ? psum[g0 + lane] : 0.0);
    if (pass == 0 && ok) N += pcnt[g0 + lane];
  }
  if (pass == 0) {
    for (int o = 32; o > 0; o >>= 1) N += __shfl_xor(N, o);
    if (lane == 0) {
      stats[0] = s / (double)N;
      stats[2] = (double)N;
    }
  } else if (lane == 0) {
    stats[1] = sqrt(s / stats[2]);
  }
}

__global__ __launch_bounds__(256) void sor_flags_kernel(const double* __restrict__ mean, const uint8_t* __restrict__ fin, uint32_t n,
                                                         const double* __restrict__ stats, float std_mul, uint8_t* __restrict__ flag) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double thr = stats[0] + (double)std_mul * stats[1];
  flag[i] = (fin[i] && mean[i] <= thr) ? 1 : 0;
}

__global__ __launch_bounds__(256) void label_flags_kernel(const uint32_t* __restrict__ label, uint32_t n, uint8_t* __restrict__ flag) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  flag[i] = label[i] != NONE ? 1 : 0;
}

// out[r] = row idx[r] of xyz (every idx[r] < the rows of xyz: the caller's to see to)
__global__ __launch_bounds__(256) void gather_rows_kernel(const float* __restrict__ xyz, const uint32_t* __restrict__ idx, uint32_t m,
                                                           float* __restrict__ out) {
  const uint32_t r = blockIdx.x * 256 + threadIdx.x;
  if (r >= m) return;
  const size_t i = idx[r];
  out[3 * (size_t)r] = xyz[3 * i];
  out[3 * (size_t)r + 1] = xyz[3 * i + 1];
  out[3 * (size_t)r + 2] = xyz[3 * i + 2];
}

}  // namespace cluster
}  // namespace gloc
