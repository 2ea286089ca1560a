// fpfh_kernels.hpp -- FPFH descriptors of a resident scan and the brute-force descriptor matcher behind the feature-based
// global registration (gloc_reg_fpfh_*; include/gloc3d.h has the definitions, tests/fpfh_ref.py the float64 restatement).
// Compiled in fpfh.hip.
//   F1 spfh_kernel        thread per point: Darboux-frame pair features against the point's k-NN list, 3 x 11 counts
//   F2 fpfh_kernel        thread per point: 1/d2-weighted sum of the neighbours' SPFH, each sub-histogram rescaled to 100
//      spfh_wide_kernel / fpfh_wide_kernel  the same two over lists wider than 16 (the radius support), a wave per point
//   F3 fpfh_match_kernel  thread per source row, target rows streamed through LDS as wave-uniform broadcasts; the
//                         un-fused fp32 distance on packed pairs of target rows; slices of the targets folded with a
//                         64-bit atomicMin on (d2 bits, original target index)
//   F4 fpfh_pairs_kernel  the kept matches of a job, compacted in ascending source index into the RANSAC stage's pairs
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fpfh.hpp"  // MatchTask, PairJob
#include "math3.hpp"

namespace gloc {
namespace fpfh {

using reg::f32x4;

constexpr int DIM = 33;            // 3 x 11 bins
constexpr int NB = 11;
constexpr int SPFH_STRIDE = (int)SPFH_BYTES;    // bytes per point: 33 counts, the number of pairs counted, two of padding
constexpr int MATCH_TILE = (int)MATCH_TILE_ROWS;  // target rows per LDS tile
constexpr int MATCH_THREADS = 256; // source rows per work-group
constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr unsigned long long NO_KEY = ~0ull;

__device__ __forceinline__ bool finite3(float x, float y, float z) {
  return isfinite(x) && isfinite(y) && isfinite(z);
}

// Is list entry (j, d2) of point i a pair F1 counts?  (the normals are checked by the caller)
__device__ __forceinline__ bool entry_ok(uint32_t i, uint32_t j, float d2, uint32_t n) {
  return j != i && j < n && d2 > 0.f && isfinite(d2);
}

// The pair feature of F1 for point i (p, normal ni) and its list entry j (q, normal nj), both finite with non-zero normals:
// false when the pair is skipped (coincident points, dp parallel to n1), else the three bins.  fp64 from the fp32 inputs.
__device__ __forceinline__ bool pair_bins(const f32x4 p, float nix, float niy, float niz, const f32x4 q, float njx, float njy, float njz,
                                          int* b1, int* b2, int* b3) {
  const double ni[3] = {(double)nix, (double)niy, (double)niz}, nj[3] = {(double)njx, (double)njy, (double)njz};
  double dp[3] = {(double)q.x - (double)p.x, (double)q.y - (double)p.y, (double)q.z - (double)p.z};
  const double f4 = sqrt((dp[0] * dp[0] + dp[1] * dp[1]) + dp[2] * dp[2]);
  if (!(f4 > 0.0)) return false;
  const double a1 = ((ni[0] * dp[0] + ni[1] * dp[1]) + ni[2] * dp[2]) / f4;
  const double a2 = ((nj[0] * dp[0] + nj[1] * dp[1]) + nj[2] * dp[2]) / f4;
  const bool swap = acos(fmin(fabs(a1), 1.0)) > acos(fmin(fabs(a2), 1.0));
  const double* n1 = swap ? nj : ni;
  const double* n2 = swap ? ni : nj;
  const double f3 = swap ? -a2 : a1;
  if (swap) { dp[0] = -dp[0]; dp[1] = -dp[1]; dp[2] = -dp[2]; }
  double v[3] = {dp[1] * n1[2] - dp[2] * n1[1], dp[2] * n1[0] - dp[0] * n1[2], dp[0] * n1[1] - dp[1] * n1[0]};
  const double vl = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
  if (!(vl > 0.0)) return false;
  v[0] = v[0] / vl; v[1] = v[1] / vl; v[2] = v[2] / vl;
  const double w[3] = {n1[1] * v[2] - n1[2] * v[1], n1[2] * v[0] - n1[0] * v[2], n1[0] * v[1] - n1[1] * v[0]};
  const double f2 = (v[0] * n2[0] + v[1] * n2[1]) + v[2] * n2[2];
  const double f1 = atan2((w[0] * n2[0] + w[1] * n2[1]) + w[2] * n2[2], (n1[0] * n2[0] + n1[1] * n2[1]) + n1[2] * n2[2]);
  const double s1 = 11.0 * (f1 + 3.14159265358979323846) / (2.0 * 3.14159265358979323846);
  const double s2 = 11.0 * (f2 + 1.0) / 2.0, s3 = 11.0 * (f3 + 1.0) / 2.0;
  auto bin = [](double x) {
    const double f = floor(x);
    return f >= 1.0 ? (f > 10.0 ? 10 : (int)f) : 0;  // (a NaN lands in bin 0; the restatement says the same)
  };
  *b1 = bin(s1); *b2 = bin(s2); *b3 = bin(s3);
  return true;
}

__device__ __forceinline__ bool has_normal(float x, float y, float z) { return x != 0.f || y != 0.f || z != 0.f; }

// F1.  pts / nrm / lists in ORIGINAL order (the order the k-NN lists are written in).
__global__ __launch_bounds__(256) void spfh_kernel(const f32x4* __restrict__ pts, const float* __restrict__ nrm,
                                                    const uint32_t* __restrict__ nb, const float* __restrict__ nb_d2, uint32_t n, int k,
                                                    uint8_t* __restrict__ out /* [n][SPFH_STRIDE] */) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  uint32_t cnt[DIM];
#pragma unroll
  for (int b = 0; b < DIM; ++b) cnt[b] = 0;
  uint32_t used = 0;
  const f32x4 p = pts[i];
  const float nix = nrm[3 * (size_t)i], niy = nrm[3 * (size_t)i + 1], niz = nrm[3 * (size_t)i + 2];
  const bool have_i = finite3(p.x, p.y, p.z) && has_normal(nix, niy, niz);
  for (int s = 0; s < k && have_i; ++s) {
    const uint32_t j = nb[(size_t)i * k + s];
    if (!entry_ok(i, j, nb_d2[(size_t)i * k + s], n)) continue;
    const f32x4 q = pts[j];
    const float njx = nrm[3 * (size_t)j], njy = nrm[3 * (size_t)j + 1], njz = nrm[3 * (size_t)j + 2];
    if (!finite3(q.x, q.y, q.z) || !has_normal(njx, njy, njz)) continue;
    int b1, b2, b3;
    if (!pair_bins(p, nix, niy, niz, q, njx, njy, njz, &b1, &b2, &b3)) continue;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      cnt[b] += (b == b1) ? 1u : 0u;
      cnt[NB + b] += (b == b2) ? 1u : 0u;
      cnt[2 * NB + b] += (b == b3) ? 1u : 0u;
    }
    ++used;
  }
  uint8_t* o = out + (size_t)i * SPFH_STRIDE;
#pragma unroll
  for (int b = 0; b < DIM; ++b) o[b] = (uint8_t)cnt[b];
  o[33] = (uint8_t)used;
  o[34] = 0;
  o[35] = 0;
}

// F1 over wide lists (the radius support: up to 128 entries): one wave per point, a lane per list entry, so that the fp64
// pair features of a list run side by side instead of one thread crawling 128 scattered neighbours.  The counts are summed
// across the lanes by ballots -- integer sums, exact in any order -- and lane b writes byte b of the row.
__global__ __launch_bounds__(256) void spfh_wide_kernel(const f32x4* __restrict__ pts, const float* __restrict__ nrm,
                                                         const uint32_t* __restrict__ nb, const float* __restrict__ nb_d2, uint32_t n, int k,
                                                         uint8_t* __restrict__ out /* [n][SPFH_STRIDE] */) {
  const int lane = threadIdx.x & 63;
  const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;  // (the whole wave)
  const f32x4 p = pts[i];
  const float nix = nrm[3 * (size_t)i], niy = nrm[3 * (size_t)i + 1], niz = nrm[3 * (size_t)i + 2];
  const bool have_i = finite3(p.x, p.y, p.z) && has_normal(nix, niy, niz);
  uint32_t mine = 0;  // lane b < 33: count b; lane 33: the pairs counted
  for (int s0 = 0; s0 < k && have_i; s0 += 64) {
    const int s = s0 + lane;
    bool ok = false;
    int b1 = 0, b2 = 0, b3 = 0;
    if (s < k) {
      const uint32_t j = nb[(size_t)i * k + s];
      if (entry_ok(i, j, nb_d2[(size_t)i * k + s], n)) {
        const f32x4 q = pts[j];
        const float njx = nrm[3 * (size_t)j], njy = nrm[3 * (size_t)j + 1], njz = nrm[3 * (size_t)j + 2];
        if (finite3(q.x, q.y, q.z) && has_normal(njx, njy, njz)) ok = pair_bins(p, nix, niy, niz, q, njx, njy, njz, &b1, &b2, &b3);
      }
    }
    for (int b = 0; b < NB; ++b) {
      const uint32_t c1 = (uint32_t)__popcll(__ballot(ok && b1 == b)), c2 = (uint32_t)__popcll(__ballot(ok && b2 == b)),
                     c3 = (uint32_t)__popcll(__ballot(ok && b3 == b));
      if (lane == b) mine += c1;
      if (lane == NB + b) mine += c2;
      if (lane == 2 * NB + b) mine += c3;
    }
    const uint32_t u = (uint32_t)__popcll(__ballot(ok));
    if (lane == DIM) mine += u;
  }
  if (lane < SPFH_STRIDE) out[(size_t)i * SPFH_STRIDE + lane] = (uint8_t)mine;  // (lanes 34, 35: the padding, zero)
}

// F2.  out [n][DIM] in ORIGINAL order; the all-zero row = no feature.
__global__ __launch_bounds__(256) void fpfh_kernel(const uint8_t* __restrict__ spfh, const uint32_t* __restrict__ nb,
                                                    const float* __restrict__ nb_d2, uint32_t n, int k, float* __restrict__ out) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double acc[DIM];
#pragma unroll
  for (int b = 0; b < DIM; ++b) acc[b] = 0.0;
  bool any = false;
  if (spfh[(size_t)i * SPFH_STRIDE + 33] != 0) {
    for (int s = 0; s < k; ++s) {
      const uint32_t j = nb[(size_t)i * k + s];
      const float d2 = nb_d2[(size_t)i * k + s];
      if (!entry_ok(i, j, d2, n)) continue;
      const uint8_t* sj = spfh + (size_t)j * SPFH_STRIDE;
      const uint32_t uj = sj[33];
      if (uj == 0) continue;  // (a neighbour without a normal, or non-finite, has no SPFH either)
      const double wgt = 1.0 / (double)d2, du = (double)uj;
#pragma unroll
      for (int b = 0; b < DIM; ++b) acc[b] += (((double)sj[b] * 100.0) / du) * wgt;
      any = true;
    }
  }
  float* o = out + (size_t)i * DIM;
#pragma unroll
  for (int h = 0; h < 3; ++h) {
    double sum = 0.0;
#pragma unroll
    for (int b = 0; b < NB; ++b) sum += acc[h * NB + b];
    const double sc = (any && sum > 0.0) ? 100.0 / sum : 0.0;
#pragma unroll
    for (int b = 0; b < NB; ++b) o[h * NB + b] = (float)(acc[h * NB + b] * sc);
  }
}

// F2 over wide lists: one wave per point.  The list is read once, a lane per entry (with the neighbour's `used`), and then
// walked in order with lane b < 33 adding bin b: each of the 33 fp64 sums is taken in list order, as F2 defines it, and the
// three sub-histogram totals in bin order.
__global__ __launch_bounds__(256) void fpfh_wide_kernel(const uint8_t* __restrict__ spfh, const uint32_t* __restrict__ nb,
                                                         const float* __restrict__ nb_d2, uint32_t n, int k, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;  // (the whole wave)
  const int bl = lane < DIM ? lane : 0;
  double acc = 0.0;
  bool any = false;
  if (spfh[(size_t)i * SPFH_STRIDE + 33] != 0) {
    for (int s0 = 0; s0 < k; s0 += 64) {
      const int s = s0 + lane;
      uint32_t j = NONE, uj = 0;
      float d2 = 0.f;
      if (s < k) {
        j = nb[(size_t)i * k + s];
        d2 = nb_d2[(size_t)i * k + s];
        if (entry_ok(i, j, d2, n)) uj = spfh[(size_t)j * SPFH_STRIDE + 33];  // (0: a neighbour without an SPFH)
      }
      unsigned long long todo = __ballot(uj != 0);
      while (todo) {  // ascending lanes = list order
        const int t = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const uint32_t jt = (uint32_t)__builtin_amdgcn_readlane((int)j, t), ut = (uint32_t)__builtin_amdgcn_readlane((int)uj, t);
        const float dt = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(d2), t));
        const double wgt = 1.0 / (double)dt, du = (double)ut;
        acc += (((double)spfh[(size_t)jt * SPFH_STRIDE + bl] * 100.0) / du) * wgt;
        any = true;
      }
    }
  }
  const int h = bl / NB;
  double sum = 0.0;
  for (int b = 0; b < NB; ++b) sum += __shfl(acc, h * NB + b);
  const double sc = (any && sum > 0.0) ? 100.0 / sum : 0.0;
  if (lane < DIM) out[(size_t)i * DIM + lane] = (float)(acc * sc);
}

// rows of `width` floats between original order and the order of the sorted points (pts[i].w = original index of i)
__global__ __launch_bounds__(256) void rows_reorder_kernel(const f32x4* __restrict__ pts, uint32_t n, const float* __restrict__ in,
                                                           float* __restrict__ out, uint32_t width, bool to_sorted) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)n * width) return;
  const uint32_t i = (uint32_t)(e / width), c = (uint32_t)(e % width);
  const uint32_t o = __float_as_uint(pts[i].w);
  if (o >= n) return;
  out[(size_t)(to_sorted ? i : o) * width + c] = in[(size_t)(to_sorted ? o : i) * width + c];
}

// One search of F3: every row of A against the rows of B.  a_pts / b_pts: the scans' sorted points when the rows are in
// the store's order (the original index is their .w), null when the rows are in original order already.  keys [a_n] by
// ORIGINAL index of the A row, preset to NO_KEY: (bits(d2) << 32) | original index of the B row.

// F3.  grid = (ceil(max a_n / 256), slices of B, tasks).  The distance is the defined one: acc = 0; acc = acc + (a - b) * (a - b)
// over the 33 values in order, every operation rounded (the file is compiled with contraction off; the packed forms round
// per element as the scalar ones do).
__global__ __launch_bounds__(MATCH_THREADS) void fpfh_match_kernel(const MatchTask* __restrict__ tasks, uint32_t slice_tiles) {
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  __shared__ f32x2 tile[(MATCH_TILE / 2) * DIM];  // [pair of rows][value]: (row 2r, row 2r + 1)
  __shared__ uint32_t tile_idx[MATCH_TILE];       // original index of the row, NONE: no feature / padding
  const MatchTask T = tasks[blockIdx.z];
  const uint32_t row = blockIdx.x * MATCH_THREADS + threadIdx.x;
  if (blockIdx.x * MATCH_THREADS >= T.a_n) return;  // (uniform over the work-group)
  const uint32_t t_begin = blockIdx.y * slice_tiles * MATCH_TILE;
  if (t_begin >= T.b_n) return;
  const uint32_t t_end = min(T.b_n, t_begin + slice_tiles * MATCH_TILE);
  float a[DIM];
  bool have = false;
#pragma unroll
  for (int c = 0; c < DIM; ++c) {
    a[c] = row < T.a_n ? T.a_feat[(size_t)row * DIM + c] : 0.f;
    have = have || a[c] != 0.f;
  }
  float best = __builtin_inff();
  uint32_t best_i = NONE;
  float* tf = reinterpret_cast<float*>(tile);
  for (uint32_t t0 = t_begin; t0 < t_end; t0 += MATCH_TILE) {
    const uint32_t rows = min((uint32_t)MATCH_TILE, t_end - t0);
    __syncthreads();  // the previous tile has been read
    for (uint32_t e = threadIdx.x; e < (uint32_t)(MATCH_TILE * DIM); e += MATCH_THREADS) {
      const uint32_t r = e / DIM, c = e % DIM;
      tf[((r >> 1) * DIM + c) * 2 + (r & 1)] = r < rows ? T.b_feat[(size_t)(t0 + r) * DIM + c] : 0.f;
    }
    __syncthreads();
    if (threadIdx.x < MATCH_TILE) {
      const uint32_t r = threadIdx.x;
      bool nz = false;
      for (int c = 0; c < DIM; ++c) nz = nz || tf[((r >> 1) * DIM + c) * 2 + (r & 1)] != 0.f;
      uint32_t o = NONE;
      if (r < rows && nz) o = T.b_pts ? __float_as_uint(T.b_pts[t0 + r].w) : t0 + r;
      tile_idx[r] = o;
    }
    __syncthreads();
    const uint32_t pairs = (rows + 1) / 2;
    for (uint32_t r = 0; r < pairs; ++r) {
      f32x2 acc = {0.f, 0.f};
#pragma unroll
      for (int c = 0; c < DIM; ++c) {
        const f32x2 t = f32x2{a[c], a[c]} - tile[r * DIM + c];
        acc = acc + t * t;
      }
      const uint32_t o0 = tile_idx[2 * r], o1 = tile_idx[2 * r + 1];
      if (o0 != NONE && (acc.x < best || (acc.x == best && o0 < best_i))) { best = acc.x; best_i = o0; }
      if (o1 != NONE && (acc.y < best || (acc.y == best && o1 < best_i))) { best = acc.y; best_i = o1; }
    }
  }
  if (row < T.a_n && have && best_i != NONE) {
    const uint32_t o = T.a_pts ? __float_as_uint(T.a_pts[row].w) : row;
    if (o < T.a_n)
      atomicMin(&T.keys[o], ((unsigned long long)__float_as_uint(best) << 32) | (unsigned long long)best_i);
  }
}

// A job of F4: the forward keys of the source's rows, the backward keys of the target's (null: not mutual), the scans'
// points in original order (packed xyz); for a job on keypoints the rows are keypoint ranks and src_map / tgt_map the
// keypoints' original indices.

// F4.  One work-group per job; pairs[(job * ld + m) * 2 + {0, 1}] = (source point, matched target point) of the m-th kept
// source in ascending original index; the count goes to counts[job].
__global__ __launch_bounds__(1024) void fpfh_pairs_kernel(const PairJob* __restrict__ pj, size_t ld, f32x4* __restrict__ pairs,
                                                          uint32_t* __restrict__ counts) {
  __shared__ uint32_t wave_cnt[16], base_s;
  const int job = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const PairJob J = pj[job];
  if (tid == 0) base_s = 0;
  __syncthreads();
  for (uint32_t i0 = 0; i0 < J.n_src; i0 += 1024) {
    const uint32_t i = i0 + (uint32_t)tid;
    bool keep = false;
    uint32_t j = NONE;
    if (i < J.n_src) {
      const unsigned long long key = J.fwd[i];
      j = (uint32_t)(key & 0xFFFFFFFFull);
      keep = key != NO_KEY && j < J.n_tgt;
      if (keep && J.bwd) {
        const unsigned long long back = J.bwd[j];
        keep = back != NO_KEY && (uint32_t)(back & 0xFFFFFFFFull) == i;
      }
    }
    const unsigned long long m = __ballot(keep);
    if (lane == 0) wave_cnt[w] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t off = base_s, tot = 0;
    for (int q = 0; q < 16; ++q) {
      if (q < w) off += wave_cnt[q];
      tot += wave_cnt[q];
    }
    if (keep) {
      const size_t slot = (size_t)job * ld + off + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
      const size_t pi = J.src_map ? J.src_map[i] : i, qj = J.tgt_map ? J.tgt_map[j] : j;  // (keypoint rank -> original index)
      pairs[slot * 2 + 0] = f32x4{J.src_xyz[3 * pi], J.src_xyz[3 * pi + 1], J.src_xyz[3 * pi + 2], 0.f};
      pairs[slot * 2 + 1] = f32x4{J.tgt_xyz[3 * qj], J.tgt_xyz[3 * qj + 1], J.tgt_xyz[3 * qj + 2], 0.f};
    }
    __syncthreads();
    if (tid == 0) base_s += tot;
    __syncthreads();
  }
  if (tid == 0) counts[job] = base_s;
}

}  // namespace fpfh
}  // namespace gloc
