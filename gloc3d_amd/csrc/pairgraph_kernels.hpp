// pairgraph_kernels.hpp -- device kernels of the correspondence-graph global registration (include/gloc3d.h, G1 - G3;
// tests/pairgraph_ref.py is the contract).  The pair list is the RANSAC stage's pairs layout (reg_kernels.hpp): slot i of
// job c at pairs[(c * ld + i) * 2 + {0, 1}], counts[c] = M pairs.
//
//   pg_matrix_kernel      G1: the compatibility matrix C as bit rows, one wave ballot per 64-bit word
//   pg_score_kernel       G2: score_i = sum over the set bits j of row i of popc(row_i & row_j); degree_i = popc(row_i)
//   pg_seeds_kernel       G3: the n_seeds largest (score, then smaller position), one work-group per job
//   pg_seed_sets_kernel   G3: S_sj of a seed's row, its maximum, the thresholded set compacted in ascending position
//   pg_moments_kernel     G3: fp64 raw moments of a set, reduced as the RANSAC refit reduces them (accum_kernel<1>); the
//                         solve from them is graph_solve_kernel in reg.hip, beside kabsch_from_cov (reg_kernels.hpp
//                         defines that stage's kernels and can be part of one translation unit only)
//
// A bit row has `words` 64-bit words (the batch's longest list, rounded up to a whole word); a job of M pairs reads and
// writes its first ceil(M / 64) words only, the bits past M in its last word zero.  Everything but the fits is integer
// arithmetic, so no order of summation can matter; the matrix entries are fp64 from the fp32 points (this unit is
// compiled with -ffp-contract=off like the others: every product and sum rounded on its own).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lane_ops.hpp"
#include "math3.hpp"  // f32x4

namespace gloc {
namespace pairgraph {

using reg::f32x4;

constexpr int PG_THREADS = 256;
constexpr int PG_WAVES = PG_THREADS / 64;
constexpr int PG_MAT_ROWS = 64;  // rows per work-group of the matrix kernel: 16 per wave against one set of 64 columns
constexpr uint32_t PG_NONE = 0xFFFFFFFFu;
constexpr int PG_NV = 16;        // moments of a fit: n, sum p [3], sum q [3], sum p q^T [9]

// A group of jobs as the kernels see it: job (job0 + g) of the batch owns matrix g of the group.
struct Group {
  const f32x4* pairs;
  size_t ld;
  const uint32_t* counts;  // [job]: M
  uint32_t job0;
  uint32_t rows, words;      // rows of a matrix (the batch's longest list) and words of a row
  unsigned long long* bits;  // [group job][rows][words]
};

__device__ __forceinline__ bool pg_finite(const f32x4& p, const f32x4& q) {
  return isfinite(p.x) && isfinite(p.y) && isfinite(p.z) && isfinite(q.x) && isfinite(q.y) && isfinite(q.z);
}

__device__ __forceinline__ uint32_t pg_wave_sum_u32(uint32_t x) {
  x += xor_lane_u32<32>(x);
  x += xor_lane_u32<16>(x);
  x += xor_lane_u32<8>(x);
  x += xor_lane_u32<4>(x);
  x += xor_lane_u32<2>(x);
  x += xor_lane_u32<1>(x);
  return x;
}

// G1.  grid = (words, ceil(rows / PG_MAT_ROWS), group jobs).  Lane l keeps pair 64 w + l -- the column -- in registers
// for the work-group's 64 rows, which are staged once in LDS and read back as wave-uniform broadcasts; each wave
// ballots 16 words.  Per entry: a = sqrt((dx dx + dy dy) + dz dz) over P_i - P_j, b over Q, C_ij = |a - b| < thr.
__global__ __launch_bounds__(PG_THREADS) void pg_matrix_kernel(Group g, double thr) {
  __shared__ double rp[PG_MAT_ROWS][6];
  __shared__ uint32_t rfin[PG_MAT_ROWS];
  const uint32_t w = blockIdx.x, r0 = blockIdx.y * PG_MAT_ROWS, job = g.job0 + blockIdx.z;
  const uint32_t M = g.counts[job];
  if (r0 >= M || w * 64u >= M) return;  // (uniform: rows and words this job does not have)
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const f32x4* pp = g.pairs + (size_t)job * g.ld * 2;
  if (tid < PG_MAT_ROWS) {
    const uint32_t i = r0 + (uint32_t)tid;
    f32x4 p = {0.f, 0.f, 0.f, 0.f}, q = {0.f, 0.f, 0.f, 0.f};
    if (i < M) {
      p = pp[2 * (size_t)i];
      q = pp[2 * (size_t)i + 1];
    }
    rp[tid][0] = (double)p.x; rp[tid][1] = (double)p.y; rp[tid][2] = (double)p.z;
    rp[tid][3] = (double)q.x; rp[tid][4] = (double)q.y; rp[tid][5] = (double)q.z;
    rfin[tid] = (i < M && pg_finite(p, q)) ? 1u : 0u;
  }
  const uint32_t j = w * 64u + (uint32_t)lane;
  double cp[3] = {0.0, 0.0, 0.0}, cq[3] = {0.0, 0.0, 0.0};
  bool cfin = false;
  if (j < M) {
    const f32x4 p = pp[2 * (size_t)j], q = pp[2 * (size_t)j + 1];
    cp[0] = (double)p.x; cp[1] = (double)p.y; cp[2] = (double)p.z;
    cq[0] = (double)q.x; cq[1] = (double)q.y; cq[2] = (double)q.z;
    cfin = pg_finite(p, q);
  }
  __syncthreads();
  unsigned long long* out = g.bits + ((size_t)blockIdx.z * g.rows + r0) * g.words + w;
  for (int r = wv * (PG_MAT_ROWS / PG_WAVES); r < (wv + 1) * (PG_MAT_ROWS / PG_WAVES); ++r) {
    const uint32_t i = r0 + (uint32_t)r;
    if (i >= M) break;  // (uniform over the wave)
    double dx = rp[r][0] - cp[0], dy = rp[r][1] - cp[1], dz = rp[r][2] - cp[2];
    const double a = sqrt((dx * dx + dy * dy) + dz * dz);
    dx = rp[r][3] - cq[0]; dy = rp[r][4] - cq[1]; dz = rp[r][5] - cq[2];
    const double b = sqrt((dx * dx + dy * dy) + dz * dz);
    const bool c = cfin && rfin[r] != 0u && i != j && fabs(a - b) < thr;
    const unsigned long long word = __ballot(c);
    if (lane == 0) out[(size_t)r * g.words] = word;
  }
}

// G2, the hot path.  grid = (ceil(rows / PG_WAVES), group jobs); a work-group holds PG_WAVES rows i in LDS, a wave owns
// one.  The wave walks the set bits of its row word by word; the lanes are cut into 64 / lanes_per_row teams (a row of 32
// words: two teams), team t takes the set bits t, t + teams, ... of the word and streams row j -- lane k of the team its
// word k -- against row i.  lanes_per_row: the power of two >= min(words, 64), from the host.  Rows longer than 64 words
// are streamed 64 words at a time by one team.  No scratch, no floating point.
__global__ __launch_bounds__(PG_THREADS) void pg_score_kernel(Group g, uint32_t lanes_per_row, unsigned long long* __restrict__ score /* [job][rows] */,
                                                             uint32_t* __restrict__ degree /* [job][rows] */) {
  extern __shared__ unsigned long long pg_rows[];  // [PG_WAVES][words]
  const uint32_t job = g.job0 + blockIdx.y, M = g.counts[job];
  if (blockIdx.x * PG_WAVES >= M) return;  // (uniform)
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const uint32_t i = blockIdx.x * PG_WAVES + (uint32_t)wv, Wc = (M + 63u) >> 6;
  const unsigned long long* mat = g.bits + (size_t)blockIdx.y * g.rows * g.words;
  unsigned long long* mine = pg_rows + (size_t)wv * g.words;
  if (i < M)
    for (uint32_t k = (uint32_t)lane; k < Wc; k += 64u) mine[k] = mat[(size_t)i * g.words + k];
  __syncthreads();
  if (i >= M) return;
  const uint32_t team = (uint32_t)lane / lanes_per_row, kw = (uint32_t)lane % lanes_per_row, teams = 64u / lanes_per_row;
  const bool one = Wc <= lanes_per_row;  // the whole row in one register per lane
  const unsigned long long my = (one && kw < Wc) ? mine[kw] : 0ull;
  uint32_t acc = 0, deg = 0;
  for (uint32_t k = (uint32_t)lane; k < Wc; k += 64u) deg += (uint32_t)__popcll(mine[k]);
  for (uint32_t w = 0; w < Wc; ++w) {
    unsigned long long rem = mine[w];  // (wave-uniform)
    if (rem == 0ull) continue;
    for (uint32_t t = 0; t < team && rem; ++t) rem &= rem - 1ull;  // the team's first set bit
    while (rem) {
      const uint32_t j = w * 64u + (uint32_t)(__ffsll((long long)rem) - 1);
      const unsigned long long* rj = mat + (size_t)j * g.words;
      if (one) {
        if (kw < Wc) acc += (uint32_t)__popcll(my & rj[kw]);
      } else {
        for (uint32_t k = kw; k < Wc; k += lanes_per_row) acc += (uint32_t)__popcll(mine[k] & rj[k]);
      }
      for (uint32_t t = 0; t < teams && rem; ++t) rem &= rem - 1ull;  // the team's next
    }
  }
  // (a lane's sum stays below 2^32: at most M bits per row, M rows)
  unsigned long long tot = (unsigned long long)acc;
  tot += xor_lane_u64<32>(tot);
  tot += xor_lane_u64<16>(tot);
  tot += xor_lane_u64<8>(tot);
  tot += xor_lane_u64<4>(tot);
  tot += xor_lane_u64<2>(tot);
  tot += xor_lane_u64<1>(tot);
  deg = pg_wave_sum_u32(deg);
  if (lane == 0) {
    score[(size_t)job * g.rows + i] = tot;
    degree[(size_t)job * g.rows + i] = deg;
  }
}

// (score, position) a before b in the seed order: the larger score, then the smaller position; PG_NONE: no entry
__device__ __forceinline__ bool pg_before(unsigned long long sa, uint32_t pa, unsigned long long sb, uint32_t pb) {
  return pa != PG_NONE && (pb == PG_NONE || sa > sb || (sa == sb && pa < pb));
}

// G3.  One work-group per job: n_seeds rounds of "the first entry in the seed order behind the one taken last", every
// round a pass over the job's scores (L2-resident: 8 bytes per pair) and a reduction.  Ranks past M get PG_NONE.
__global__ __launch_bounds__(PG_THREADS) void pg_seeds_kernel(const uint32_t* __restrict__ counts, uint32_t job0, uint32_t rows,
                                                             const unsigned long long* __restrict__ score, uint32_t n_seeds,
                                                             uint32_t* __restrict__ seeds /* [job][n_seeds] */) {
  __shared__ unsigned long long ws[PG_WAVES];
  __shared__ uint32_t wp[PG_WAVES];
  const uint32_t job = job0 + blockIdx.x, M = counts[job];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const unsigned long long* sc = score + (size_t)job * rows;
  unsigned long long ps = 0ull;
  uint32_t pp = PG_NONE;  // the entry taken last (none yet)
  for (uint32_t r = 0; r < n_seeds; ++r) {
    unsigned long long bs = 0ull;
    uint32_t bp = PG_NONE;
    for (uint32_t i = (uint32_t)tid; i < M; i += PG_THREADS) {
      const unsigned long long s = sc[i];
      const bool behind = pp == PG_NONE || s < ps || (s == ps && i > pp);
      if (behind && pg_before(s, i, bs, bp)) {
        bs = s;
        bp = i;
      }
    }
#define GLOC_PG_STEP(O)                                     \
  {                                                         \
    const unsigned long long os = xor_lane_u64<O>(bs);      \
    const uint32_t op = xor_lane_u32<O>(bp);                \
    if (pg_before(os, op, bs, bp)) {                        \
      bs = os;                                              \
      bp = op;                                              \
    }                                                       \
  }
    GLOC_PG_STEP(32) GLOC_PG_STEP(16) GLOC_PG_STEP(8) GLOC_PG_STEP(4) GLOC_PG_STEP(2) GLOC_PG_STEP(1)
#undef GLOC_PG_STEP
    if (lane == 0) {
      ws[wv] = bs;
      wp[wv] = bp;
    }
    __syncthreads();
    bs = ws[0];
    bp = wp[0];
    for (int q = 1; q < PG_WAVES; ++q)
      if (pg_before(ws[q], wp[q], bs, bp)) {
        bs = ws[q];
        bp = wp[q];
      }
    __syncthreads();  // (ws / wp are written again next round)
    if (tid == 0) seeds[(size_t)job * n_seeds + r] = bp;
    if (bp == PG_NONE) {  // (uniform) the list is used up
      for (uint32_t q = r + 1 + (uint32_t)tid; q < n_seeds; q += PG_THREADS) seeds[(size_t)job * n_seeds + q] = PG_NONE;
      return;
    }
    ps = bs;
    pp = bp;
  }
}

// G3.  grid = (n_seeds, group jobs).  The seed's row in LDS; thread <-> pair j: S_sj = popc(row_s & row_j) where bit j of
// row s is set, kept in srow; the row maximum; then the set {s} u {j: theta_den S_sj >= theta_num max, S_sj > 0}
// compacted in ascending position by ballot prefix sums (as fpfh_pairs_kernel compacts the matches).  set_sizes: 0 for a
// rank past M or a seed whose row maximum is 0.
__global__ __launch_bounds__(PG_THREADS) void pg_seed_sets_kernel(Group g, const uint32_t* __restrict__ seeds, uint32_t n_seeds, uint32_t theta_num,
                                                                 uint32_t theta_den, uint32_t* __restrict__ srow /* [group job][n_seeds][rows] */,
                                                                 uint32_t* __restrict__ sets /* [group job][n_seeds][rows] */,
                                                                 uint32_t* __restrict__ set_sizes /* [job][n_seeds] */) {
  extern __shared__ unsigned long long pg_rows[];  // [words]
  __shared__ uint32_t wave_val[PG_WAVES], base_s;
  const uint32_t r = blockIdx.x, job = g.job0 + blockIdx.y, M = g.counts[job];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const size_t o = (size_t)job * n_seeds + r;
  const uint32_t s = seeds[o];
  if (s >= M) {  // (uniform; PG_NONE)
    if (tid == 0) set_sizes[o] = 0;
    return;
  }
  const uint32_t Wc = (M + 63u) >> 6;
  const unsigned long long* mat = g.bits + (size_t)blockIdx.y * g.rows * g.words;
  for (uint32_t k = (uint32_t)tid; k < Wc; k += PG_THREADS) pg_rows[k] = mat[(size_t)s * g.words + k];
  if (tid == 0) base_s = 0;
  __syncthreads();
  uint32_t* sr = srow + ((size_t)blockIdx.y * n_seeds + r) * g.rows;
  uint32_t* list = sets + ((size_t)blockIdx.y * n_seeds + r) * g.rows;
  uint32_t mx = 0;
  for (uint32_t j = (uint32_t)tid; j < M; j += PG_THREADS) {
    uint32_t v = 0;
    if ((pg_rows[j >> 6] >> (j & 63u)) & 1ull) {
      const unsigned long long* rj = mat + (size_t)j * g.words;
      for (uint32_t k = 0; k < Wc; ++k) v += (uint32_t)__popcll(pg_rows[k] & rj[k]);
    }
    sr[j] = v;  // (read back below by the thread that wrote it)
    mx = v > mx ? v : mx;
  }
  for (int off = 32; off > 0; off >>= 1) {
    const uint32_t t = (uint32_t)__shfl_xor((int)mx, off);
    mx = t > mx ? t : mx;
  }
  if (lane == 0) wave_val[wv] = mx;
  __syncthreads();
  mx = wave_val[0];
  for (int q = 1; q < PG_WAVES; ++q) mx = wave_val[q] > mx ? wave_val[q] : mx;
  __syncthreads();  // (wave_val is the compaction's counter next)
  if (mx == 0) {    // (uniform) no hypothesis
    if (tid == 0) set_sizes[o] = 0;
    return;
  }
  const unsigned long long need = (unsigned long long)theta_num * mx;
  for (uint32_t j0 = 0; j0 < M; j0 += PG_THREADS) {
    const uint32_t j = j0 + (uint32_t)tid;
    bool keep = false;
    if (j < M) {
      const uint32_t v = sr[j];
      keep = j == s || (v > 0 && (unsigned long long)theta_den * v >= need);
    }
    const unsigned long long m = __ballot(keep);
    if (lane == 0) wave_val[wv] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t off = base_s, tot = 0;
    for (int q = 0; q < PG_WAVES; ++q) {
      if (q < wv) off += wave_val[q];
      tot += wave_val[q];
    }
    if (keep) list[off + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = j;
    __syncthreads();
    if (tid == 0) base_s += tot;
    __syncthreads();
  }
  if (tid == 0) set_sizes[o] = base_s;
}

// G3.  grid = (n_seeds, group jobs).  The fp64 raw moments of a set of at least three members, over the set's list:
// thread t takes entries t, t + 256, ...; xor butterfly inside the wave, the four waves in order (accum_kernel's
// reduction).  moments [job][n_seeds][PG_NV]; valid = 0 where there is no hypothesis.
__global__ __launch_bounds__(PG_THREADS) void pg_moments_kernel(Group g, const uint32_t* __restrict__ sets, const uint32_t* __restrict__ set_sizes,
                                                               uint32_t n_seeds, double* __restrict__ moments, uint32_t* __restrict__ valid) {
  __shared__ double red[PG_WAVES][PG_NV];
  const uint32_t r = blockIdx.x, job = g.job0 + blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const size_t o = (size_t)job * n_seeds + r;
  const uint32_t n = set_sizes[o];
  if (n < 3u) {  // (uniform)
    if (tid == 0) valid[o] = 0;
    return;
  }
  const uint32_t* list = sets + ((size_t)blockIdx.y * n_seeds + r) * g.rows;
  const f32x4* pp = g.pairs + (size_t)job * g.ld * 2;
  double v[PG_NV];
#pragma unroll
  for (int k = 0; k < PG_NV; ++k) v[k] = 0.0;
  for (uint32_t e = (uint32_t)tid; e < n; e += PG_THREADS) {
    const uint32_t j = list[e];
    const f32x4 p = pp[2 * (size_t)j], q = pp[2 * (size_t)j + 1];
    const double P[3] = {(double)p.x, (double)p.y, (double)p.z};
    const double Q[3] = {(double)q.x, (double)q.y, (double)q.z};
    v[0] += 1.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      v[1 + a] += P[a];
      v[4 + a] += Q[a];
#pragma unroll
      for (int b = 0; b < 3; ++b) v[7 + 3 * a + b] += P[a] * Q[b];
    }
  }
#pragma unroll
  for (int k = 0; k < PG_NV; ++k) {
    double x = v[k];
    x += xor_lane<32>(x);
    x += xor_lane<16>(x);
    x += xor_lane<8>(x);
    x += xor_lane<4>(x);
    x += xor_lane<2>(x);
    x += xor_lane<1>(x);
    if (lane == 0) red[wv][k] = x;
  }
  __syncthreads();
  if (tid < PG_NV) {
    double s = 0.0;
    for (int q = 0; q < PG_WAVES; ++q) s += red[q][tid];
    moments[o * PG_NV + (size_t)tid] = s;
  }
  if (tid == 0) valid[o] = 1;
}

}  // namespace pairgraph
}  // namespace gloc
