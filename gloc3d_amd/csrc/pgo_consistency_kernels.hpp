// pgo_consistency_kernels.hpp -- device side of the pose graph's closure selection (include/gloc3d.h, gloc_pgo_consistency,
// C1 - C6; gfx950), fp64 and integers.  tests/pcm_ref.py is the contract; pgo.hip is the host side.
//
//   pc_setup_kernel    C1, a lane per closure: its end poses gathered, Z widened, B = (T_j Z) T_i^-1, Sigma = Omega^-1 by chol6 /
//                      chol_solve of the unit vectors, the status; PC_OPS doubles per closure, structure of arrays [k][L]
//   pc_pair_kernel     C2 and C3, the hot path: the consistency matrix as bit rows, one wave ballot per 64-bit word
//   (degree, score and the seed ranking are pairgraph_kernels.hpp's pg_score_kernel and pg_seeds_kernel, unchanged, through
//   pairgraph::score_matrix and rank_seeds; pc_key_kernel makes the key they rank)
//   pc_clique_kernel   C5, one work-group per seed: cand as bit words in LDS, a team of lanes per candidate for the popcounts
//                      of the seed's row, which are then held per candidate and updated by what each step removes
//   pc_choose_kernel   C6, one work-group: the winner and its mask
//
// The pair kernel's layout is pg_matrix_kernel's: a work-group takes one word column w -- lane l keeps closure 64 w + l, the
// pair's b, in registers -- and the 64 rows of row block rb, staged once in LDS and read back as wave-uniform broadcasts;
// each wave ballots 16 words.  The statistic is defined for a < b only, so only the blocks rb <= w do work (the others
// leave at once) and every unordered pair is evaluated ONCE: the block's 64 ballot words are kept in LDS, thread t gathers
// bit t of each into the transposed word, and the block writes word w of its rows and word rb of its columns' rows (the
// diagonal block ORs the two).  Mirroring costs 64 LDS reads a thread against some 1500 fp64 operations a pair.
//
// No work-group waits for another, there are no atomics, and no floating-point value crosses a lane: a pair's statistic is
// computed by one lane from its operands alone, so determinism is structural.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lane_ops.hpp"
#include "pgo_kernels.hpp"

namespace gloc {
namespace pgo {

// a closure's operands: rigid motions as R [9] row-major then t [3]
enum { PC_TI = 0, PC_TJ = 12, PC_Z = 24, PC_B = 36, PC_SIG = 48, PC_PI = 69, PC_PJ = 70, PC_OPS = 71 };
constexpr int PC_ROWS = 64;                // rows of a work-group of the pair kernel: one 64 x 64 block of the matrix
constexpr int PC_ROW_OPS = PC_OPS - 12;    // a row's operands in LDS: all but B
constexpr uint32_t PC_NONE = 0xFFFFFFFFu;
constexpr size_t PC_MAX_L = 16384, PC_MAX_S2_L = 4096;

// C = A B for rigid motions
__device__ __forceinline__ void pc_rigid_mul(const double* A, const double* B, double* C) {
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int b = 0; b < 3; ++b) C[3 * a + b] = (A[3 * a] * B[b] + A[3 * a + 1] * B[3 + b]) + A[3 * a + 2] * B[6 + b];
    C[9 + a] = ((A[3 * a] * B[9] + A[3 * a + 1] * B[10]) + A[3 * a + 2] * B[11]) + A[9 + a];
  }
}

// ---- C1 -------------------------------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(THREADS) void pc_setup_kernel(uint32_t L, const uint32_t* __restrict__ src, const uint32_t* __restrict__ tgt,
                                                                  const float* __restrict__ Zf /* [12][L] */, const double* __restrict__ Om /* [21][L] */,
                                                                  const double* __restrict__ P /* [n][12] */, const double* __restrict__ pth /* [2][L] */,
                                                                  double* __restrict__ ops /* [PC_OPS][L] */, uint8_t* __restrict__ status) {
  const uint32_t a = blockIdx.x * THREADS + threadIdx.x;
  if (a >= L) return;
  const double* Pi = P + 12 * (size_t)src[a];
  const double* Pj = P + 12 * (size_t)tgt[a];
  double Ti[12], Tj[12], Z[12], TZ[12], Tinv[12], B[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) Ti[k] = Pi[k], Tj[k] = Pj[k], Z[k] = (double)Zf[(size_t)k * L + a];
  pc_rigid_mul(Tj, Z, TZ);
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) Tinv[3 * r + c] = Ti[3 * c + r];
    Tinv[9 + r] = -((Ti[r] * Ti[9] + Ti[3 + r] * Ti[10]) + Ti[6 + r] * Ti[11]);
  }
  pc_rigid_mul(TZ, Tinv, B);
  double O[21], Lf[21], S[21];
#pragma unroll
  for (int k = 0; k < 21; ++k) O[k] = Om[(size_t)k * L + a];
  const bool ok = chol6(O, Lf);
#pragma unroll
  for (int b = 0; b < 6; ++b) {
    double e[6], z[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) e[k] = k == b ? 1.0 : 0.0;
    chol_solve(Lf, e, 1.0, z);
#pragma unroll
    for (int r = 0; r <= b; ++r) S[ut(r, b)] = ok ? z[r] : 0.0;
  }
  double* o = ops + a;
#pragma unroll
  for (int k = 0; k < 12; ++k) {
    o[(size_t)(PC_TI + k) * L] = Ti[k];
    o[(size_t)(PC_TJ + k) * L] = Tj[k];
    o[(size_t)(PC_Z + k) * L] = Z[k];
    o[(size_t)(PC_B + k) * L] = B[k];
  }
#pragma unroll
  for (int k = 0; k < 21; ++k) o[(size_t)(PC_SIG + k) * L] = S[k];
  o[(size_t)PC_PI * L] = pth[a];
  o[(size_t)PC_PJ * L] = pth[(size_t)L + a];
  status[a] = ok ? 0 : 1;
}

// ---- C2 -------------------------------------------------------------------------------------------------------------------
// The statistic of the pair (a, b), a < b.  rw: a's operands (LDS: T_i, T_j, Z, Sigma, path_i, path_j); b's in registers.
// False where M fails the pivot rule or the value is not finite.
__device__ __forceinline__ bool pc_pair_s2(const double* rw, const double* Bb, const double* Tjb, const double* Sb, double pib, double pjb, double dr2,
                                           double dt2, double* out) {
  const double* Rj = rw + 12;  // T_ja
  const double* Rz = rw + 24;  // Z_a
  double Tn[12];               // T_i := B_b T_ia
  pc_rigid_mul(Bb, rw, Tn);
  double r[6];
  {  // G2, as linearize_kernel words it
    double M[9], RE[9], u[3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) M[3 * a + b] = (Rj[a] * Tn[b] + Rj[3 + a] * Tn[3 + b]) + Rj[6 + a] * Tn[6 + b];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) RE[3 * a + b] = (M[3 * a] * Rz[3 * b] + M[3 * a + 1] * Rz[3 * b + 1]) + M[3 * a + 2] * Rz[3 * b + 2];
#pragma unroll
    for (int a = 0; a < 3; ++a) u[a] = (RE[3 * a] * Rz[9] + RE[3 * a + 1] * Rz[10]) + RE[3 * a + 2] * Rz[11];
    const double d0 = Tn[9] - Rj[9], d1 = Tn[10] - Rj[10], d2 = Tn[11] - Rj[11];
#pragma unroll
    for (int a = 0; a < 3; ++a) r[3 + a] = ((Rj[a] * d0 + Rj[3 + a] * d1) + Rj[6 + a] * d2) - u[a];
    const double v0 = 0.5 * (RE[7] - RE[5]), v1 = 0.5 * (RE[2] - RE[6]), v2 = 0.5 * (RE[3] - RE[1]);
    const double s = sqrt((v0 * v0 + v1 * v1) + v2 * v2), c = (((RE[0] + RE[4]) + RE[8]) - 1.0) * 0.5;
    const double f = s < 1e-8 ? 1.0 + s * s / 6.0 : atan2(s, c) / s;
    r[0] = v0 * f, r[1] = v1 * f, r[2] = v2 * f;
  }
  // X = T_ja^-1 T_jb; Ad_X = [RX, 0; KR, RX], KR = [t_X]x R_X
  double RX[9], KR[9];
  {
    double tX[3];
    const double d0 = Tjb[9] - Rj[9], d1 = Tjb[10] - Rj[10], d2 = Tjb[11] - Rj[11];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
      for (int b = 0; b < 3; ++b) RX[3 * a + b] = (Rj[a] * Tjb[b] + Rj[3 + a] * Tjb[3 + b]) + Rj[6 + a] * Tjb[6 + b];
      tX[a] = (Rj[a] * d0 + Rj[3 + a] * d1) + Rj[6 + a] * d2;
    }
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      KR[b] = -tX[2] * RX[3 + b] + tX[1] * RX[6 + b];
      KR[3 + b] = tX[2] * RX[b] + -tX[0] * RX[6 + b];
      KR[6 + b] = -tX[1] * RX[b] + tX[0] * RX[3 + b];
    }
  }
  // entry (a, k) of Ad_X where it is not a structural zero (a < 3 and k >= 3)
  auto Ad = [&](int a, int k) -> double { return a < 3 ? RX[3 * a + k] : (k < 3 ? KR[3 * (a - 3) + k] : RX[3 * (a - 3) + (k - 3)]); };
  const double d = fabs(rw[57] - pib) + fabs(rw[58] - pjb);
  double Mu[21];
#pragma unroll
  for (int b = 0; b < 6; ++b) {  // column b of Sigma_b Ad^T, then column b of Ad (Sigma_b Ad^T) down to the diagonal
    double q[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      double s = 0.0;
#pragma unroll
      for (int c = 0; c < (b < 3 ? 3 : 6); ++c) s += sym(Sb, k, c) * Ad(b, c);
      q[k] = s;
    }
#pragma unroll
    for (int a = 0; a <= b; ++a) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < (a < 3 ? 3 : 6); ++k) s += Ad(a, k) * q[k];
      Mu[ut(a, b)] = rw[36 + ut(a, b)] + s;
    }
  }
  const double er = dr2 * d, et = dt2 * d;
#pragma unroll
  for (int a = 0; a < 3; ++a) Mu[ut(a, a)] += er, Mu[ut(3 + a, 3 + a)] += et;
  double Lf[21], y[6];
  const bool ok = chol6(Mu, Lf);
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double s = r[i];
#pragma unroll
    for (int k = 0; k < i; ++k) s -= Lf[i * (i + 1) / 2 + k] * y[k];
    y[i] = s / Lf[i * (i + 1) / 2 + i];
  }
  const double s2 = ((((y[0] * y[0] + y[1] * y[1]) + y[2] * y[2]) + y[3] * y[3]) + y[4] * y[4]) + y[5] * y[5];
  *out = s2;
  return ok && isfinite(s2);
}

// C2, C3.  grid = (words, words): word column w, row block rb; the blocks rb > w leave at once.  s2_out: null, or [L][L].
static __global__ __launch_bounds__(THREADS) void pc_pair_kernel(uint32_t L, uint32_t words, const double* __restrict__ ops,
                                                                 const uint8_t* __restrict__ status, double chi2, double dr2, double dt2,
                                                                 unsigned long long* __restrict__ bits /* [L][words] */, double* __restrict__ s2_out) {
  __shared__ double rp[PC_ROWS][PC_ROW_OPS];
  __shared__ uint32_t rbad[PC_ROWS];
  __shared__ unsigned long long sw[PC_ROWS];
  const uint32_t w = blockIdx.x, rb = blockIdx.y;
  if (rb > w) return;  // (uniform) the mirror of block (w, rb)
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const uint32_t r0 = rb * PC_ROWS;
  for (int idx = tid; idx < PC_ROWS * PC_ROW_OPS; idx += THREADS) {
    const int k = idx / PC_ROWS, r = idx % PC_ROWS;
    const uint32_t i = r0 + (uint32_t)r;
    rp[r][k] = i < L ? ops[(size_t)(k < PC_B ? k : k + 12) * L + i] : 0.0;
  }
  if (tid < PC_ROWS) {
    const uint32_t i = r0 + (uint32_t)tid;
    rbad[tid] = i < L ? (uint32_t)status[i] : 1u;
  }
  const uint32_t j = w * 64u + (uint32_t)lane;
  double Bb[12], Tjb[12], Sb[21], pib = 0.0, pjb = 0.0;
  bool cok = false;
#pragma unroll
  for (int k = 0; k < 12; ++k) Bb[k] = 0.0, Tjb[k] = 0.0;
#pragma unroll
  for (int k = 0; k < 21; ++k) Sb[k] = 0.0;
  if (j < L) {
#pragma unroll
    for (int k = 0; k < 12; ++k) Bb[k] = ops[(size_t)(PC_B + k) * L + j], Tjb[k] = ops[(size_t)(PC_TJ + k) * L + j];
#pragma unroll
    for (int k = 0; k < 21; ++k) Sb[k] = ops[(size_t)(PC_SIG + k) * L + j];
    pib = ops[(size_t)PC_PI * L + j], pjb = ops[(size_t)PC_PJ * L + j];
    cok = status[j] == 0;
  }
  __syncthreads();
  for (int r = wv * (PC_ROWS / WAVES); r < (wv + 1) * (PC_ROWS / WAVES); ++r) {
    const uint32_t i = r0 + (uint32_t)r;
    if (i >= L) {  // (uniform over the wave) a row the matrix does not have
      if (lane == 0) sw[r] = 0ull;
      continue;
    }
    bool c = false;
    double s2 = __builtin_inf();
    if (j < L && i < j && cok && rbad[r] == 0u) {
      double v;
      if (pc_pair_s2(rp[r], Bb, Tjb, Sb, pib, pjb, dr2, dt2, &v)) {
        s2 = v;
        c = v < chi2;
      }
    }
    const unsigned long long word = __ballot(c);
    if (lane == 0) sw[r] = word;
    if (s2_out != nullptr && j < L && i <= j) {
      s2_out[(size_t)i * L + j] = s2;
      if (i < j) s2_out[(size_t)j * L + i] = s2;
    }
  }
  __syncthreads();
  if (tid < PC_ROWS) {
    unsigned long long tw = 0ull;  // bit r: row r0 + r against column 64 w + tid, seen from the column
    for (int r = 0; r < PC_ROWS; ++r) tw |= ((sw[r] >> tid) & 1ull) << r;
    const uint32_t i = r0 + (uint32_t)tid, jt = w * 64u + (uint32_t)tid;
    if (rb == w) {
      if (i < L) bits[(size_t)i * words + w] = sw[tid] | tw;
    } else {
      bits[(size_t)i * words + w] = sw[tid];  // (rb < w: the row block is whole)
      if (jt < L) bits[(size_t)jt * words + rb] = tw;
    }
  }
}

// C4's key
static __global__ __launch_bounds__(THREADS) void pc_key_kernel(uint32_t L, const unsigned long long* __restrict__ score, const uint32_t* __restrict__ degree,
                                                                unsigned long long* __restrict__ key) {
  const uint32_t a = blockIdx.x * THREADS + threadIdx.x;
  if (a < L) key[a] = score[a] + (unsigned long long)degree[a];
}

// ---- C5, C6 -----------------------------------------------------------------------------------------------------------------
// (count, position) a before b: the larger count, then the smaller position; PC_NONE: no entry
__device__ __forceinline__ bool pc_before(uint32_t ca, uint32_t pa, uint32_t cb, uint32_t pb) {
  return pa != PC_NONE && (pb == PC_NONE || ca > cb || (ca == cb && pa < pb));
}

// the work-group's first entry in that order, the same in every thread; wc, wp: LDS [WAVES]
__device__ __forceinline__ void pc_first(uint32_t& bc, uint32_t& bp, uint32_t* wc, uint32_t* wp) {
#define GLOC_PC_STEP(O)                              \
  {                                                  \
    const uint32_t oc = xor_lane_u32<O>(bc);         \
    const uint32_t op = xor_lane_u32<O>(bp);         \
    if (pc_before(oc, op, bc, bp)) bc = oc, bp = op; \
  }
  GLOC_PC_STEP(32) GLOC_PC_STEP(16) GLOC_PC_STEP(8) GLOC_PC_STEP(4) GLOC_PC_STEP(2) GLOC_PC_STEP(1)
#undef GLOC_PC_STEP
  if ((threadIdx.x & 63) == 0) wc[threadIdx.x >> 6] = bc, wp[threadIdx.x >> 6] = bp;
  __syncthreads();
  bc = wc[0], bp = wp[0];
  for (int q = 1; q < WAVES; ++q)
    if (pc_before(wc[q], wp[q], bc, bp)) bc = wc[q], bp = wp[q];
  __syncthreads();  // (wc / wp are written again by the next call)
}

// C5.  grid = n_seeds.  LDS: cand [words], the members [words], the candidates a step removes [words]; a row has at most
// THREADS words, so a thread owns a word.  popcount(row_v & cand) is HELD per candidate (counts, global: read by other
// threads than wrote it, across barriers) instead of recounted at every step.  First the seed's row: the threads are cut
// into 256 / lanes_per_row teams (lanes_per_row: the power of two >= min(words, 64), from the host, as for
// pg_score_kernel), team t takes the set bits t, t + teams, ... of each word of cand -- every team makes the same number
// of rounds, one without a candidate left idles through them, so the exchanges run with all lanes --, lane k of the team
// counts words k, k + lanes_per_row, ... of row_v & cand, and the team's lanes are added by xor exchanges below
// lanes_per_row.  Then per step: a thread per word finds the first of the largest count among its candidates (ascending
// position: C5's tie rule), the ordered (count, -position) reduction picks v, a thread per word ANDs row_v into cand and
// keeps what left, gone = cand & ~row_v; the non-empty words of gone are listed by a ballot, and every candidate that
// stays loses popcount(row_u & gone) over those words -- one word in a true clique, where v alone leaves.  Recounting
// cost (clique size)^2 x words / 256 dependent loads a thread: 11 s for a clique of 7891 of 16384 closures.
static_assert(PC_MAX_L / 64 <= (size_t)THREADS, "a thread per word of a row");
static __global__ __launch_bounds__(THREADS) void pc_clique_kernel(uint32_t L, uint32_t words, uint32_t lanes_per_row,
                                                                   const unsigned long long* __restrict__ bits, const uint32_t* __restrict__ seeds,
                                                                   uint32_t* __restrict__ sizes /* [n_seeds] */,
                                                                   unsigned long long* __restrict__ members /* [n_seeds][words] */,
                                                                   uint32_t* counts /* [n_seeds][L] */) {
  extern __shared__ unsigned long long pc_lds[];
  __shared__ uint32_t wc[WAVES], wp[WAVES], nzw[THREADS];
  unsigned long long* cand = pc_lds;
  unsigned long long* mem = pc_lds + words;
  unsigned long long* gone = pc_lds + 2 * words;
  const uint32_t rank = blockIdx.x, s = seeds[rank];
  const uint32_t tid = threadIdx.x;
  unsigned long long* mine = members + (size_t)rank * words;
  if (s >= L) {  // (uniform; PC_NONE) a rank past the closures
    for (uint32_t k = tid; k < words; k += THREADS) mine[k] = 0ull;
    if (tid == 0) sizes[rank] = 0u;
    return;
  }
  for (uint32_t k = tid; k < words; k += THREADS) {
    cand[k] = bits[(size_t)s * words + k];
    mem[k] = k == (s >> 6) ? 1ull << (s & 63u) : 0ull;
  }
  __syncthreads();
  const uint32_t team = tid / lanes_per_row, kw = tid % lanes_per_row, teams = THREADS / lanes_per_row;
  const uint32_t lane = tid & 63u, wv = tid >> 6;
  uint32_t* cnt = counts + (size_t)rank * L;
  // the counts of the seed's row: a team per candidate
  for (uint32_t w = 0; w < words; ++w) {
    const unsigned long long all = cand[w];  // (uniform over the work-group)
    if (all == 0ull) continue;
    const uint32_t rounds = ((uint32_t)__popcll(all) + teams - 1) / teams;
    unsigned long long rem = all;
    for (uint32_t t = 0; t < team && rem; ++t) rem &= rem - 1ull;  // the team's first set bit
    for (uint32_t q = 0; q < rounds; ++q) {
      uint32_t v = PC_NONE, c = 0;
      if (rem) {
        v = w * 64u + (uint32_t)(__ffsll((long long)rem) - 1);
        const unsigned long long* rv = bits + (size_t)v * words;
        for (uint32_t k = kw; k < words; k += lanes_per_row) c += (uint32_t)__popcll(rv[k] & cand[k]);
      }
      if (lanes_per_row > 1) c += xor_lane_u32<1>(c);
      if (lanes_per_row > 2) c += xor_lane_u32<2>(c);
      if (lanes_per_row > 4) c += xor_lane_u32<4>(c);
      if (lanes_per_row > 8) c += xor_lane_u32<8>(c);
      if (lanes_per_row > 16) c += xor_lane_u32<16>(c);
      if (lanes_per_row > 32) c += xor_lane_u32<32>(c);
      if (v != PC_NONE && kw == 0) cnt[v] = c;
      for (uint32_t t = 0; t < teams && rem; ++t) rem &= rem - 1ull;  // the team's next
    }
  }
  __syncthreads();  // (the counts are read by other threads than wrote them)
  uint32_t size = 1;
  for (;;) {
    uint32_t bc = 0, bp = PC_NONE;
    if (tid < words) {  // the first of the largest count among this word's candidates, in ascending position
      unsigned long long rem = cand[tid];
      while (rem) {
        const uint32_t v = tid * 64u + (uint32_t)(__ffsll((long long)rem) - 1), c = cnt[v];
        if (bp == PC_NONE || c > bc) bc = c, bp = v;
        rem &= rem - 1ull;
      }
    }
    pc_first(bc, bp, wc, wp);
    if (bp == PC_NONE) break;  // (uniform) cand is empty
    unsigned long long keep = 0ull, out = 0ull;
    if (tid < words) {
      const unsigned long long old = cand[tid], rv = bits[(size_t)bp * words + tid];
      keep = old & rv, out = old & ~rv;  // (bit bp itself leaves: C_vv = 0)
      cand[tid] = keep, gone[tid] = out;
    }
    // the words of `gone` that are not empty, in ascending order
    const unsigned long long bal = __ballot(out != 0ull);
    if (lane == 0) wc[wv] = (uint32_t)__popcll(bal);
    __syncthreads();
    uint32_t off = 0, n_nz = 0;
    for (uint32_t q = 0; q < (uint32_t)WAVES; ++q) {
      if (q < wv) off += wc[q];
      n_nz += wc[q];
    }
    if (out != 0ull) nzw[off + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull))] = tid;
    if (tid == 0) mem[bp >> 6] |= 1ull << (bp & 63u);
    __syncthreads();
    if (tid < words) {  // popcount(row_u & cand) loses what row_u had in `gone`
      unsigned long long rem = keep;
      while (rem) {
        const uint32_t u = tid * 64u + (uint32_t)(__ffsll((long long)rem) - 1);
        const unsigned long long* ru = bits + (size_t)u * words;
        uint32_t sub = 0;
        for (uint32_t q = 0; q < n_nz; ++q) sub += (uint32_t)__popcll(ru[nzw[q]] & gone[nzw[q]]);
        cnt[u] -= sub;
        rem &= rem - 1ull;
      }
    }
    ++size;
    __syncthreads();
  }
  for (uint32_t k = tid; k < words; k += THREADS) mine[k] = mem[k];
  if (tid == 0) sizes[rank] = size;
}

// C6.  One work-group.  res: the winner's size, its rank, ok.
static __global__ __launch_bounds__(THREADS) void pc_choose_kernel(uint32_t L, uint32_t words, uint32_t n_seeds, uint32_t min_clique,
                                                                   const uint32_t* __restrict__ sizes, const unsigned long long* __restrict__ members,
                                                                   uint32_t* __restrict__ res /* [3] */, uint8_t* __restrict__ mask /* [L] */) {
  __shared__ uint32_t wc[WAVES], wp[WAVES];
  uint32_t bc = 0, bp = PC_NONE;
  for (uint32_t r = threadIdx.x; r < n_seeds; r += THREADS)
    if (pc_before(sizes[r], r, bc, bp)) bc = sizes[r], bp = r;
  pc_first(bc, bp, wc, wp);
  const bool ok = bc >= min_clique;
  if (threadIdx.x == 0) res[0] = bc, res[1] = bp, res[2] = ok ? 1u : 0u;
  const unsigned long long* m = members + (size_t)bp * words;
  for (uint32_t a = threadIdx.x; a < L; a += THREADS) mask[a] = ok ? (uint8_t)((m[a >> 6] >> (a & 63u)) & 1ull) : (uint8_t)0;
}

}  // namespace pgo
}  // namespace gloc
