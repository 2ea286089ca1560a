// pgo_kernels.hpp -- device side of the pose-graph optimisation (include/gloc3d.h, gloc_pgo_*; gfx950), all fp64.
// tests/pgo_ref.py is the contract; pgo.hip is the host side and owns the Levenberg-Marquardt loop.
//
//   fill_kernel / rowstart_kernel   the CSR (node -> incident edge, sign): entry 2 e is edge e at its source, 2 e + 1 at its
//                                   target; seg_sort.hpp's stable radix sort by node keeps the entries of a node in
//                                   ascending order, rowstart is a lower bound per node
//   linearize_kernel                one lane per edge: r, s2, the robust weight w and objective rho, W_e = w A^T Omega A
//                                   (21, upper triangle) and b_e = w A^T Omega r (6); the objective's per-work-group partial
//   gather_kernel                   one wave per node: g_k = sum +- b_e, H_kk = sum W_e, H_kk's Cholesky factor
//   pcg_init / pcg_matvec / pcg_update   block-Jacobi preconditioned conjugate gradients on (H + lambda D) x = -g
//   retract_kernel                  T_k <- (exp(w_k) R_k, exp(w_k) t_k + v_k) into the trial poses, the gain's denominator
//   finalize_kernel                 one work-group: the partials of the launches above into the scalars the host reads
//
// Determinism: no floating-point atomics.  A node's row is summed by one wave -- lane l adds the row's entries l, l + 64,
// ... in that order, then the 64 lanes are added by a butterfly (wave_sum) -- so a hub's row costs degree / 64 rounds, not
// degree.  Every scalar (the objective, the dot products of the PCG, the maxima) is a per-work-group partial in a slot of
// its own; a consumer adds the slots in one fixed order (sum_partials).  The grids are capped at MAX_GRID work-groups
// that stride over the work, so there are at most MAX_GRID partials and grid sizes depend on (n, m) alone.
// No work-group waits for another: alpha, beta and the stop test of the PCG are recomputed by EVERY work-group from the
// partials of the launch before, and the launches are ordered by the stream.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lane_ops.hpp"
#include "robust.hpp"

namespace gloc {
namespace pgo {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int MAX_GRID = 1024;  // work-groups of a strided launch = partials of a reduction

// what the host reads after a linearisation (finalize_kernel) and while the PCG runs
struct Scalars {
  double F, ginf, denom, max_w, max_v;
  uint32_t bad, pcg_iters, pcg_stop, pad_;
};

// one linearisation: per edge (structure of arrays, [k][m]) and per node (rows)
struct Lin {
  double *r, *s2, *w, *rho, *W, *b;  // [6][m], [m], [m], [m], [21][m], [6][m]
  double *g, *Hd, *Lf;               // [n][6], [n][21] upper triangle row-major, [n][21] lower factor row-major
  uint32_t* bad;                     // a free node whose block failed the pivot rule
};

__device__ __forceinline__ double wave_sum(double v) {
  v += xor_lane<32>(v);
  v += xor_lane<16>(v);
  v += xor_lane<8>(v);
  v += xor_lane<4>(v);
  v += xor_lane<2>(v);
  v += xor_lane<1>(v);
  return v;
}

// the work-group's sum, the same bits in every lane: waves by the butterfly, then the waves' sums in index order
__device__ __forceinline__ double block_sum(double v, double* red /* LDS [WAVES] */) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}
__device__ __forceinline__ double block_max(double v, double* red) {
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;  // (callers pass a wave-uniform value)
  __syncthreads();
  return fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
}
__device__ __forceinline__ double sum_partials(const double* __restrict__ part, uint32_t cnt, double* red) {
  double s = 0.0;
  for (uint32_t i = threadIdx.x; i < cnt; i += THREADS) s += part[i];
  return block_sum(s, red);
}
__device__ __forceinline__ double max_partials(const double* __restrict__ part, uint32_t cnt, double* red) {
  double s = 0.0;
  for (uint32_t i = threadIdx.x; i < cnt; i += THREADS) s = fmax(s, part[i]);
  s = fmax(s, xor_lane<32>(s));
  s = fmax(s, xor_lane<16>(s));
  s = fmax(s, xor_lane<8>(s));
  s = fmax(s, xor_lane<4>(s));
  s = fmax(s, xor_lane<2>(s));
  s = fmax(s, xor_lane<1>(s));
  return block_max(s, red);
}

// the objective whose derivative in s2 is robust::weight
__device__ __forceinline__ double rho_of(uint32_t kind, double s2, double c2) {
  const double t = s2 / c2;
  switch (kind) {
    case GLOC_ROBUST_HUBER: return t <= 1.0 ? s2 : c2 * (2.0 * sqrt(t) - 1.0);
    case GLOC_ROBUST_CAUCHY: return c2 * log1p(t);
    case GLOC_ROBUST_TUKEY: {
      const double u = 1.0 - t;
      return t <= 1.0 ? (c2 / 3.0) * (1.0 - u * u * u) : c2 / 3.0;
    }
    case GLOC_ROBUST_GEMAN_MCCLURE: return s2 / (1.0 + t);
    default: return s2;
  }
}
__device__ __forceinline__ double weight_of_dev(uint32_t kind, double s2, double c2) {
  switch (kind) {
    case GLOC_ROBUST_HUBER: return robust::weight<GLOC_ROBUST_HUBER>(s2, c2);
    case GLOC_ROBUST_CAUCHY: return robust::weight<GLOC_ROBUST_CAUCHY>(s2, c2);
    case GLOC_ROBUST_TUKEY: return robust::weight<GLOC_ROBUST_TUKEY>(s2, c2);
    case GLOC_ROBUST_GEMAN_MCCLURE: return robust::weight<GLOC_ROBUST_GEMAN_MCCLURE>(s2, c2);
    default: return 1.0;
  }
}

// index of (a, b), a <= b, in the row-major upper triangle of a 6 x 6 matrix
__host__ __device__ constexpr int ut(int a, int b) { return a * 6 - a * (a - 1) / 2 + (b - a); }
__device__ __forceinline__ double sym(const double* U, int a, int b) { return a <= b ? U[ut(a, b)] : U[ut(b, a)]; }

// ---- the CSR ----------------------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(THREADS) void fill_kernel(const uint32_t* __restrict__ src, const uint32_t* __restrict__ tgt, uint32_t m,
                                                              uint32_t* __restrict__ key, uint32_t* __restrict__ val) {
  const uint32_t q = blockIdx.x * THREADS + threadIdx.x;
  if (q >= 2u * m) return;
  key[q] = (q & 1u) ? tgt[q >> 1] : src[q >> 1];
  val[q] = q;
}

__device__ __forceinline__ uint32_t lower_bound(const uint32_t* __restrict__ key, uint32_t cnt, uint32_t x) {
  uint32_t lo = 0, hi = cnt;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (key[mid] < x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// row[k] for k in [0, n]; free[k] for k in [0, n)
static __global__ __launch_bounds__(THREADS) void rowstart_kernel(const uint32_t* __restrict__ key, uint32_t cnt, uint32_t n,
                                                                  const uint8_t* __restrict__ fixed, uint32_t* __restrict__ row,
                                                                  uint8_t* __restrict__ free_) {
  const uint32_t k = blockIdx.x * THREADS + threadIdx.x;
  if (k > n) return;
  const uint32_t a = lower_bound(key, cnt, k);
  row[k] = a;
  if (k < n) free_[k] = (!fixed[k] && lower_bound(key, cnt, k + 1) > a) ? 1 : 0;
}

// ---- the linearisation ------------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(THREADS) void linearize_kernel(uint32_t m, const uint32_t* __restrict__ src, const uint32_t* __restrict__ tgt,
                                                                   const float* __restrict__ Zf /* [12][m] */, const double* __restrict__ Om /* [21][m] */,
                                                                   const uint8_t* __restrict__ mask, uint32_t kind, double c2,
                                                                   const double* __restrict__ P /* [n][12] */, Lin L, double* __restrict__ part_F) {
  __shared__ double red[WAVES];
  double F = 0.0;
  for (uint32_t e = blockIdx.x * THREADS + threadIdx.x; e < m; e += gridDim.x * THREADS) {
    const double* Pi = P + 12 * (size_t)src[e];
    const double* Pj = P + 12 * (size_t)tgt[e];
    double Ri[9], Rj[9], Rz[9], ti[3], tj[3], tz[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) Ri[k] = Pi[k], Rj[k] = Pj[k], Rz[k] = (double)Zf[(size_t)k * m + e];
#pragma unroll
    for (int k = 0; k < 3; ++k) ti[k] = Pi[9 + k], tj[k] = Pj[9 + k], tz[k] = (double)Zf[(size_t)(9 + k) * m + e];
    // R_E = R_j^T R_i R_Z^T
    double M[9], RE[9];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) M[3 * a + b] = (Rj[a] * Ri[b] + Rj[3 + a] * Ri[3 + b]) + Rj[6 + a] * Ri[6 + b];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) RE[3 * a + b] = (M[3 * a] * Rz[3 * b] + M[3 * a + 1] * Rz[3 * b + 1]) + M[3 * a + 2] * Rz[3 * b + 2];
    double u[3], r[6];  // u = R_E t_Z
#pragma unroll
    for (int a = 0; a < 3; ++a) u[a] = (RE[3 * a] * tz[0] + RE[3 * a + 1] * tz[1]) + RE[3 * a + 2] * tz[2];
    const double d0 = ti[0] - tj[0], d1 = ti[1] - tj[1], d2 = ti[2] - tj[2];
#pragma unroll
    for (int a = 0; a < 3; ++a) r[3 + a] = ((Rj[a] * d0 + Rj[3 + a] * d1) + Rj[6 + a] * d2) - u[a];
    // log R_E: v = vee(R_E - R_E^T) / 2 has |v| = sin th
    {
      const double v0 = 0.5 * (RE[7] - RE[5]), v1 = 0.5 * (RE[2] - RE[6]), v2 = 0.5 * (RE[3] - RE[1]);
      const double s = sqrt((v0 * v0 + v1 * v1) + v2 * v2), c = (((RE[0] + RE[4]) + RE[8]) - 1.0) * 0.5;
      const double f = s < 1e-8 ? 1.0 + s * s / 6.0 : atan2(s, c) / s;
      r[0] = v0 * f, r[1] = v1 * f, r[2] = v2 * f;
    }
    // A = [Jl^-1(w) R_j^T, 0; [u]x R_j^T - R_j^T [t_i]x, R_j^T]: rows 0-2 have three columns, rows 3-5 six
    double A1[9], A2[9];  // A[0:3][0:3] and A[3:6][0:3]; A[3:6][3:6] = R_j^T
    {
      const double wx = r[0], wy = r[1], wz = r[2];
      const double th2 = (wx * wx + wy * wy) + wz * wz, th = sqrt(th2);
      double cc = 1.0 / 12.0;
      if (!(th < 1e-6)) cc = 1.0 / (th * th) - (1.0 + cos(th)) / (2.0 * th * sin(th));
      const double J[9] = {1.0 + cc * (-(wz * wz) - wy * wy), 0.5 * wz + cc * (wx * wy),           -0.5 * wy + cc * (wx * wz),
                           -0.5 * wz + cc * (wx * wy),          1.0 + cc * (-(wz * wz) - wx * wx), 0.5 * wx + cc * (wy * wz),
                           0.5 * wy + cc * (wx * wz),           -0.5 * wx + cc * (wy * wz),          1.0 + cc * (-(wy * wy) - wx * wx)};
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) A1[3 * a + b] = (J[3 * a] * Rj[3 * b] + J[3 * a + 1] * Rj[3 * b + 1]) + J[3 * a + 2] * Rj[3 * b + 2];
      // ([u]x R_j^T)[a][b] = sum_k [u]x[a][k] Rj[b][k];  (R_j^T [t_i]x)[a][b] = sum_k Rj[k][a] [t_i]x[k][b]
      const double ux[9] = {0.0, -u[2], u[1], u[2], 0.0, -u[0], -u[1], u[0], 0.0};
      const double tx[9] = {0.0, -ti[2], ti[1], ti[2], 0.0, -ti[0], -ti[1], ti[0], 0.0};
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b)
          A2[3 * a + b] = ((ux[3 * a] * Rj[3 * b] + ux[3 * a + 1] * Rj[3 * b + 1]) + ux[3 * a + 2] * Rj[3 * b + 2]) -
                          ((Rj[a] * tx[b] + Rj[3 + a] * tx[3 + b]) + Rj[6 + a] * tx[6 + b]);
    }
    double O[21], y[6];
#pragma unroll
    for (int k = 0; k < 21; ++k) O[k] = Om[(size_t)k * m + e];
    double s2 = 0.0;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < 6; ++k) s += sym(O, a, k) * r[k];
      y[a] = s;
    }
#pragma unroll
    for (int a = 0; a < 6; ++a) s2 += r[a] * y[a];
    const uint32_t kd = (mask == nullptr || mask[e]) ? kind : (uint32_t)GLOC_ROBUST_NONE;
    const double w = weight_of_dev(kd, s2, c2), rh = rho_of(kd, s2, c2);
    F += rh;
#pragma unroll
    for (int a = 0; a < 6; ++a) L.r[(size_t)a * m + e] = r[a];
    L.s2[e] = s2, L.w[e] = w, L.rho[e] = rh;
    // A[k][b]: the entry of A (k row, b column)
    auto Aat = [&](int k, int b) -> double {
      if (k < 3) return b < 3 ? A1[3 * k + b] : 0.0;
      return b < 3 ? A2[3 * (k - 3) + b] : Rj[3 * (b - 3) + (k - 3)];
    };
#pragma unroll
    for (int a = 0; a < 6; ++a) {  // b_e = w A^T y
      double s = 0.0;
#pragma unroll
      for (int k = (a < 3 ? 0 : 3); k < 6; ++k) s += Aat(k, a) * y[k];
      L.b[(size_t)a * m + e] = w * s;
    }
#pragma unroll
    for (int b = 0; b < 6; ++b) {  // column b of Omega A, then column b of W's upper triangle
      double col[6];
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        double s = 0.0;
#pragma unroll
        for (int q = (b < 3 ? 0 : 3); q < 6; ++q) s += sym(O, k, q) * Aat(q, b);
        col[k] = s;
      }
#pragma unroll
      for (int a = 0; a <= b; ++a) {
        double s = 0.0;
#pragma unroll
        for (int k = (a < 3 ? 0 : 3); k < 6; ++k) s += Aat(k, a) * col[k];
        L.W[(size_t)ut(a, b) * m + e] = w * s;
      }
    }
  }
  const double tot = block_sum(F, red);
  if (threadIdx.x == 0) part_F[blockIdx.x] = tot;
}

// 6 x 6 Cholesky with gn6_kernels.hpp's pivot rule.  H: upper triangle (21); Lf: the lower factor, row-major (21).
__device__ inline bool chol6(const double* H, double* Lf) {
  double L[6][6];
  double dmax = 0.0;
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int b = a; b < 6; ++b) L[a][b] = L[b][a] = H[ut(a, b)];
#pragma unroll
  for (int a = 0; a < 6; ++a) dmax = L[a][a] > dmax ? L[a][a] : dmax;
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double d = L[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
    if (!(d > 1e-12 * dmax)) ok = false;
    const double dj = ok ? sqrt(d) : 1.0;
    L[j][j] = dj;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double s = L[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k];
      L[i][j] = s / dj;
    }
  }
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = 0; j <= i; ++j) Lf[i * (i + 1) / 2 + j] = ok ? L[i][j] : (i == j ? 1.0 : 0.0);
  return ok;
}

// z = (L L^T)^-1 r * scale
__device__ __forceinline__ void chol_solve(const double* __restrict__ Lf, const double* r, double scale, double* z) {
  double y[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double s = r[i];
#pragma unroll
    for (int k = 0; k < i; ++k) s -= Lf[i * (i + 1) / 2 + k] * y[k];
    y[i] = s / Lf[i * (i + 1) / 2 + i];
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    double s = y[i];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) s -= Lf[k * (k + 1) / 2 + i] * z[k];
    z[i] = s / Lf[i * (i + 1) / 2 + i];
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) z[i] *= scale;
}

// one wave per node (strided): g, H_kk, its factor; the work-group's max |g| over the free nodes
static __global__ __launch_bounds__(THREADS) void gather_kernel(uint32_t n, uint32_t m, const uint32_t* __restrict__ row, const uint32_t* __restrict__ csr,
                                                                const uint8_t* __restrict__ free_, Lin L, double* __restrict__ part_ginf) {
  __shared__ double red[WAVES];
  const int lane = threadIdx.x & 63;
  const uint32_t wave = blockIdx.x * WAVES + (threadIdx.x >> 6), n_waves = gridDim.x * WAVES;
  double ginf = 0.0;
  for (uint32_t k = wave; k < n; k += n_waves) {
    double acc[27];
#pragma unroll
    for (int c = 0; c < 27; ++c) acc[c] = 0.0;
    const uint32_t end = row[k + 1];
    for (uint32_t q = row[k] + lane; q < end; q += 64) {
      const uint32_t code = csr[q], e = code >> 1;
      const double sg = (code & 1u) ? -1.0 : 1.0;
#pragma unroll
      for (int c = 0; c < 6; ++c) acc[c] += sg * L.b[(size_t)c * m + e];
#pragma unroll
      for (int c = 0; c < 21; ++c) acc[6 + c] += L.W[(size_t)c * m + e];
    }
#pragma unroll
    for (int c = 0; c < 27; ++c) acc[c] = wave_sum(acc[c]);
    if (lane == 0) {
      double Lf[21];
      const bool ok = chol6(acc + 6, Lf);
#pragma unroll
      for (int c = 0; c < 6; ++c) L.g[6 * (size_t)k + c] = acc[c];
#pragma unroll
      for (int c = 0; c < 21; ++c) L.Hd[21 * (size_t)k + c] = acc[6 + c], L.Lf[21 * (size_t)k + c] = Lf[c];
      if (free_[k]) {
        if (!ok) *L.bad = 1u;
#pragma unroll
        for (int c = 0; c < 6; ++c) ginf = fmax(ginf, fabs(acc[c]));
      }
    }
  }
  const double tot = block_max(ginf, red);  // (a wave's first lane holds the wave's maximum, and block_max reads that lane)
  if (threadIdx.x == 0) part_ginf[blockIdx.x] = tot;
}

// ---- the PCG ------------------------------------------------------------------------------------------------------------
struct Pcg {
  double *x, *r, *z, *Ap, *p[2];               // [n][6]
  double *part_rr[2], *part_rz[2], *part_g2;   // [gu] each: the update launches' partials (by parity of the iteration)
  double* part_pAp;                            // [gm]: the matvec launch's
  Scalars* sc;
  uint32_t gu, gm;                             // work-groups of the lane-per-node and of the wave-per-node launches
};

__device__ __forceinline__ bool read_stop(const Scalars* sc, uint32_t* flag /* LDS */) {
  if (threadIdx.x == 0) *flag = sc->pcg_stop;
  __syncthreads();
  return *flag != 0;
}

static __global__ __launch_bounds__(THREADS) void pcg_init_kernel(uint32_t n, const uint8_t* __restrict__ free_, Lin L, double lambda, Pcg c) {
  __shared__ double red[WAVES];
  double rr = 0.0, rz = 0.0;
  for (uint32_t k = blockIdx.x * THREADS + threadIdx.x; k < n; k += gridDim.x * THREADS) {
    double r[6], z[6];
    if (free_[k]) {
#pragma unroll
      for (int a = 0; a < 6; ++a) r[a] = -L.g[6 * (size_t)k + a];
      chol_solve(L.Lf + 21 * (size_t)k, r, 1.0 / (1.0 + lambda), z);
    } else {
#pragma unroll
      for (int a = 0; a < 6; ++a) r[a] = 0.0, z[a] = 0.0;
    }
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      c.r[6 * (size_t)k + a] = r[a], c.z[6 * (size_t)k + a] = z[a], c.x[6 * (size_t)k + a] = 0.0;
      c.p[0][6 * (size_t)k + a] = 0.0, c.p[1][6 * (size_t)k + a] = 0.0;
      rr += r[a] * r[a], rz += r[a] * z[a];
    }
  }
  const double trr = block_sum(rr, red), trz = block_sum(rz, red);
  if (threadIdx.x == 0) {
    c.part_rr[0][blockIdx.x] = trr, c.part_g2[blockIdx.x] = trr, c.part_rz[0][blockIdx.x] = trz;
    if (blockIdx.x == 0) c.sc->pcg_stop = 0u;
  }
}

// iteration `it`: p = z + beta p (beta = 0 at it = 0) for this node and, on the fly, for its neighbours; Ap = (H + lambda D) p
static __global__ __launch_bounds__(THREADS) void pcg_matvec_kernel(uint32_t n, uint32_t m, uint32_t it, double lambda, double tol2,
                                                                    const uint32_t* __restrict__ row, const uint32_t* __restrict__ csr,
                                                                    const uint32_t* __restrict__ src, const uint32_t* __restrict__ tgt,
                                                                    const uint8_t* __restrict__ free_, Lin L, Pcg c) {
  __shared__ double red[WAVES];
  __shared__ uint32_t flag;
  if (read_stop(c.sc, &flag)) return;
  const double rr = sum_partials(c.part_rr[it & 1], c.gu, red), g2 = sum_partials(c.part_g2, c.gu, red);
  if (rr <= tol2 * g2) {
    if (blockIdx.x == 0 && threadIdx.x == 0) c.sc->pcg_stop = 1u;
    return;
  }
  double beta = 0.0;
  if (it > 0) beta = sum_partials(c.part_rz[it & 1], c.gu, red) / sum_partials(c.part_rz[(it - 1) & 1], c.gu, red);
  const double* __restrict__ po = c.p[(it & 1) ^ 1];
  double* __restrict__ pn = c.p[it & 1];
  const int lane = threadIdx.x & 63;
  const uint32_t wave = blockIdx.x * WAVES + (threadIdx.x >> 6), n_waves = gridDim.x * WAVES;
  double pAp = 0.0;
  for (uint32_t k = wave; k < n; k += n_waves) {
    double pk[6], acc[6];
#pragma unroll
    for (int a = 0; a < 6; ++a) acc[a] = 0.0;
    if (!free_[k]) {  // (wave-uniform)
      if (lane == 0)
#pragma unroll
        for (int a = 0; a < 6; ++a) pn[6 * (size_t)k + a] = 0.0, c.Ap[6 * (size_t)k + a] = 0.0;
      continue;
    }
#pragma unroll
    for (int a = 0; a < 6; ++a) pk[a] = c.z[6 * (size_t)k + a] + beta * po[6 * (size_t)k + a];
    const uint32_t end = row[k + 1];
    for (uint32_t q = row[k] + lane; q < end; q += 64) {
      const uint32_t code = csr[q], e = code >> 1;
      const uint32_t o = (code & 1u) ? src[e] : tgt[e];  // the other end: W_e (p_k - p_o) whichever end k is
      double d[6];
#pragma unroll
      for (int a = 0; a < 6; ++a) d[a] = pk[a] - (c.z[6 * (size_t)o + a] + beta * po[6 * (size_t)o + a]);
      double W[21];
#pragma unroll
      for (int a = 0; a < 21; ++a) W[a] = L.W[(size_t)a * m + e];
#pragma unroll
      for (int a = 0; a < 6; ++a) {
        double s = 0.0;
#pragma unroll
        for (int b = 0; b < 6; ++b) s += sym(W, a, b) * d[b];
        acc[a] += s;
      }
    }
#pragma unroll
    for (int a = 0; a < 6; ++a) acc[a] = wave_sum(acc[a]);
    if (lane == 0) {
      const double* H = L.Hd + 21 * (size_t)k;
#pragma unroll
      for (int a = 0; a < 6; ++a) {
        double s = 0.0;
#pragma unroll
        for (int b = 0; b < 6; ++b) s += sym(H, a, b) * pk[b];
        const double ap = acc[a] + lambda * s;
        pn[6 * (size_t)k + a] = pk[a], c.Ap[6 * (size_t)k + a] = ap;
        pAp += pk[a] * ap;
      }
    }
  }
  const double tot = block_sum(pAp, red);  // (lanes other than a wave's first hold 0)
  if (threadIdx.x == 0) c.part_pAp[blockIdx.x] = tot;
}

static __global__ __launch_bounds__(THREADS) void pcg_update_kernel(uint32_t n, uint32_t it, double lambda, double tol2,
                                                                    const uint8_t* __restrict__ free_, Lin L, Pcg c) {
  __shared__ double red[WAVES];
  __shared__ uint32_t flag;
  if (read_stop(c.sc, &flag)) return;
  const double rr0 = sum_partials(c.part_rr[it & 1], c.gu, red), g2 = sum_partials(c.part_g2, c.gu, red);
  if (rr0 <= tol2 * g2) return;  // (the matvec launch before this one has set the flag)
  const double pAp = sum_partials(c.part_pAp, c.gm, red), rz0 = sum_partials(c.part_rz[it & 1], c.gu, red);
  if (!(pAp > 0.0)) {  // a breakdown: x stays
    if (blockIdx.x == 0 && threadIdx.x == 0) c.sc->pcg_stop = 1u;
    return;
  }
  const double alpha = rz0 / pAp;
  const double* __restrict__ p = c.p[it & 1];
  double rr = 0.0, rz = 0.0;
  for (uint32_t k = blockIdx.x * THREADS + threadIdx.x; k < n; k += gridDim.x * THREADS) {
    if (!free_[k]) continue;
    double r[6], z[6];
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      c.x[6 * (size_t)k + a] += alpha * p[6 * (size_t)k + a];
      r[a] = c.r[6 * (size_t)k + a] - alpha * c.Ap[6 * (size_t)k + a];
    }
    chol_solve(L.Lf + 21 * (size_t)k, r, 1.0 / (1.0 + lambda), z);
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      c.r[6 * (size_t)k + a] = r[a], c.z[6 * (size_t)k + a] = z[a];
      rr += r[a] * r[a], rz += r[a] * z[a];
    }
  }
  const double trr = block_sum(rr, red), trz = block_sum(rz, red);
  if (threadIdx.x == 0) {
    c.part_rr[(it + 1) & 1][blockIdx.x] = trr, c.part_rz[(it + 1) & 1][blockIdx.x] = trz;
    if (blockIdx.x == 0) c.sc->pcg_iters += 1u;
  }
}

// ---- the step -----------------------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(THREADS) void retract_kernel(uint32_t n, const uint8_t* __restrict__ free_, const double* __restrict__ x, Lin L,
                                                                 double lambda, const double* __restrict__ P, double* __restrict__ Pn,
                                                                 double* __restrict__ part_den, double* __restrict__ part_w, double* __restrict__ part_v) {
  __shared__ double red[WAVES];
  double den = 0.0, mw = 0.0, mv = 0.0;
  for (uint32_t k = blockIdx.x * THREADS + threadIdx.x; k < n; k += gridDim.x * THREADS) {
    double T[12];
#pragma unroll
    for (int a = 0; a < 12; ++a) T[a] = P[12 * (size_t)k + a];
    if (free_[k]) {
      double d[6];
#pragma unroll
      for (int a = 0; a < 6; ++a) d[a] = x[6 * (size_t)k + a];
      const double* H = L.Hd + 21 * (size_t)k;
#pragma unroll
      for (int a = 0; a < 6; ++a) {
        double s = 0.0;
#pragma unroll
        for (int b = 0; b < 6; ++b) s += sym(H, a, b) * d[b];
        den += d[a] * (lambda * s - L.g[6 * (size_t)k + a]);
      }
      const double wx = d[0], wy = d[1], wz = d[2];
      const double th2 = (wx * wx + wy * wy) + wz * wz, th = sqrt(th2);
      mw = fmax(mw, th), mv = fmax(mv, sqrt((d[3] * d[3] + d[4] * d[4]) + d[5] * d[5]));
      double A = 1.0, B = 0.5;  // Rodrigues as chol_rodrigues (gn6_kernels.hpp) states it
      if (th > 0.0) {
        A = sin(th) / th;
        const double sh = sin(0.5 * th);
        B = 2.0 * (sh * sh) / th2;
      }
      const double K[9] = {0.0, -wz, wy, wz, 0.0, -wx, -wy, wx, 0.0};
      double E[9], Tn[12];
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) {
          const double k2 = (K[3 * a] * K[b] + K[3 * a + 1] * K[3 + b]) + K[3 * a + 2] * K[6 + b];
          E[3 * a + b] = ((a == b ? 1.0 : 0.0) + A * K[3 * a + b]) + B * k2;
        }
#pragma unroll
      for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int b = 0; b < 3; ++b) Tn[3 * a + b] = (E[3 * a] * T[b] + E[3 * a + 1] * T[3 + b]) + E[3 * a + 2] * T[6 + b];
        Tn[9 + a] = ((E[3 * a] * T[9] + E[3 * a + 1] * T[10]) + E[3 * a + 2] * T[11]) + d[3 + a];
      }
#pragma unroll
      for (int a = 0; a < 12; ++a) T[a] = Tn[a];
    }
#pragma unroll
    for (int a = 0; a < 12; ++a) Pn[12 * (size_t)k + a] = T[a];
  }
  const double tden = block_sum(den, red);
  mw = fmax(mw, xor_lane<32>(mw)), mv = fmax(mv, xor_lane<32>(mv));
  mw = fmax(mw, xor_lane<16>(mw)), mv = fmax(mv, xor_lane<16>(mv));
  mw = fmax(mw, xor_lane<8>(mw)), mv = fmax(mv, xor_lane<8>(mv));
  mw = fmax(mw, xor_lane<4>(mw)), mv = fmax(mv, xor_lane<4>(mv));
  mw = fmax(mw, xor_lane<2>(mw)), mv = fmax(mv, xor_lane<2>(mv));
  mw = fmax(mw, xor_lane<1>(mw)), mv = fmax(mv, xor_lane<1>(mv));
  const double tw = block_max(mw, red), tv = block_max(mv, red);
  if (threadIdx.x == 0) part_den[blockIdx.x] = tden, part_w[blockIdx.x] = tw, part_v[blockIdx.x] = tv;
}

// one work-group: what the host reads about the linearisation L and the step that led to it
static __global__ __launch_bounds__(THREADS) void finalize_kernel(Lin L, const double* __restrict__ part_F, uint32_t ge, const double* __restrict__ part_ginf,
                                                                  uint32_t gm, const double* __restrict__ part_den, const double* __restrict__ part_w,
                                                                  const double* __restrict__ part_v, uint32_t gu, Scalars* __restrict__ sc) {
  __shared__ double red[WAVES];
  const double F = sum_partials(part_F, ge, red), ginf = max_partials(part_ginf, gm, red);
  const double den = sum_partials(part_den, gu, red), mw = max_partials(part_w, gu, red), mv = max_partials(part_v, gu, red);
  if (threadIdx.x == 0) sc->F = F, sc->ginf = ginf, sc->denom = den, sc->max_w = mw, sc->max_v = mv, sc->bad = *L.bad;
}

}  // namespace pgo
}  // namespace gloc
