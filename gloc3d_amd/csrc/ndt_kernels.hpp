// ndt_kernels.hpp -- NDT scan registration on gfx950 (gloc_reg_ndt_*, gloc_scan_store_add_approx_voxel): the device
// half of tests/ndt_ref.py, which states every step below in float64 numpy.  Included by ndt.hip alone.  The kernels that
// key, sort, scan and hash the cells are voxel_map_kernels.hpp's, shared with the voxelized generalized ICP; what a cell
// holds (Cell, cell_stats_kernel) is here.
//
//   approximate voxel filter   avf_keys_kernel -> segmented radix sort by hash slot (stable) -> avf_flags_kernel
//                              (a run of equal cells inside a slot starts here) -> flag scan -> avf_emit_kernel (the
//                              run's fp32 sum in point order / count)
//   cells of the targets       the voxel map of voxel_map_kernels.hpp with cell_stats_kernel as its statistics kernel
//                              (fp64 sums relative to the cell corner, Jacobi eigen, inflation, inverse)
//   Newton / More-Thuente      rounds of (ndt_deriv_kernel: score + gradient [+ Hessian] partials per work-group,
//                              ndt_state_kernel: one wave per candidate sums them in block order and steps its state)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "math3.hpp"
#include "voxel_map_kernels.hpp"

namespace gloc {
namespace ndt {

using voxmap::KEY_BIAS;
using voxmap::KEY_NONE;
using voxmap::TgtDesc;
using voxmap::hash_slot;
using voxmap::pack_key;

constexpr int HIST = 512;                     // ApproximateVoxelGrid's slots
constexpr uint32_t AVF_INVALID = HIST;        // slot key of a point the filter skips (sorts last)
constexpr int NACC = 28;                      // score, gradient 6, Hessian upper triangle 21
constexpr int DERIV_THREADS = 256;
constexpr int PTS_PER_THREAD = 2;
constexpr int CHUNK = DERIV_THREADS * PTS_PER_THREAD;  // filtered source points per work-group

enum Phase : int { PH_INIT = 0, PH_FIRST = 1, PH_MORE = 2, PH_HESS = 3, PH_DONE = 4 };

// What the derivative kernel needs of one candidate's pose: T = [R | t] and the angle derivative matrices (dR/da_k and
// d2R/da_k da_l, k <= l, with PCL's small-angle rule), fp64.
struct Eval {
  int active, hess, pad0, pad1;
  double R[9], t[3], M[3][9], MH[6][9];
};

// One candidate's Newton / More-Thuente state (tests/ndt_ref.py::align), fp64.
struct State {
  int phase, converged, iters, step_iters, open_interval, interval_converged, stepped, tgt;
  double p[6], dir[6], x_t[6];
  double score, g[6], H[36];
  double phi_0, dphi_0, a_t, I[6];
  double n_src, step_max, step_min, eps;
  int max_iters, pad;
};

struct Out {
  float T[16];
  double prob;
  uint32_t iters;
  int converged;
};

struct Cell {
  unsigned long long key;
  uint32_t count, valid;
  double mean[3];
  double icov[6];  // xx xy xz yy yz zz
};

struct Consts {
  double res, inv_res, d1, d2;
};

// ---- small fp64 helpers ---------------------------------------------------------------------------------------------
__host__ __device__ inline void rot_elem(int axis, double c, double s, double* M) {
  for (int i = 0; i < 9; ++i) M[i] = 0.0;
  if (axis == 0) {
    M[0] = 1; M[4] = c; M[5] = -s; M[7] = s; M[8] = c;
  } else if (axis == 1) {
    M[0] = c; M[2] = s; M[4] = 1; M[6] = -s; M[8] = c;
  } else {
    M[0] = c; M[1] = -s; M[3] = s; M[4] = c; M[8] = 1;
  }
}
// d^order / da^order of the elementary rotation (tests/ndt_ref.py::_drot)
__host__ __device__ inline void drot_elem(int axis, double c, double s, int order, double* M) {
  const double c_ = order == 1 ? -s : -c, s_ = order == 1 ? c : -s;
  rot_elem(axis, c_, s_, M);
  M[4 * axis] = 0.0;
}
__host__ __device__ inline void mul3(const double* A, const double* B, double* C) {
  double T[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) T[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
  for (int i = 0; i < 9; ++i) C[i] = T[i];
}

// T(p) and the derivative matrices at p (tests/ndt_ref.py::pose_matrix, angle_derivatives)
__host__ __device__ inline void make_eval(const double* p, Eval* e) {
  double E[3][9], D1[3][9], D2[3][9], A[9];
  for (int a = 0; a < 3; ++a) {
    rot_elem(a, cos(p[3 + a]), sin(p[3 + a]), E[a]);
  }
  mul3(E[0], E[1], A);
  mul3(A, E[2], e->R);
  for (int i = 0; i < 3; ++i) e->t[i] = p[i];
  for (int a = 0; a < 3; ++a) {
    const bool small = fabs(p[3 + a]) < 1e-4;
    const double c = small ? 1.0 : cos(p[3 + a]), s = small ? 0.0 : sin(p[3 + a]);
    rot_elem(a, c, s, E[a]);
    drot_elem(a, c, s, 1, D1[a]);
    drot_elem(a, c, s, 2, D2[a]);
  }
  for (int k = 0; k < 3; ++k) {
    const double* f0 = k == 0 ? D1[0] : E[0];
    const double* f1 = k == 1 ? D1[1] : E[1];
    const double* f2 = k == 2 ? D1[2] : E[2];
    mul3(f0, f1, A);
    mul3(A, f2, e->M[k]);
  }
  int m = 0;
  for (int k = 0; k < 3; ++k)
    for (int l = k; l < 3; ++l, ++m) {
      int o[3] = {0, 0, 0};
      o[k]++;
      o[l]++;
      const double* f[3];
      for (int a = 0; a < 3; ++a) f[a] = o[a] == 0 ? E[a] : o[a] == 1 ? D1[a] : D2[a];
      mul3(f[0], f[1], A);
      mul3(A, f[2], e->MH[m]);
    }
}

// Eigen's R.eulerAngles(0, 1, 2), fp64 (tests/ndt_ref.py::euler_xyz)
__host__ __device__ inline void euler_xyz(const double* R, double* out) {
  const double PI = 3.14159265358979323846;
  double r0 = atan2(R[5], R[8]);
  const double c2 = hypot(R[0], R[1]);
  double r1;
  if (r0 > 0) {
    r0 -= PI;
    r1 = atan2(-R[2], -c2);
  } else {
    r1 = atan2(-R[2], c2);
  }
  const double s1 = sin(r0), c1 = cos(r0);
  const double r2 = atan2(s1 * R[6] - c1 * R[3], c1 * R[4] - s1 * R[7]);
  out[0] = -r0;
  out[1] = -r1;
  out[2] = -r2;
}

// cyclic Jacobi on a symmetric 6x6 (A destroyed: its diagonal ends as the eigenvalues, V's columns the vectors)
__device__ inline void jacobi_eig6(double* A, double* V) {
  for (int i = 0; i < 36; ++i) V[i] = (i % 7 == 0) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 50; ++sweep) {
    double off = 0.0, diag = 0.0;
    for (int i = 0; i < 6; ++i) {
      diag += A[7 * i] * A[7 * i];
      for (int j = i + 1; j < 6; ++j) off += A[6 * i + j] * A[6 * i + j];
    }
    if (off <= 1e-34 * diag || off == 0.0) break;
    for (int p = 0; p < 5; ++p)
      for (int q = p + 1; q < 6; ++q) {
        const double apq = A[6 * p + q];
        if (apq == 0.0) continue;
        const double theta = (A[7 * q] - A[7 * p]) / (2.0 * apq);
        double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
        if (theta < 0) t = -t;
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < 6; ++k) {
          const double akp = A[6 * k + p], akq = A[6 * k + q];
          A[6 * k + p] = c * akp - s * akq;
          A[6 * k + q] = s * akp + c * akq;
        }
        for (int k = 0; k < 6; ++k) {
          const double apk = A[6 * p + k], aqk = A[6 * q + k];
          A[6 * p + k] = c * apk - s * aqk;
          A[6 * q + k] = s * apk + c * aqk;
        }
        for (int k = 0; k < 6; ++k) {
          const double vkp = V[6 * k + p], vkq = V[6 * k + q];
          V[6 * k + p] = c * vkp - s * vkq;
          V[6 * k + q] = s * vkp + c * vkq;
        }
      }
  }
}

// ---- approximate voxel filter ----------------------------------------------------------------------------------------
__device__ inline bool avf_cell(const float* __restrict__ xyz, uint32_t i, float inv, int* k) {
  bool ok = true;
  for (int a = 0; a < 3; ++a) {
    const float f = floorf(xyz[3 * i + a] * inv);
    ok = ok && fabsf(f) < 1073741824.f;  // finite, and an int32 holds it
    k[a] = ok ? (int)f : 0;
  }
  return ok;
}

static __global__ void avf_keys_kernel(const float* __restrict__ xyz, uint32_t n, float inv, uint32_t* __restrict__ key,
                                uint32_t* __restrict__ val) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int k[3];
  const bool ok = avf_cell(xyz, i, inv, k);
  const uint32_t h = ((uint32_t)k[0] * 7171u + (uint32_t)k[1] * 3079u + (uint32_t)k[2] * 4231u) & (uint32_t)(HIST - 1);
  key[i] = ok ? h : AVF_INVALID;
  val[i] = i;
}

// single: no filter (leaf <= 0), every finite point is a run of its own, unsorted
static __global__ void avf_flags_kernel(const float* __restrict__ xyz, uint32_t n, float inv, const uint32_t* __restrict__ key,
                                 const uint32_t* __restrict__ val, uint32_t* __restrict__ flag, int single) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const uint32_t h = key[j];
  uint32_t f = 0;
  if (h != AVF_INVALID) {
    if (single || j == 0 || key[j - 1] != h) {
      f = 1;
    } else {
      int a[3], b[3];
      avf_cell(xyz, val[j], inv, a);
      avf_cell(xyz, val[j - 1], inv, b);
      f = (a[0] != b[0] || a[1] != b[1] || a[2] != b[2]) ? 1u : 0u;
    }
  }
  flag[j] = f;
}

// one thread per run: its fp32 sum in point order (the sort is stable), divided by the fp32 count
static __global__ void avf_emit_kernel(const float* __restrict__ xyz, uint32_t n, const uint32_t* __restrict__ key,
                                const uint32_t* __restrict__ val, const uint32_t* __restrict__ flag,
                                const uint32_t* __restrict__ pos, float* __restrict__ out, int single) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n || !flag[j]) return;
  float sx = 0.f, sy = 0.f, sz = 0.f;
  uint32_t c = 0;
  for (uint32_t t = j; t < n; ++t) {
    if (t > j && (single || flag[t] || key[t] == AVF_INVALID)) break;
    const uint32_t i = val[t];
    sx = sx + xyz[3 * i];
    sy = sy + xyz[3 * i + 1];
    sz = sz + xyz[3 * i + 2];
    ++c;
  }
  const float fc = (float)c;
  const uint32_t o = pos[j];
  out[3 * o] = sx / fc;
  out[3 * o + 1] = sy / fc;
  out[3 * o + 2] = sz / fc;
}

// ---- target cells (one thread per cell: the first of a run of equal keys) -------------------------------------------
__device__ inline void inv_sym3(const double* C, double* I) {  // cofactors / determinant (Eigen's 3x3 inverse)
  const double a = C[0], b = C[1], c = C[2], d = C[4], e = C[5], f = C[8];
  const double A = d * f - e * e, B = c * e - b * f, Cc = b * e - c * d;
  const double det = a * A + b * B + c * Cc;
  const double r = 1.0 / det;
  I[0] = A * r;
  I[1] = B * r;
  I[2] = Cc * r;
  I[3] = (a * f - c * c) * r;
  I[4] = (b * c - a * e) * r;
  I[5] = (a * d - b * b) * r;
}

static __global__ void cell_stats_kernel(const TgtDesc* __restrict__ tg, const unsigned long long* __restrict__ key,
                                  const uint32_t* __restrict__ val, const uint32_t* __restrict__ flag,
                                  const uint32_t* __restrict__ pos, double res, uint32_t min_pts, double eig_mult,
                                  Cell* __restrict__ cells) {
  const TgtDesc d = tg[blockIdx.y];
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= d.n || !flag[d.begin + i]) return;
  const unsigned long long k = key[d.begin + i];
  const double cx = (double)((long long)((k >> 42) & 0x1FFFFF) - KEY_BIAS) * res;
  const double cy = (double)((long long)((k >> 21) & 0x1FFFFF) - KEY_BIAS) * res;
  const double cz = (double)((long long)(k & 0x1FFFFF) - KEY_BIAS) * res;
  double s1[3] = {0, 0, 0}, s2[6] = {0, 0, 0, 0, 0, 0};
  uint32_t n = 0;
  for (uint32_t t = i; t < d.n && key[d.begin + t] == k; ++t) {
    const uint32_t j = val[d.begin + t];
    const double r[3] = {(double)d.xyz[3 * j] - cx, (double)d.xyz[3 * j + 1] - cy, (double)d.xyz[3 * j + 2] - cz};
    s1[0] += r[0]; s1[1] += r[1]; s1[2] += r[2];
    s2[0] += r[0] * r[0]; s2[1] += r[0] * r[1]; s2[2] += r[0] * r[2];
    s2[3] += r[1] * r[1]; s2[4] += r[1] * r[2]; s2[5] += r[2] * r[2];
    ++n;
  }
  Cell out;
  out.key = k;
  out.count = n;
  out.valid = 0;
  const double nd = (double)n;
  const double m[3] = {s1[0] / nd, s1[1] / nd, s1[2] / nd};
  out.mean[0] = cx + m[0];
  out.mean[1] = cy + m[1];
  out.mean[2] = cz + m[2];
  for (int q = 0; q < 6; ++q) out.icov[q] = 0.0;
  if (n >= min_pts) {
    const int ia[6] = {0, 0, 0, 1, 1, 2}, ib[6] = {0, 1, 2, 1, 2, 2};
    double C[9];
    for (int q = 0; q < 6; ++q) {
      const double v = ((s2[q] - 2.0 * s1[ia[q]] * m[ib[q]]) / nd + m[ia[q]] * m[ib[q]]) * ((nd - 1.0) / nd);
      C[3 * ia[q] + ib[q]] = v;
      C[3 * ib[q] + ia[q]] = v;
    }
    double A[9], V[9];
    for (int q = 0; q < 9; ++q) A[q] = C[q];
    gloc::reg::jacobi_eig3(A, V);
    double lam[3] = {A[0], A[4], A[8]};
    int o[3] = {0, 1, 2};  // ascending
    for (int a = 0; a < 2; ++a)
      for (int b = 0; b < 2 - a; ++b)
        if (lam[o[b]] > lam[o[b + 1]]) {
          const int t = o[b];
          o[b] = o[b + 1];
          o[b + 1] = t;
        }
    double l0 = lam[o[0]], l1 = lam[o[1]];
    const double l2 = lam[o[2]];
    if (!(l0 < 0 || l1 < 0 || l2 <= 0)) {
      const double lo = eig_mult * l2;
      if (l0 < lo) {
        l0 = lo;
        if (l1 < lo) l1 = lo;
        const double L[3] = {l0, l1, l2};
        for (int a = 0; a < 3; ++a)
          for (int b = 0; b < 3; ++b) {
            double s = 0.0;
            for (int c = 0; c < 3; ++c) s += V[3 * a + o[c]] * L[c] * V[3 * b + o[c]];
            C[3 * a + b] = s;
          }
      }
      double I[6];
      inv_sym3(C, I);
      bool fin = true;
      for (int q = 0; q < 6; ++q) fin = fin && isfinite(I[q]);
      if (fin) {
        out.valid = 1;
        for (int q = 0; q < 6; ++q) out.icov[q] = I[q];
      }
    }
  }
  cells[pos[d.begin + i]] = out;
}

// ---- derivatives -----------------------------------------------------------------------------------------------------
// grid (work-groups over the filtered source, candidates): per work-group the fp64 sums [score, g 6, H upper 21] of its
// CHUNK points, in a fixed order (lanes in order inside a wave by a butterfly, waves in order), no atomics
static __global__ __launch_bounds__(DERIV_THREADS) void ndt_deriv_kernel(
    const float* __restrict__ src, uint32_t n_src, const Eval* __restrict__ evals, const int* __restrict__ cand_tgt,
    const Cell* __restrict__ cells, const unsigned long long* __restrict__ hkey, const uint32_t* __restrict__ hval,
    const uint32_t* __restrict__ toff, const uint32_t* __restrict__ tmask, Consts K, double* __restrict__ partials) {
  const uint32_t c = blockIdx.y;
  __shared__ Eval E;
  __shared__ double red[DERIV_THREADS / 64][NACC];
  if (!evals[c].active) return;  // uniform: a finished candidate leaves at once
  for (int i = threadIdx.x; i < (int)(sizeof(Eval) / 8); i += DERIV_THREADS)
    reinterpret_cast<double*>(&E)[i] = reinterpret_cast<const double*>(&evals[c])[i];
  __syncthreads();
  const bool hess = E.hess != 0;
  const int t = cand_tgt[c];
  const unsigned long long* hk = hkey + toff[t];
  const uint32_t* hv = hval + toff[t];
  const uint32_t mask = tmask[t];
  double acc[NACC];
#pragma unroll
  for (int q = 0; q < NACC; ++q) acc[q] = 0.0;
  const double res2 = K.res * K.res;
  for (int r = 0; r < PTS_PER_THREAD; ++r) {
    const uint32_t i = blockIdx.x * CHUNK + r * DERIV_THREADS + threadIdx.x;
    if (i >= n_src) break;
    const double x[3] = {(double)src[3 * i], (double)src[3 * i + 1], (double)src[3 * i + 2]};
    double y[3];
    for (int a = 0; a < 3; ++a) y[a] = E.R[3 * a] * x[0] + E.R[3 * a + 1] * x[1] + E.R[3 * a + 2] * x[2] + E.t[a];
    if (!(isfinite(y[0]) && isfinite(y[1]) && isfinite(y[2]))) continue;
    long long home[3];
    bool inr = true;
    for (int a = 0; a < 3; ++a) {
      const double h = floor(y[a] * K.inv_res);
      inr = inr && fabs(h) < (double)(KEY_BIAS * 2);
      home[a] = inr ? (long long)h : 0;
    }
    if (!inr) continue;
    double J[3][3];  // dR/da_k x, column k of the angular part of the point Jacobian
    for (int k = 0; k < 3; ++k)
      for (int a = 0; a < 3; ++a) J[k][a] = E.M[k][3 * a] * x[0] + E.M[k][3 * a + 1] * x[1] + E.M[k][3 * a + 2] * x[2];
    for (int dz = -1; dz <= 1; ++dz)
      for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
          const long long kx = home[0] + dx, ky = home[1] + dy, kz = home[2] + dz;
          if (!(kx > -(KEY_BIAS - 1) && kx < KEY_BIAS - 1 && ky > -(KEY_BIAS - 1) && ky < KEY_BIAS - 1 &&
                kz > -(KEY_BIAS - 1) && kz < KEY_BIAS - 1))
            continue;
          const unsigned long long key = pack_key(kx, ky, kz);
          uint32_t s = hash_slot(key, mask);
          uint32_t ci = 0xFFFFFFFFu;
          while (true) {
            const unsigned long long hkv = hk[s];
            if (hkv == key) {
              ci = hv[s];
              break;
            }
            if (hkv == KEY_NONE) break;
            s = (s + 1) & mask;
          }
          if (ci == 0xFFFFFFFFu) continue;
          const Cell& C = cells[ci];
          const double d[3] = {y[0] - C.mean[0], y[1] - C.mean[1], y[2] - C.mean[2]};
          if (!(d[0] * d[0] + d[1] * d[1] + d[2] * d[2] < res2)) continue;
          const double* ic = C.icov;
          const double IC[9] = {ic[0], ic[1], ic[2], ic[1], ic[3], ic[4], ic[2], ic[4], ic[5]};
          double u[3];
          for (int a = 0; a < 3; ++a) u[a] = IC[3 * a] * d[0] + IC[3 * a + 1] * d[1] + IC[3 * a + 2] * d[2];
          const double qf = d[0] * u[0] + d[1] * u[1] + d[2] * u[2];
          const double e = exp(-K.d2 * qf / 2.0);
          const double de = K.d2 * e;
          if (!(de >= 0.0 && de <= 1.0)) continue;
          const double w = K.d1 * de;
          double av[6];
          av[0] = u[0];
          av[1] = u[1];
          av[2] = u[2];
          for (int k = 0; k < 3; ++k) av[3 + k] = u[0] * J[k][0] + u[1] * J[k][1] + u[2] * J[k][2];
          acc[0] += -K.d1 * e;
#pragma unroll
          for (int q = 0; q < 6; ++q) acc[1 + q] += w * av[q];
          if (hess) {
            // icov J_j for the angular columns (the translational ones are icov's columns)
            double IJ[3][3];
            for (int k = 0; k < 3; ++k)
              for (int a = 0; a < 3; ++a) IJ[k][a] = IC[3 * a] * J[k][0] + IC[3 * a + 1] * J[k][1] + IC[3 * a + 2] * J[k][2];
            int q = 7;
#pragma unroll
            for (int ii = 0; ii < 6; ++ii)
#pragma unroll
              for (int jj = ii; jj < 6; ++jj, ++q) {
                double jij;  // J_i^T icov J_j
                if (jj < 3) {
                  jij = IC[3 * ii + jj];
                } else if (ii < 3) {
                  jij = IJ[jj - 3][ii];
                } else {
                  jij = J[ii - 3][0] * IJ[jj - 3][0] + J[ii - 3][1] * IJ[jj - 3][1] + J[ii - 3][2] * IJ[jj - 3][2];
                }
                double uh = 0.0;  // x'^T icov d2T/dp_i dp_j
                if (ii >= 3) {
                  const int k = ii - 3, l = jj - 3;
                  const int m = k == 0 ? l : k == 1 ? 2 + l : 5;  // (0,0) (0,1) (0,2) (1,1) (1,2) (2,2)
                  const double* MH = E.MH[m];
                  for (int a = 0; a < 3; ++a) uh += u[a] * (MH[3 * a] * x[0] + MH[3 * a + 1] * x[1] + MH[3 * a + 2] * x[2]);
                }
                acc[q] += w * (-K.d2 * av[ii] * av[jj] + uh + jij);
              }
          }
        }
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < NACC; ++q) {
    double v = acc[q];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == 0) red[wv][q] = v;
  }
  __syncthreads();
  if (threadIdx.x < NACC) {
    double s = 0.0;
    for (int w = 0; w < DERIV_THREADS / 64; ++w) s += red[w][threadIdx.x];
    partials[((size_t)c * gridDim.x + blockIdx.x) * NACC + threadIdx.x] = s;
  }
}

// ---- the Newton / More-Thuente state machine (tests/ndt_ref.py::align) -----------------------------------------------
// The line search's scalar pieces are plain fp64 arithmetic, built for the host too: gloc_ndt_debug_line_search (ndt.hip)
// runs them there, and tests/test_ndt_sweep_cpu.py holds them to the restatement's bit for bit.
__host__ __device__ inline double psi_f(double a, double f_a, double f_0, double g_0, double mu) { return f_a - f_0 - mu * g_0 * a; }
__host__ __device__ inline double dpsi_f(double g_a, double g_0, double mu) { return g_a - mu * g_0; }
__host__ __device__ inline double cubic_min(double a_l, double f_l, double g_l, double a_t, double f_t, double g_t) {
  const double z = 3 * (f_t - f_l) / (a_t - a_l) - g_t - g_l;
  const double w = sqrt(z * z - g_t * g_l);
  return a_l + (a_t - a_l) * (w - g_l - z) / (g_t - g_l + 2 * w);
}
__host__ __device__ inline double trial_value(const double* I, double a_t, double f_t, double g_t) {
  const double a_l = I[0], f_l = I[1], g_l = I[2], a_u = I[3], f_u = I[4], g_u = I[5];
  if (f_t > f_l) {
    const double a_c = cubic_min(a_l, f_l, g_l, a_t, f_t, g_t);
    const double a_q = a_l - 0.5 * (a_l - a_t) * g_l / (g_l - (f_l - f_t) / (a_l - a_t));
    return fabs(a_c - a_l) < fabs(a_q - a_l) ? a_c : 0.5 * (a_q + a_c);
  }
  if (g_t * g_l < 0) {
    const double a_c = cubic_min(a_l, f_l, g_l, a_t, f_t, g_t);
    const double a_s = a_l - (a_l - a_t) / (g_l - g_t) * g_l;
    return fabs(a_c - a_t) >= fabs(a_s - a_t) ? a_c : a_s;
  }
  if (fabs(g_t) <= fabs(g_l)) {
    const double a_c = cubic_min(a_l, f_l, g_l, a_t, f_t, g_t);
    const double a_s = a_l - (a_l - a_t) / (g_l - g_t) * g_l;
    const double a_n = fabs(a_c - a_t) < fabs(a_s - a_t) ? a_c : a_s;
    const double b = a_t + 0.66 * (a_u - a_t);
    if (a_t > a_l) return (a_n < b) ? a_n : b;   // std::min(b, a_n)
    return (b < a_n) ? a_n : b;                   // std::max(b, a_n)
  }
  return cubic_min(a_u, f_u, g_u, a_t, f_t, g_t);
}
__host__ __device__ inline bool update_interval(double* I, double a_t, double f_t, double g_t) {
  if (f_t > I[1]) {
    I[3] = a_t; I[4] = f_t; I[5] = g_t;
    return false;
  }
  if (g_t * (I[0] - a_t) > 0) {
    I[0] = a_t; I[1] = f_t; I[2] = g_t;
    return false;
  }
  if (g_t * (I[0] - a_t) < 0) {
    I[3] = I[0]; I[4] = I[1]; I[5] = I[2];
    I[0] = a_t; I[1] = f_t; I[2] = g_t;
    return false;
  }
  return true;
}
__host__ __device__ inline double clamp_step(double a, double lo, double hi) {  // std::max(std::min(a, hi), lo): NaN stays NaN
  a = (hi < a) ? hi : a;
  return (a < lo) ? lo : a;
}

// the interval's values turn from psi to phi once a trial has psi <= 0 and dpsi >= 0 (open -> closed)
__host__ __device__ inline void close_interval(double* I, double phi_0, double dphi_0, double mu) {
  I[1] = I[1] + phi_0 - mu * dphi_0 * I[0];
  I[2] = I[2] + mu * dphi_0;
  I[4] = I[4] + phi_0 - mu * dphi_0 * I[3];
  I[5] = I[5] + mu * dphi_0;
}

__device__ inline void request(State& S, Eval* ev, const double* at, int phase, bool hess) {
  S.phase = phase;
  make_eval(at, ev);
  ev->hess = hess ? 1 : 0;
  ev->active = 1;
}

__device__ inline void finish(State& S, Eval* ev, Out* out, uint32_t* done_count) {
  S.phase = PH_DONE;
  ev->active = 0;
  Eval T;
  make_eval(S.p, &T);
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) out->T[4 * i + j] = (float)T.R[3 * i + j];
    out->T[4 * i + 3] = (float)T.t[i];
    out->T[12 + i] = 0.f;
  }
  out->T[15] = 1.f;
  out->prob = S.score / S.n_src;
  out->iters = (uint32_t)S.iters;
  out->converged = S.converged;
  atomicAdd(done_count, 1u);
}

// Newton steps from the current (score, g, H) until an evaluation is needed or the loop stops
__device__ inline void newton(State& S, Eval* ev, Out* out, uint32_t* done_count) {
  const double mu = 1e-4;
  while (true) {
    double A[36], V[36];
    for (int i = 0; i < 36; ++i) A[i] = S.H[i];
    jacobi_eig6(A, V);
    double smax = 0.0;
    for (int i = 0; i < 6; ++i) smax = fmax(smax, fabs(A[7 * i]));
    const double cut = fmax(6.0 * 2.220446049250313e-16 * smax, 2.2250738585072014e-308);
    double vg[6], delta[6];
    for (int k = 0; k < 6; ++k) {
      double s = 0.0;
      for (int i = 0; i < 6; ++i) s += V[6 * i + k] * (-S.g[i]);
      const double lam = A[7 * k];
      vg[k] = fabs(lam) >= cut ? s / lam : 0.0;
    }
    double dn2 = 0.0;
    for (int i = 0; i < 6; ++i) {
      double s = 0.0;
      for (int k = 0; k < 6; ++k) s += V[6 * i + k] * vg[k];
      delta[i] = s;
      dn2 += s * s;
    }
    const double dn = sqrt(dn2);
    if (dn == 0.0 || dn != dn) {
      S.converged = dn == dn;
      finish(S, ev, out, done_count);
      return;
    }
    for (int i = 0; i < 6; ++i) S.dir[i] = delta[i] / dn;
    S.phi_0 = -S.score;
    double gd = 0.0;
    for (int i = 0; i < 6; ++i) gd += S.g[i] * S.dir[i];
    S.dphi_0 = -gd;
    if (S.dphi_0 >= 0 && S.dphi_0 == 0) {  // not a descent direction and no way to flip it: a zero step
      S.a_t = 0.0;
      S.stepped = 0;
      const bool stop = S.iters > S.max_iters || (S.iters && fabs(S.a_t) < S.eps);
      if (stop) {
        S.converged = S.iters && fabs(S.a_t) < S.eps;
        S.iters++;
        finish(S, ev, out, done_count);
        return;
      }
      S.iters++;
      continue;
    }
    if (S.dphi_0 > 0) {
      S.dphi_0 = -S.dphi_0;
      for (int i = 0; i < 6; ++i) S.dir[i] = -S.dir[i];
    }
    S.stepped = 1;
    const double f0 = psi_f(0.0, S.phi_0, S.phi_0, S.dphi_0, mu), g0 = dpsi_f(S.dphi_0, S.dphi_0, mu);
    S.I[0] = 0.0; S.I[1] = f0; S.I[2] = g0;
    S.I[3] = 0.0; S.I[4] = f0; S.I[5] = g0;
    S.interval_converged = 0;
    S.open_interval = 1;
    S.step_iters = 0;
    S.a_t = clamp_step(dn, S.step_min, S.step_max);
    for (int i = 0; i < 6; ++i) S.x_t[i] = S.p[i] + S.dir[i] * S.a_t;
    request(S, ev, S.x_t, PH_FIRST, true);
    return;
  }
}

// p <- x_t; the stop test; the next Newton step
__device__ inline void finish_step(State& S, Eval* ev, Out* out, uint32_t* done_count) {
  if (S.stepped)
    for (int i = 0; i < 6; ++i) S.p[i] = S.p[i] + S.dir[i] * S.a_t;
  const bool stop = S.iters > S.max_iters || (S.iters && fabs(S.a_t) < S.eps);
  if (stop) {
    S.converged = S.iters && fabs(S.a_t) < S.eps;
    S.iters++;
    finish(S, ev, out, done_count);
    return;
  }
  S.iters++;
  newton(S, ev, out, done_count);
}

__device__ inline void after_trial(State& S, Eval* ev, Out* out, uint32_t* done_count, bool first) {
  const double mu = 1e-4, nu = 0.9;
  double gd = 0.0;
  for (int i = 0; i < 6; ++i) gd += S.g[i] * S.dir[i];
  const double phi_t = -S.score, dphi_t = -gd;
  const double psi_t = psi_f(S.a_t, phi_t, S.phi_0, S.dphi_0, mu), dpsi_t = dpsi_f(dphi_t, S.dphi_0, mu);
  if (!first) {
    if (S.open_interval && (psi_t <= 0 && dpsi_t >= 0)) {
      S.open_interval = 0;
      close_interval(S.I, S.phi_0, S.dphi_0, mu);
    }
    S.interval_converged = S.open_interval ? update_interval(S.I, S.a_t, psi_t, dpsi_t)
                                           : update_interval(S.I, S.a_t, phi_t, dphi_t);
    S.step_iters++;
  }
  if (!S.interval_converged && S.step_iters < 10 && !(psi_t <= 0 && dphi_t <= -nu * S.dphi_0)) {
    const double a = S.open_interval ? trial_value(S.I, S.a_t, psi_t, dpsi_t) : trial_value(S.I, S.a_t, phi_t, dphi_t);
    S.a_t = clamp_step(a, S.step_min, S.step_max);
    for (int i = 0; i < 6; ++i) S.x_t[i] = S.p[i] + S.dir[i] * S.a_t;
    request(S, ev, S.x_t, PH_MORE, false);
    return;
  }
  if (S.step_iters) {
    request(S, ev, S.x_t, PH_HESS, true);
    return;
  }
  finish_step(S, ev, out, done_count);
}

// one wave per candidate: sum the work-groups' partials in block order, then step the state.  export_sums: only write
// the sums (gloc_reg_ndt_derivatives)
static __global__ __launch_bounds__(64) void ndt_state_kernel(const double* __restrict__ partials, uint32_t n_blk, State* __restrict__ states,
                                                       Eval* __restrict__ evals, Out* __restrict__ outs, uint32_t* __restrict__ done_count,
                                                       double* __restrict__ export_sums) {
  const uint32_t c = blockIdx.x;
  __shared__ double sums[NACC];
  if (!evals[c].active) return;
  const int l = threadIdx.x;
  if (l < NACC) {
    double s = 0.0;
    for (uint32_t b = 0; b < n_blk; ++b) s += partials[((size_t)c * n_blk + b) * NACC + l];
    sums[l] = s;
  }
  __syncthreads();
  if (l != 0) return;
  double H[36];
  {
    int q = 7;
    for (int i = 0; i < 6; ++i)
      for (int j = i; j < 6; ++j, ++q) {
        H[6 * i + j] = sums[q];
        H[6 * j + i] = sums[q];
      }
  }
  if (export_sums) {
    for (int q = 0; q < 7; ++q) export_sums[(size_t)c * 43 + q] = sums[q];
    for (int q = 0; q < 36; ++q) export_sums[(size_t)c * 43 + 7 + q] = H[q];
    evals[c].active = 0;
    return;
  }
  State S = states[c];
  Eval* ev = &evals[c];
  Out* out = &outs[c];
  const int ph = S.phase;
  if (ph == PH_HESS) {
    for (int i = 0; i < 36; ++i) S.H[i] = H[i];
    finish_step(S, ev, out, done_count);
  } else {
    S.score = sums[0];
    for (int i = 0; i < 6; ++i) S.g[i] = sums[1 + i];
    if (ph != PH_MORE)
      for (int i = 0; i < 36; ++i) S.H[i] = H[i];
    if (ph == PH_INIT)
      newton(S, ev, out, done_count);
    else
      after_trial(S, ev, out, done_count, ph == PH_FIRST);
  }
  states[c] = S;
}

// initial state of every candidate: p0 from its guess (Eigen's eulerAngles(0, 1, 2), fp64), an evaluation at p0 with the
// Hessian.  init_T: [n][16] row-major floats or null (identity); p6: a fixed p for every candidate instead (derivatives)
static __global__ void ndt_init_kernel(uint32_t n, const float* __restrict__ init_T, const double* __restrict__ p6, const int* __restrict__ cand_tgt,
                                double n_src, double step_max, double step_min, double eps, int max_iters,
                                State* __restrict__ states, Eval* __restrict__ evals) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  State S;
  memset(&S, 0, sizeof(S));
  if (p6) {
    for (int i = 0; i < 6; ++i) S.p[i] = p6[i];
  } else {
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if (init_T) {
      const float* T = init_T + 16 * (size_t)c;
      for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) R[3 * i + j] = (double)T[4 * i + j];
        S.p[i] = (double)T[4 * i + 3];
      }
    }
    euler_xyz(R, S.p + 3);
  }
  S.tgt = cand_tgt[c];
  S.n_src = n_src;
  S.step_max = step_max;
  S.step_min = step_min;
  S.eps = eps;
  S.max_iters = max_iters;
  request(S, &evals[c], S.p, PH_INIT, true);
  states[c] = S;
}

}  // namespace ndt
}  // namespace gloc
