// p2l_kernels.hpp -- device kernels of the point-to-plane ICP refinement (gfx950).  tests/p2l_ref.py is the contract.
//
//   p2l_accum_kernel   one lane per source point (sorted slot): p = R s + t in fp32 as the search moved it, the matched
//                      target point and its normal, r = n.(p - q), J = [p x n ; n]; the 29 sums of a pass (21 entries of
//                      the upper triangle of J J^T, 6 of J r, r^2, the count) in fp64, one partial per work-group
//   p2l_solve_kernel   one wave per job: the partials summed in index order, 6 x 6 Cholesky, Rodrigues, T <- T_k T,
//                      the stop test and the freeze flag -- all fp64
//
// The correspondences are the registration's own exact 1-NN pass (reg.hip: launch_nn), unchanged.
//
// Registers: a lane has ONE point, so its 29 fp64 values are products, not loop-carried accumulators; they are live only
// through a reduce-scatter (lane_ops.hpp) that halves them at every step -- 32 -> 16 -> 8 -> 4 -> 2 -> 1 values, 32 exchanges
// of a double in all instead of 29 x 6 -- and the kernel stays far below the 128 registers that would cost occupancy.
// No floating-point atomics anywhere: a partial's slot is (job, work-group), the solve adds the slots in index order, so
// a job's sums do not depend on the batch it runs in.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lane_ops.hpp"
#include "math3.hpp"  // f32x4, xform

namespace gloc {
namespace p2l {

using reg::f32x4;

constexpr int ACC_THREADS = 256;  // source points per work-group
constexpr int NSUM = 29;          // H upper triangle 21 (row-major), g 6, sum r^2, count
constexpr int NSLOT = 32;         // a partial's row (256 B)

struct Target {  // of a job
  const f32x4* pts;  // the search order: x, y, z, bits(original index)
  const float* nrm;  // normals in that order, packed
  uint32_t n, pad_;
};

// per-job state beside the fp32 pose the search reads
struct State {
  double Td[12];  // R row-major 9, t 3: source -> target
  double sum_r2;  // of the last evaluation
  double rmse;
  uint64_t count;
  uint32_t iters;
  int status;   // 0 iteration cap, 1 converged, 2 degenerate
  int stopped;  // frozen: later passes leave the job alone
  int pad_;
};

// keep the half of v[0 .. 2H) this lane owns at the step that exchanges with lane ^ O, add the partner's share of it
template <int O, int H>
__device__ __forceinline__ void scatter_step(double* v, bool up) {
#pragma unroll
  for (int k = 0; k < H; ++k) {
    const double keep = up ? v[k + H] : v[k], send = up ? v[k] : v[k + H];
    v[k] = keep + xor_lane<O>(send);
  }
}

__global__ __launch_bounds__(ACC_THREADS) void p2l_accum_kernel(const f32x4* __restrict__ src_pts, uint32_t n_src,
                                                                const Target* __restrict__ tgts, const float* __restrict__ pose_f32,
                                                                size_t pose_stride /* floats */, const State* __restrict__ states,
                                                                const uint32_t* __restrict__ corr, const float* __restrict__ d2in, size_t ld,
                                                                float gate2, bool skip_stopped, double* __restrict__ partials /* [job][n_blk][NSLOT] */) {
  __shared__ double red[ACC_THREADS / 64][NSLOT];
  const uint32_t job = blockIdx.y;
  if (skip_stopped && states[job].stopped) return;  // (uniform; the solve does not read a stopped job's partials)
  const uint32_t i = blockIdx.x * ACC_THREADS + threadIdx.x;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  double v[NSLOT];
#pragma unroll
  for (int k = 0; k < NSLOT; ++k) v[k] = 0.0;
  if (i < n_src) {
    const Target T = tgts[job];
    const uint32_t j = corr[(size_t)job * ld + i];
    const float d2 = d2in[(size_t)job * ld + i];
    // (d2 - d2 == 0: finite)
    if (j < T.n && d2 - d2 == 0.f && (!(gate2 > 0.f) || d2 <= gate2)) {
      const float nx = T.nrm[3 * (size_t)j], ny = T.nrm[3 * (size_t)j + 1], nz = T.nrm[3 * (size_t)j + 2];
      if (nx != 0.f || ny != 0.f || nz != 0.f) {
        float Tf[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) Tf[k] = pose_f32[(size_t)job * pose_stride + k];
        const f32x4 s = src_pts[i];
        const f32x4 q = T.pts[j];
        float px, py, pz;
        reg::xform(Tf, s.x, s.y, s.z, px, py, pz);
        const double P[3] = {(double)px, (double)py, (double)pz};
        const double N[3] = {(double)nx, (double)ny, (double)nz};
        const double r = (N[0] * (P[0] - (double)q.x) + N[1] * (P[1] - (double)q.y)) + N[2] * (P[2] - (double)q.z);
        double J[6];
        reg::cross3(P, N, J);
        J[3] = N[0]; J[4] = N[1]; J[5] = N[2];
        int e = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
          for (int b = a; b < 6; ++b) v[e++] = J[a] * J[b];
#pragma unroll
        for (int a = 0; a < 6; ++a) v[21 + a] = J[a] * r;
        v[27] = r * r;
        v[28] = 1.0;
      }
    }
  }
  // reduce-scatter over the wave: lane l ends with the wave's sum of value l >> 1
  scatter_step<32, 16>(v, (lane & 32) != 0);
  scatter_step<16, 8>(v, (lane & 16) != 0);
  scatter_step<8, 4>(v, (lane & 8) != 0);
  scatter_step<4, 2>(v, (lane & 4) != 0);
  scatter_step<2, 1>(v, (lane & 2) != 0);
  const double x = v[0] + xor_lane<1>(v[0]);
  if ((lane & 1) == 0) red[w][lane >> 1] = x;
  __syncthreads();
  if (threadIdx.x < NSLOT) {
    double s = 0.0;
#pragma unroll
    for (int ww = 0; ww < ACC_THREADS / 64; ++ww) s += red[ww][threadIdx.x];
    partials[((size_t)job * gridDim.x + blockIdx.x) * NSLOT + threadIdx.x] = s;
  }
}

// mode 0: a pass (solve, update, stop test).  mode 1: evaluation only (sum_r2, count, rmse; `exp`, if given, gets the
// job's 29 sums).
__global__ __launch_bounds__(64) void p2l_solve_kernel(const double* __restrict__ partials, uint32_t n_blk, State* __restrict__ states,
                                                       float* __restrict__ pose_f32, size_t pose_stride, double trans_eps, double rot_eps,
                                                       int mode, uint32_t* __restrict__ done, double* __restrict__ exp) {
  __shared__ double tot[NSLOT];
  const uint32_t job = blockIdx.x;
  State& st = states[job];
  if (mode == 0 && st.stopped) return;
  const int lane = threadIdx.x;
  if (lane < NSLOT) {
    const double* p = partials + (size_t)job * n_blk * NSLOT + lane;
    double s = 0.0;
    for (uint32_t b = 0; b < n_blk; ++b) s += p[(size_t)b * NSLOT];
    tot[lane] = s;
    if (exp && lane < NSUM) exp[(size_t)job * NSUM + lane] = s;
  }
  __syncthreads();
  if (lane != 0) return;
  const double cnt = tot[28];
  st.sum_r2 = tot[27];
  st.count = (uint64_t)cnt;
  st.rmse = cnt > 0.0 ? sqrt(tot[27] / cnt) : 0.0;
  if (mode != 0) return;
  auto stop = [&](int status) {
    st.status = status;
    st.stopped = 1;
    atomicAdd(done, 1u);
  };
  double L[6][6];
  double dmax = 0.0;
  {
    int e = 0;
    for (int a = 0; a < 6; ++a)
      for (int b = a; b < 6; ++b) {
        L[a][b] = tot[e];
        L[b][a] = tot[e];
        ++e;
      }
    for (int a = 0; a < 6; ++a) dmax = L[a][a] > dmax ? L[a][a] : dmax;
  }
  bool ok = cnt >= 6.0;
  // Cholesky, row by row (lower triangle in place): a pivot at or below 1e-12 of the largest diagonal entry is degenerate
  for (int jj = 0; jj < 6 && ok; ++jj) {
    double d = L[jj][jj];
    for (int k = 0; k < jj; ++k) d -= L[jj][k] * L[jj][k];
    if (!(d > 1e-12 * dmax)) {
      ok = false;
      break;
    }
    const double dj = sqrt(d);
    L[jj][jj] = dj;
    for (int i = jj + 1; i < 6; ++i) {
      double s = L[i][jj];
      for (int k = 0; k < jj; ++k) s -= L[i][k] * L[jj][k];
      L[i][jj] = s / dj;
    }
  }
  if (!ok) {
    stop(2);
    return;
  }
  double y[6], xi[6];
  for (int i = 0; i < 6; ++i) {
    double s = -tot[21 + i];
    for (int k = 0; k < i; ++k) s -= L[i][k] * y[k];
    y[i] = s / L[i][i];
  }
  for (int i = 5; i >= 0; --i) {
    double s = y[i];
    for (int k = i + 1; k < 6; ++k) s -= L[k][i] * xi[k];
    xi[i] = s / L[i][i];
  }
  // Rodrigues: R = I + (sin th / th) K + ((1 - cos th) / th^2) K^2, K = [w]x
  const double wx = xi[0], wy = xi[1], wz = xi[2];
  const double th2 = (wx * wx + wy * wy) + wz * wz, th = sqrt(th2);
  double A = 1.0, B = 0.5;
  if (th > 0.0) {
    A = sin(th) / th;
    const double sh = sin(0.5 * th);
    B = 2.0 * (sh * sh) / th2;  // (1 - cos th) / th^2 without the cancellation
  }
  const double K[9] = {0.0, -wz, wy, wz, 0.0, -wx, -wy, wx, 0.0};
  double Rk[9];
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) {
      const double k2 = (K[3 * a + 0] * K[0 + b] + K[3 * a + 1] * K[3 + b]) + K[3 * a + 2] * K[6 + b];
      Rk[3 * a + b] = ((a == b ? 1.0 : 0.0) + A * K[3 * a + b]) + B * k2;
    }
  double Tn[12];
  for (int a = 0; a < 3; ++a) {
    for (int b = 0; b < 3; ++b) Tn[3 * a + b] = (Rk[3 * a + 0] * st.Td[0 + b] + Rk[3 * a + 1] * st.Td[3 + b]) + Rk[3 * a + 2] * st.Td[6 + b];
    Tn[9 + a] = ((Rk[3 * a + 0] * st.Td[9] + Rk[3 * a + 1] * st.Td[10]) + Rk[3 * a + 2] * st.Td[11]) + xi[3 + a];
  }
  for (int k = 0; k < 12; ++k) {
    st.Td[k] = Tn[k];
    pose_f32[(size_t)job * pose_stride + k] = (float)Tn[k];
  }
  st.iters += 1;
  const double vn = sqrt((xi[3] * xi[3] + xi[4] * xi[4]) + xi[5] * xi[5]);
  if (trans_eps > 0.0 && rot_eps > 0.0 && vn < trans_eps && th < rot_eps) stop(1);
}

}  // namespace p2l
}  // namespace gloc
