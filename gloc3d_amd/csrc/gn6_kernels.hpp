// gn6_kernels.hpp -- what the Gauss-Newton refinements on 6 pose parameters share on the device (gfx950): point-to-plane
// (p2l_kernels.hpp), generalized ICP (gicp_kernels.hpp) and its voxelized form (vgicp_kernels.hpp).  Each has its own
// accumulate kernel -- one lane per source point, the pair's 29 fp64 contributions, a 30th (the robust weight: robust.hpp)
// from the robust instantiations -- and ends it with reduce_store() here; solve_kernel here takes it from there.
//
//   reduce_store    the 29 sums of a pass (21 entries of the upper triangle of H, 6 of g, the squared residual, the count):
//                   a reduce-scatter over the wave, the work-group's waves in LDS, one partial per work-group
//   chol_rodrigues  the update itself, fp64: 6 x 6 Cholesky with the pivot rule, xi = -H^-1 g, Rodrigues, exp(xi) T (also
//                   what the one-launch GNC of fgr_kernels.hpp runs once per update)
//   solve_kernel    one wave per job: the partials summed in index order, chol_rodrigues, T <- T_k T,
//                   the stop test and the freeze flag -- all fp64
//
// Registers: a lane has ONE point, so its 29 fp64 values are products, not loop-carried accumulators; they are live only
// through a reduce-scatter (lane_ops.hpp) that halves them at every step -- 32 -> 16 -> 8 -> 4 -> 2 -> 1 values, 32 exchanges
// of a double in all instead of 29 x 6 -- and the kernels stay far below the 128 registers that would cost occupancy.
// No floating-point atomics anywhere: a partial's slot is (job, work-group), the solve adds the slots in index order, so
// a job's sums do not depend on the batch it runs in.
//
// Sources: every job has its own (Source) -- one scan repeated by the single-source entries, a scan per row by the pair
// lists.  A job of n source slots is cut into ceil(n / ACC_THREADS) work-groups of consecutive slots whatever batch it is
// in, and its partials are that many consecutive rows from row0 (a prefix sum of the counts): the solve adds exactly the
// rows a call on the job alone adds, in the same order.  The accumulate grid is (the batch's largest count, jobs); a
// work-group at or beyond its job's own count leaves at once.
//
// The kernel is static: p2l.hip and gicp.hip each carry their copy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lane_ops.hpp"
#include "math3.hpp"  // f32x4
#include "p2l.hpp"    // gn6::Target: declared where reg.hip, which fills the table, sees it
#include "robust.hpp"

namespace gloc {
namespace gn6 {

constexpr int ACC_THREADS = 256;  // source points per work-group
constexpr int NSUM = 29;          // H upper triangle 21 (row-major), g 6, the squared residual, count
constexpr int NSLOT = 32;         // a partial's row (256 B)
constexpr int WSLOT = 29;         // ... whose slot behind the sums holds the robust weights' sum (0 from a plain kernel)

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
  double wsum;  // of the last evaluation: the robust weights' sum (0 from a plain kernel)
};

// A job's source as the accumulate kernels take it, and where its partials are.
struct Source {
  const reg::f32x4* pts;  // the search order: x, y, z, bits(original index)
  const float* nrm;       // normals in that order, packed; zero = none (null for point-to-plane, which reads none)
  uint32_t n;
  uint32_t n_blk;         // work-groups of ACC_THREADS slots: ceil(n / ACC_THREADS); 0: a job without a target
  uint64_t row0;          // the job's first row of the partials: the sum of n_blk over the jobs before it
};
static_assert(sizeof(Source) == 32, "two to a 64-byte line");

// The scale of a robust accumulate kernel's pass, squared: the table's entry at the job's update index (the last entry
// from there on), or `fixed` without a table -- the evaluation after the loop and the system form.
struct Scale2 {
  const double* tab;
  uint32_t n_tab;
  double fixed;
};
__device__ __forceinline__ double scale2_of(const Scale2& s, const State& st) {
  if (!s.tab) return s.fixed;
  const uint32_t k = st.iters < s.n_tab - 1 ? st.iters : s.n_tab - 1;
  return s.tab[k];
}

// keep the half of v[0 .. 2H) this lane owns at the step that exchanges with lane ^ O, add the partner's share of it
template <int O, int H>
__device__ __forceinline__ void scatter_step(double* v, bool up) {
#pragma unroll
  for (int k = 0; k < H; ++k) {
    const double keep = up ? v[k + H] : v[k], send = up ? v[k] : v[k + H];
    v[k] = keep + xor_lane<O>(send);
  }
}

// The tail of an accumulate kernel of ACC_THREADS lanes, reached by every lane (v zero where there is no pair): `row` is
// the work-group's NSLOT doubles.
__device__ __forceinline__ void reduce_store(double* v, double (*red)[NSLOT] /* LDS [ACC_THREADS / 64] */, double* __restrict__ row) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
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
    row[threadIdx.x] = s;
  }
}

// The update of a pose from a 6 x 6 system, as both the refinements' solve_kernel below and the one-launch GNC of the Fast
// Global Registration (fgr_kernels.hpp) run it: tot is H's upper triangle (21, row-major) and g (6); Cholesky row by row
// with the pivot rule, xi = -H^-1 g (rotation first), Rodrigues, Tn = exp(xi) Td.  false: a degenerate system (Tn, xi and
// th_out are then not written).  th_out: |xi's rotation part|.
__device__ inline bool chol_rodrigues(const double* tot /* [27] */, const double* Td /* [12] */, double* Tn /* [12] */, double* xi /* [6] */,
                                      double* th_out) {
  double L[6][6];
  double dmax = 0.0;
  {
    int e = 0;
    #pragma unroll
    for (int a = 0; a < 6; ++a)
      #pragma unroll
      for (int b = a; b < 6; ++b) {
        L[a][b] = tot[e];
        L[b][a] = tot[e];
        ++e;
      }
    #pragma unroll
    for (int a = 0; a < 6; ++a) dmax = L[a][a] > dmax ? L[a][a] : dmax;
  }
  bool ok = true;
  // Cholesky, row by row (lower triangle in place): a pivot at or below 1e-12 of the largest diagonal entry is degenerate
  #pragma unroll
  for (int jj = 0; jj < 6 && ok; ++jj) {
    double d = L[jj][jj];
    #pragma unroll
    for (int k = 0; k < jj; ++k) d -= L[jj][k] * L[jj][k];
    if (!(d > 1e-12 * dmax)) {
      ok = false;
      break;
    }
    const double dj = sqrt(d);
    L[jj][jj] = dj;
    #pragma unroll
    for (int i = jj + 1; i < 6; ++i) {
      double s = L[i][jj];
      #pragma unroll
      for (int k = 0; k < jj; ++k) s -= L[i][k] * L[jj][k];
      L[i][jj] = s / dj;
    }
  }
  if (!ok) return false;
  double y[6];
  #pragma unroll
  for (int i = 0; i < 6; ++i) {
    double s = -tot[21 + i];
    #pragma unroll
    for (int k = 0; k < i; ++k) s -= L[i][k] * y[k];
    y[i] = s / L[i][i];
  }
  #pragma unroll
  for (int i = 5; i >= 0; --i) {
    double s = y[i];
    #pragma unroll
    for (int k = i + 1; k < 6; ++k) s -= L[k][i] * xi[k];
    xi[i] = s / L[i][i];
  }
  // Rodrigues: R = I + (sin th / th) K + ((1 - cos th) / th^2) K^2, K = [w]x
  const double wx = xi[0], wy = xi[1], wz = xi[2];
  const double th2 = (wx * wx + wy * wy) + wz * wz, th = sqrt(th2);
  *th_out = th;
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
  for (int a = 0; a < 3; ++a) {
    for (int b = 0; b < 3; ++b) Tn[3 * a + b] = (Rk[3 * a + 0] * Td[0 + b] + Rk[3 * a + 1] * Td[3 + b]) + Rk[3 * a + 2] * Td[6 + b];
    Tn[9 + a] = ((Rk[3 * a + 0] * Td[9] + Rk[3 * a + 1] * Td[10]) + Rk[3 * a + 2] * Td[11]) + xi[3 + a];
  }
  return true;
}

// mode 0: a pass (solve, update, stop test).  mode 1: evaluation only (sum_r2, count, rmse, wsum; `exp`, if given, gets
// the job's 29 sums).  stop_from: the first update index at which the stop test counts (0: every update; a robust
// schedule's first index at its final scale).
static __global__ __launch_bounds__(64) void solve_kernel(const double* __restrict__ partials /* [sum of n_blk][NSLOT] */,
                                                          const Source* __restrict__ srcs, uint32_t stop_from,
                                                          State* __restrict__ states,
                                                          float* __restrict__ pose_f32, size_t pose_stride, double trans_eps, double rot_eps,
                                                          int mode, uint32_t* __restrict__ done, double* __restrict__ exp) {
  __shared__ double tot[NSLOT];
  const uint32_t job = blockIdx.x;
  State& st = states[job];
  if (mode == 0 && st.stopped) return;
  const int lane = threadIdx.x;
  if (lane < NSLOT) {
    const uint32_t n_blk = srcs[job].n_blk;
    const double* p = partials + (size_t)srcs[job].row0 * NSLOT + lane;
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
  st.wsum = tot[WSLOT];
  if (mode != 0) return;
  auto stop = [&](int status) {
    st.status = status;
    st.stopped = 1;
    atomicAdd(done, 1u);
  };
  double Tn[12], xi[6], th;
  if (!(cnt >= 6.0) || !chol_rodrigues(tot, st.Td, Tn, xi, &th)) {
    stop(2);
    return;
  }
  for (int k = 0; k < 12; ++k) {
    st.Td[k] = Tn[k];
    pose_f32[(size_t)job * pose_stride + k] = (float)Tn[k];
  }
  const uint32_t k = st.iters;
  st.iters = k + 1;
  const double vn = sqrt((xi[3] * xi[3] + xi[4] * xi[4]) + xi[5] * xi[5]);
  if (trans_eps > 0.0 && rot_eps > 0.0 && vn < trans_eps && th < rot_eps && k >= stop_from) stop(1);
}

}  // namespace gn6
}  // namespace gloc
