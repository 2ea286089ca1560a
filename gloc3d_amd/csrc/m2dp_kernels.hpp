// m2dp_kernels.hpp -- device side of the M2DP place descriptor (gloc_m2dp_* of include/gloc3d.h; m2dp.hip is the host
// side).  Everything is batched over scans through a per-scan table (blockIdx.y = scan).  Three stages:
//   frame:   moments_kernel<S> / combine_kernel<S>, S = 0, 1, 2: the used points' sum; their central second moments and
//            max |p - c|^2; their central third moments along e1 and e2.  A block reduces one slice of SLICE points in a
//            fixed tree, a block per scan adds the slices' partials in a fixed tree, and its first lane closes the
//            stage: the mean; the Jacobi and the sorted eigenvectors; the signs, e3 and the frame.
//   project: project_kernel   lane = plane; a wave walks its points (each wave-uniform, four a step) and lane j counts the
//            point into its own 16-bit LDS counter of the bin -- no atomics on the way, integer atomics for the block's
//            sums at the end
//   svd:     svd_kernel       a work-group per signature: power iteration on A A^T in fp64, deflated once for sigma2
// Determinism: no floating-point atomics.  A scan's slices, and the order they are added in, depend on the scan's own
// length alone, so a scan in a batch gives the bits it gives alone; the counts are integer sums.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "math3.hpp"  // jacobi_eig3, cross3

namespace gloc {
namespace m2dp {

constexpr int MAX_PLANES = 64, MAX_BINS = 128;
constexpr int SLICE = 2048;      // points a block of moments_kernel reduces
constexpr int PART_W = 7;        // doubles per slice partial (the widest stage: 6 second moments and the maximum)
constexpr int PROJ_WAVES = 2;    // waves per block of project_kernel, a 16 KiB histogram copy each
constexpr uint32_t MAX_CHUNK = 8192;  // points per block of project_kernel: 4096 per wave, so a 16-bit counter never wraps
constexpr int SVD_ITERS = 20000, SVD2_ITERS = 2048;

struct ScanRef {
  const float* xyz;
  uint32_t n, stride;
};

// What the frame stage leaves per scan.  n_used = 0: no descriptor (R = identity, c = 0).
struct Info {
  double R[9];    // row-major, columns e1 e2 e3 (after stage 1: e1 and e2 unsigned, in columns 0 and 1)
  double c[3];
  double inv_r2;  // 1 / max |p - c|^2 (inf when all points are equal)
  uint32_t n_used, pad_;
};

// Made on the host in fp64 (m2dp.hip).
struct Tables {
  double u[MAX_PLANES][3], v[MAX_PLANES][3];  // the in-plane unit pair of every plane
  double ring_thr[MAX_BINS];                  // (k / l)^4: ring >= k iff (rho / r)^2 >= ring_thr[k]
  double sec_cos[MAX_BINS], sec_sin[MAX_BINS];  // of the sector borders 2 pi k / t
};

// M1: finite, and inside max_range by the un-fused fp32 test of the contract
__device__ __forceinline__ bool used_point(float x, float y, float z, float max_range2) {
  return isfinite(x) && isfinite(y) && isfinite(z) && ((x * x + y * y) + z * z < max_range2);
}

// the block's 256 values of each of W sums -> thread 0's acc[]; slot IS_MAX (or none) is a maximum.  A fixed tree.
template <int W, int IS_MAX>
__device__ __forceinline__ void block_reduce(double (&acc)[W], double* lds /* [W][256] */) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int w = 0; w < W; ++w) lds[w * 256 + tid] = acc[w];
  for (int s = 128; s >= 1; s >>= 1) {
    __syncthreads();
    if (tid < s) {
#pragma unroll
      for (int w = 0; w < W; ++w) {
        const double a = lds[w * 256 + tid], b = lds[w * 256 + tid + s];
        lds[w * 256 + tid] = (w == IS_MAX) ? fmax(a, b) : a + b;
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int w = 0; w < W; ++w) acc[w] = lds[w * 256];
}

template <int STAGE>
struct StageW {
  static constexpr int W = STAGE == 0 ? 4 : STAGE == 1 ? 7 : 2;
  static constexpr int IS_MAX = STAGE == 1 ? 6 : -1;
};

// part [n_scans][nb_max][PART_W]: slice b of a scan is its points [b * SLICE, (b + 1) * SLICE)
template <int STAGE>
__global__ __launch_bounds__(256) void moments_kernel(const ScanRef* __restrict__ scans, float max_range2,
                                                      const Info* __restrict__ info, double* __restrict__ part,
                                                      uint32_t nb_max) {
  constexpr int W = StageW<STAGE>::W;
  __shared__ double lds[W * 256];
  const ScanRef sc = scans[blockIdx.y];
  const size_t first = (size_t)blockIdx.x * SLICE;
  if (first >= sc.n) return;
  double c[3] = {0, 0, 0}, e1[3] = {0, 0, 0}, e2[3] = {0, 0, 0};
  if (STAGE > 0) {
    const Info& in = info[blockIdx.y];
    if (in.n_used == 0) return;
    for (int k = 0; k < 3; ++k) c[k] = in.c[k], e1[k] = in.R[3 * k], e2[k] = in.R[3 * k + 1];
  }
  double acc[W];
#pragma unroll
  for (int w = 0; w < W; ++w) acc[w] = 0.0;
  for (int k = 0; k < SLICE / 256; ++k) {
    const size_t i = first + (size_t)k * 256 + threadIdx.x;
    if (i >= sc.n) break;
    const float* p = sc.xyz + i * sc.stride;
    const float x = p[0], y = p[1], z = p[2];
    if (!used_point(x, y, z, max_range2)) continue;
    if (STAGE == 0) {
      acc[0] += (double)x, acc[1] += (double)y, acc[2] += (double)z, acc[3] += 1.0;
    } else {
      const double dx = (double)x - c[0], dy = (double)y - c[1], dz = (double)z - c[2];
      if (STAGE == 1) {
        acc[0] += dx * dx, acc[1] += dx * dy, acc[2] += dx * dz;
        acc[3] += dy * dy, acc[4] += dy * dz, acc[5] += dz * dz;
        acc[6] = fmax(acc[6], (dx * dx + dy * dy) + dz * dz);
      } else {
        const double a = (dx * e1[0] + dy * e1[1]) + dz * e1[2], b = (dx * e2[0] + dy * e2[1]) + dz * e2[2];
        acc[0] += a * a * a, acc[1] += b * b * b;
      }
    }
  }
  block_reduce<W, StageW<STAGE>::IS_MAX>(acc, lds);
  if (threadIdx.x == 0) {
    double* o = part + ((size_t)blockIdx.y * nb_max + blockIdx.x) * PART_W;
#pragma unroll
    for (int w = 0; w < W; ++w) o[w] = acc[w];
  }
}

// One block per scan: the slices' partials in a fixed tree, then lane 0 closes the stage.
//   frames [n_scans][12] (R row-major, c) and n_used [n_scans] are written by stage 2.
template <int STAGE>
__global__ __launch_bounds__(256) void combine_kernel(const ScanRef* __restrict__ scans, const double* __restrict__ part,
                                                      uint32_t nb_max, uint32_t min_points, Info* __restrict__ info,
                                                      double* __restrict__ frames, uint32_t* __restrict__ n_used) {
  constexpr int W = StageW<STAGE>::W;
  __shared__ double lds[W * 256];
  const uint32_t scan = blockIdx.x;
  Info& in = info[scan];
  const bool none = STAGE > 0 && in.n_used == 0;
  double acc[W];
#pragma unroll
  for (int w = 0; w < W; ++w) acc[w] = 0.0;
  if (!none) {
    const uint32_t nb = (scans[scan].n + SLICE - 1) / SLICE;
    for (uint32_t b = threadIdx.x; b < nb; b += 256) {
      const double* s = part + ((size_t)scan * nb_max + b) * PART_W;
#pragma unroll
      for (int w = 0; w < W; ++w) acc[w] = (w == StageW<STAGE>::IS_MAX) ? fmax(acc[w], s[w]) : acc[w] + s[w];
    }
    block_reduce<W, StageW<STAGE>::IS_MAX>(acc, lds);
  }
  if (threadIdx.x != 0) return;
  if (STAGE == 0) {
    const bool ok = acc[3] >= (double)min_points;
    in.n_used = ok ? (uint32_t)acc[3] : 0u;
    for (int k = 0; k < 9; ++k) in.R[k] = (k % 4 == 0) ? 1.0 : 0.0;
    for (int k = 0; k < 3; ++k) in.c[k] = ok ? acc[k] / acc[3] : 0.0;
    in.inv_r2 = 0.0;
  } else if (STAGE == 1) {
    if (none) return;
    const double n = (double)in.n_used;
    double A[9] = {acc[0] / n, acc[1] / n, acc[2] / n, acc[1] / n, acc[3] / n, acc[4] / n, acc[2] / n, acc[4] / n, acc[5] / n};
    double V[9];
    reg::jacobi_eig3(A, V);
    int o[3] = {0, 1, 2};  // l1 >= l2 >= l3, ties to the lower column: a stable insertion sort
    for (int i = 1; i < 3; ++i)
      for (int j = i; j > 0 && A[4 * o[j]] > A[4 * o[j - 1]]; --j) {
        const int t = o[j];
        o[j] = o[j - 1], o[j - 1] = t;
      }
    for (int k = 0; k < 3; ++k) in.R[3 * k] = V[3 * k + o[0]], in.R[3 * k + 1] = V[3 * k + o[1]];
    in.inv_r2 = 1.0 / acc[6];
  } else {
    if (!none) {
      double e1[3], e2[3], e3[3];
      for (int k = 0; k < 3; ++k) {
        e1[k] = acc[0] < 0.0 ? -in.R[3 * k] : in.R[3 * k];
        e2[k] = acc[1] < 0.0 ? -in.R[3 * k + 1] : in.R[3 * k + 1];
      }
      reg::cross3(e1, e2, e3);
      for (int k = 0; k < 3; ++k) in.R[3 * k] = e1[k], in.R[3 * k + 1] = e2[k], in.R[3 * k + 2] = e3[k];
    }
    for (int k = 0; k < 9; ++k) frames[(size_t)scan * 12 + k] = in.R[k];
    for (int k = 0; k < 3; ++k) frames[(size_t)scan * 12 + 9 + k] = in.c[k];
    n_used[scan] = in.n_used;
  }
}

__device__ __forceinline__ double readlane_f64(double v, int lane) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}

// Block (x, scan): the points [x * chunk, (x + 1) * chunk) of the scan, chunk <= MAX_CHUNK.  counts [n_scans][P][B],
// zeroed by the caller.  The 64 lanes of a wave load 64 points and bring them into the frame (fp64); then the wave takes
// the used ones PTS at a time -- a point is wave-uniform (v_readlane) -- and lane j, which holds plane j's unit pair,
// finds the bin and adds one to ITS counter of that bin.  Counter (bin, lane) is the 16-bit half (lane >> 5) of dword
// bin * 32 + (lane & 31): the 32 lanes of a half-wave fall on 32 different banks whatever their bins.
// Ring and sector come from comparisons in fp64, no sqrt and no atan2: ring >= k iff (rho / r)^2 >= (k / l)^4, and the
// angle is at or past the border 2 pi k / t iff the border's direction has the point on its left (within its half turn).
__global__ __launch_bounds__(64 * PROJ_WAVES) void project_kernel(const ScanRef* __restrict__ scans,
                                                                  const Info* __restrict__ info,
                                                                  const Tables* __restrict__ tab, int P, int L, int T,
                                                                  float max_range2, uint32_t chunk,
                                                                  uint32_t* __restrict__ counts) {
  __shared__ uint16_t hist[PROJ_WAVES][MAX_BINS * 64];
  __shared__ double s_ring[MAX_BINS], s_cos[MAX_BINS], s_sin[MAX_BINS];
  const ScanRef sc = scans[blockIdx.y];
  const Info& in = info[blockIdx.y];
  const size_t first = (size_t)blockIdx.x * chunk;
  if (first >= sc.n || in.n_used == 0) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < PROJ_WAVES * MAX_BINS * 32; i += 64 * PROJ_WAVES) reinterpret_cast<uint32_t*>(&hist[0][0])[i] = 0u;
  for (int i = tid; i < MAX_BINS; i += 64 * PROJ_WAVES) {
    s_ring[i] = i < L ? tab->ring_thr[i] : 0.0;
    s_cos[i] = i < T ? tab->sec_cos[i] : 0.0;
    s_sin[i] = i < T ? tab->sec_sin[i] : 0.0;
  }
  __syncthreads();
  const bool active = lane < P;
  const int pl = active ? lane : 0;
  const double ux = tab->u[pl][0], uy = tab->u[pl][1], uz = tab->u[pl][2];
  const double vx = tab->v[pl][0], vy = tab->v[pl][1], vz = tab->v[pl][2];
  double Rm[9], c[3];
  for (int k = 0; k < 9; ++k) Rm[k] = in.R[k];
  for (int k = 0; k < 3; ++k) c[k] = in.c[k];
  const double inv_r2 = in.inv_r2;
  const int half = T >> 1;  // the borders 1 .. half lie in [0, pi]: 2 pi k / t <= pi iff 2 k <= t
  constexpr int PTS = 4;
  // ceil(log2(range)) steps bring a range to one entry: the rings' is L, the sectors' at most half + 1
  const int ring_steps = L > 1 ? 32 - __builtin_clz((unsigned)(L - 1)) : 0, sec_steps = 32 - __builtin_clz((unsigned)half);
  uint16_t* h = &hist[wave][0] + (lane >> 5);
  const int col = lane & 31;
  const size_t end = first + chunk < sc.n ? first + chunk : sc.n;
  for (size_t base = first + (size_t)wave * 64; base < end; base += 64 * PROJ_WAVES) {
    const size_t i = base + lane;
    bool ok = false;
    double y0 = 0.0, y1 = 0.0, y2 = 0.0;
    if (i < end) {
      const float* p = sc.xyz + i * sc.stride;
      const float x = p[0], y = p[1], z = p[2];
      ok = used_point(x, y, z, max_range2);
      const double dx = (double)x - c[0], dy = (double)y - c[1], dz = (double)z - c[2];
      y0 = (dx * Rm[0] + dy * Rm[3]) + dz * Rm[6];  // y = R^T (p - c)
      y1 = (dx * Rm[1] + dy * Rm[4]) + dz * Rm[7];
      y2 = (dx * Rm[2] + dy * Rm[5]) + dz * Rm[8];
    }
    unsigned long long todo = __ballot(ok);
    // PTS points per step: their bisections are independent chains of LDS reads, which hide each other's latency.
    // A bisection keeps [lo, lo + len): the answer's range; its trip count is the same for every lane (a step on a range
    // of one entry changes nothing).  With beta >= 0 the angle lies in [0, pi]: the borders beyond pi are not reached;
    // with beta < 0 those up to pi are all passed.  Within its half turn the angle is at or past border k iff the
    // border's direction has the point on its left.
    while (todo) {
      double px[PTS], py[PTS], pz[PTS];
      bool live[PTS];
#pragma unroll
      for (int u = 0; u < PTS; ++u) {
        live[u] = todo != 0ull;  // (uniform)
        const int j = __builtin_amdgcn_readfirstlane(live[u] ? (int)__builtin_ctzll(todo) : 0);
        todo &= todo - 1ull;     // (0 stays 0)
        px[u] = readlane_f64(y0, j), py[u] = readlane_f64(y1, j), pz[u] = readlane_f64(y2, j);
      }
      if (!active) continue;
      double al[PTS], be[PTS], q[PTS], s[PTS];
      int lo[PTS], len[PTS], ring[PTS];
#pragma unroll
      for (int u = 0; u < PTS; ++u) {
        al[u] = fma(pz[u], uz, fma(py[u], uy, px[u] * ux)), be[u] = fma(pz[u], vz, fma(py[u], vy, px[u] * vx));
        q[u] = fma(be[u], be[u], al[u] * al[u]);
        s[u] = q[u] * inv_r2;  // (r = 0: every q is 0 and the bin is 0 whatever this gives)
        lo[u] = 0, len[u] = L;
      }
      for (int st = 0; st < ring_steps; ++st) {
#pragma unroll
        for (int u = 0; u < PTS; ++u) {
          const int hl = len[u] >> 1, mid = lo[u] + hl;
          const bool ge = s[u] >= s_ring[mid];
          lo[u] = ge ? mid : lo[u], len[u] = ge ? len[u] - hl : hl;
        }
      }
#pragma unroll
      for (int u = 0; u < PTS; ++u) {
        const bool neg = be[u] < 0.0;
        ring[u] = lo[u];
        lo[u] = neg ? half : 0, len[u] = neg ? T - half : half + 1;
      }
      for (int st = 0; st < sec_steps; ++st) {
#pragma unroll
        for (int u = 0; u < PTS; ++u) {
          const int hl = len[u] >> 1, mid = lo[u] + hl;
          const bool ge = fma(s_cos[mid], be[u], -(s_sin[mid] * al[u])) >= 0.0;
          lo[u] = ge ? mid : lo[u], len[u] = ge ? len[u] - hl : hl;
        }
      }
#pragma unroll
      for (int u = 0; u < PTS; ++u) {
        const int bin = q[u] > 0.0 ? ring[u] * T + lo[u] : 0;
        if (live[u]) h[(bin * 32 + col) * 2] += 1;
      }
    }
  }
  __syncthreads();
  const int B = L * T;
  uint32_t* out = counts + (size_t)blockIdx.y * P * B;
  for (int e = tid; e < B * 64; e += 64 * PROJ_WAVES) {
    const int bin = e >> 6, ln = e & 63;
    if (ln >= P) continue;
    uint32_t s = 0;
#pragma unroll
    for (int w = 0; w < PROJ_WAVES; ++w) s += hist[w][(bin * 32 + (ln & 31)) * 2 + (ln >> 5)];
    if (s) atomicAdd(&out[(size_t)ln * B + bin], s);
  }
}

// the 64 lanes' values -> every lane: a fixed butterfly
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = fmax(v, __shfl_xor(v, m, 64));
  return v;
}

// One block of 128 threads per signature: counts [P][B] u32, n_points [1].  The singular vectors of A = counts / n are
// those of the counts, which are exact in fp64; only the sigmas are divided by n.
//   x <- A (A^T x) / |.| from x = 1 / sqrt(P) (A >= 0: never orthogonal to u1) until max |x' - x| <= 2^-46;
//   sigma1 = |A^T u1|, v1 = A^T u1 / sigma1; both negated iff sum u1 < 0.
//   sigma2 = |A^T y| of the same iteration kept orthogonal to u1, until it moves by less than 2^-48 sigma1.
// desc [P + B] fp32, sigma [2] (may be null).  An all-zero matrix or n = 0: the zero row, sigmas 0.
__global__ __launch_bounds__(128) void svd_kernel(const uint32_t* __restrict__ counts, const uint32_t* __restrict__ n_points,
                                                  int P, int B, float* __restrict__ desc, double* __restrict__ sigma) {
  constexpr int LD = MAX_BINS + 1;  // an odd row stride: the rows a half-wave reads at one column fall on different banks
  __shared__ uint32_t A[MAX_PLANES * LD];
  __shared__ double x[MAX_PLANES], u1[MAX_PLANES], w[MAX_BINS], s_flag[2];
  const int tid = threadIdx.x;
  const size_t sig = blockIdx.x;
  const uint32_t* cnt = counts + sig * (size_t)P * B;
  const double n = (double)n_points[sig];
  float* out = desc + sig * (size_t)(P + B);
  for (int i = tid; i < P * B; i += 128) A[(i / B) * LD + (i % B)] = cnt[i];
  if (tid < P) x[tid] = 1.0 / sqrt((double)P);
  __syncthreads();

  auto at_x = [&]() {  // w = A^T x
    if (tid < B) {
      double s = 0.0;
      for (int p = 0; p < P; ++p) s += (double)A[p * LD + tid] * x[p];
      w[tid] = s;
    }
    __syncthreads();
  };
  auto a_w = [&]() -> double {  // row tid of A w (threads < P)
    double s = 0.0;
    if (tid < P)
      for (int j = 0; j < B; ++j) s += (double)A[tid * LD + j] * w[j];
    return s;
  };

  double s1 = 0.0;
  for (int it = 0; it < SVD_ITERS; ++it) {
    at_x();
    const double z = a_w();
    if (tid < 64) {
      const double nrm = sqrt(wave_sum(z * z));
      const double xn = nrm > 0.0 ? z / nrm : 0.0;
      const double diff = wave_max(tid < P ? fabs(xn - x[tid]) : 0.0);
      if (tid < P) x[tid] = xn;
      if (tid == 0) s_flag[0] = diff, s_flag[1] = nrm;
    }
    __syncthreads();
    const double diff = s_flag[0], nrm = s_flag[1];
    __syncthreads();
    if (nrm == 0.0 || diff <= 0x1p-46) break;
  }
  at_x();  // w = A^T u1
  if (tid < 64) {
    const double a = tid < B ? w[tid] : 0.0, b = tid + 64 < B ? w[tid + 64] : 0.0;
    const double nrm = sqrt(wave_sum(a * a + b * b));
    const double su = wave_sum(tid < P ? x[tid] : 0.0);
    if (tid == 0) s_flag[0] = nrm, s_flag[1] = su;
  }
  __syncthreads();
  s1 = s_flag[0];
  const double sgn = s_flag[1] < 0.0 ? -1.0 : 1.0;
  __syncthreads();
  const bool zero = !(s1 > 0.0) || !(n > 0.0);
  if (tid < P) {
    u1[tid] = x[tid];
    out[tid] = zero ? 0.f : (float)(sgn * x[tid]);
  }
  if (tid < B) out[P + tid] = zero ? 0.f : (float)(sgn * (w[tid] / s1));
  if (!sigma) return;
  if (zero) {
    if (tid == 0) sigma[2 * sig] = 0.0, sigma[2 * sig + 1] = 0.0;
    return;
  }
  // sigma2: the same iteration on the complement of u1, from a vector with no symmetry of its own
  double s2 = 0.0;
  if (tid < 64) {
    double y = tid < P ? 1.0 + 0.61803398874989485 * (double)((tid * 7 + 3) % 11) : 0.0;
    const double d = wave_sum(tid < P ? y * u1[tid] : 0.0);
    if (tid < P) y -= d * u1[tid];
    const double nrm = sqrt(wave_sum(y * y));
    if (tid < P) x[tid] = nrm > 0.0 ? y / nrm : 0.0;
  }
  __syncthreads();
  for (int it = 0; it < SVD2_ITERS; ++it) {
    at_x();
    double z = a_w();
    if (tid < 64) {
      const double a = tid < B ? w[tid] : 0.0, b = tid + 64 < B ? w[tid + 64] : 0.0;
      const double sw = sqrt(wave_sum(a * a + b * b));  // |A^T y|
      const double d = wave_sum(tid < P ? z * u1[tid] : 0.0);
      if (tid < P) z -= d * u1[tid];
      const double nrm = sqrt(wave_sum(z * z));
      if (tid < P) x[tid] = nrm > 0.0 ? z / nrm : 0.0;
      if (tid == 0) s_flag[0] = sw, s_flag[1] = nrm;
    }
    __syncthreads();
    const double sw = s_flag[0], nrm = s_flag[1];
    __syncthreads();
    const bool settled = fabs(sw - s2) <= 0x1p-48 * s1;
    s2 = sw;
    if (settled || nrm == 0.0) break;
  }
  if (tid == 0) sigma[2 * sig] = s1 / n, sigma[2 * sig + 1] = s2 / n;
}

}  // namespace m2dp
}  // namespace gloc
