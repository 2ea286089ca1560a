// sc_kernels.hpp -- device side of the Scan Context place descriptor (gloc_sc_* of include/gloc3d.h; sc.hip is the host
// side).  Three stages:
//   build:   scatter_kernel   every finite point -> (ring, sector), unsigned max of the height's bit pattern
//            finish_kernel    per descriptor: unit columns in sector-major order, the non-empty-column mask, the ring key
//   compare: dist_kernel      a wave per (row, 4 queries): lane s owns shift s
//   select:  topk_step_kernel 256 keys -> the k smallest, repeated until one list per query is left
// Determinism: the only atomic is the build's integer max (heights are >= 0, so their bit patterns order as the values
// do); a pair's 64 shift sums are fma chains in a fixed order that read nothing but the pair; the selection sorts whole
// 64-bit keys (distance bits, row, shift), which are distinct.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace gloc {
namespace sc {

constexpr int MAX_RINGS = 32, MAX_SECTORS = 64;
constexpr int QB = 4;             // queries a block holds in LDS and a wave scores against the row it has loaded
constexpr int DIST_WAVES = 4;     // waves per block of dist_kernel, a row each
constexpr int ROWS_PER_WAVE = 4;  // rows a wave takes one after the other
constexpr int ROWS_PER_BLOCK = DIST_WAVES * ROWS_PER_WAVE;
constexpr int SORT_N = 256;       // keys one block of topk_step_kernel sorts (two per thread)
constexpr int MAX_K = 64;         // so that a step always shrinks its input: ceil(n / 256) * 64 < n for n > 256
constexpr uint64_t NO_KEY = ~0ull;

struct ScanRef {
  const float* xyz;
  uint32_t n, stride;
};

// bins [n_scans][R * S], zeroed by the caller.  Points are reduced in LDS first: a scan's ~10^5 points fall into ~10^3
// bins, and the block's own maxima are what goes to memory.
__global__ __launch_bounds__(256) void scatter_kernel(const ScanRef* __restrict__ scans, int R, int S, float max_radius,
                                                      float sensor_height, uint32_t* __restrict__ bins) {
  __shared__ uint32_t lb[MAX_RINGS * MAX_SECTORS];
  const ScanRef sc = scans[blockIdx.y];
  const int nb = R * S;
  for (int i = threadIdx.x; i < nb; i += 256) lb[i] = 0;
  __syncthreads();
  const float two_pi = 6.28318530717958647692f;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < sc.n; i += (size_t)gridDim.x * 256) {
    const float* p = sc.xyz + i * sc.stride;
    const float x = p[0], y = p[1], z = p[2];
    if (!(isfinite(x) && isfinite(y) && isfinite(z))) continue;
    const float r = hypotf(x, y);
    if (!(r < max_radius)) continue;
    int ring = (int)floorf(r / max_radius * (float)R);
    ring = ring < R - 1 ? ring : R - 1;
    float th = atan2f(y, x);
    if (th < 0.f) th += two_pi;
    int sec = (int)floorf(th / two_pi * (float)S);
    sec = sec < S - 1 ? sec : S - 1;
    const float v = z + sensor_height;
    if (v > 0.f) atomicMax(&lb[ring * S + sec], __float_as_uint(v));  // (-0 and everything below stay the empty 0)
  }
  __syncthreads();
  uint32_t* out = bins + (size_t)blockIdx.y * nb;
  for (int i = threadIdx.x; i < nb; i += 256)
    if (lb[i]) atomicMax(&out[i], lb[i]);
}

// One descriptor per block of 64 lanes; lane = sector for the columns, lane = ring for the key.
//   unit [row][S][RP]: column j scaled to length 1 (by its maximum first, so that small heights do not underflow in the
//                      squares), zeros for an empty column and for the rings RP pads R to
//   mask [row]:        bit j set: column j holds a height above 0
//   rkeys [row][R]:    (((d[r][0] + d[r][1]) + ...) + d[r][S - 1]) / S in fp32 (may be null: queries have no key)
__global__ __launch_bounds__(64) void finish_kernel(const float* __restrict__ raw, int R, int S, int RP,
                                                    float* __restrict__ unit, uint64_t* __restrict__ mask,
                                                    float* __restrict__ rkeys) {
  const size_t row = blockIdx.x;
  const int lane = threadIdx.x;
  const float* d = raw + row * (size_t)R * S;
  bool ne = false;
  if (lane < S) {
    float m = 0.f;
    for (int r = 0; r < R; ++r) m = fmaxf(m, d[r * S + lane]);
    ne = m > 0.f;
    float nrm = 1.f;
    if (ne) {
      float ss = 0.f;
      for (int r = 0; r < R; ++r) {
        const float t = d[r * S + lane] / m;
        ss = fmaf(t, t, ss);
      }
      nrm = sqrtf(ss);
    }
    float* u = unit + (row * S + lane) * (size_t)RP;
    for (int r = 0; r < RP; ++r) u[r] = (ne && r < R) ? d[r * S + lane] / m / nrm : 0.f;
  }
  const unsigned long long b = __ballot(ne);
  if (lane == 0) mask[row] = b;
  if (rkeys && lane < R) {
    float s = 0.f;
    for (int j = 0; j < S; ++j) s += d[lane * S + j];
    rkeys[row * R + lane] = s / (float)S;
  }
}

// The 64 shift scores of a pair are the wrapped diagonal sums of G = Qu^T Cu (unit columns): lane s walks the diagonal
// G[(j - s) mod S][j], j = 0 .. S-1, so every entry of G is computed once per pair, by the lane that owns its diagonal.
// Column j of the row is the same address for all lanes (an LDS broadcast); the query's column is one 16-byte-aligned
// LDS read per lane and four rings.  Each column's cosine is its own fma chain over the rings (NV * 4 terms, zeros for
// the padding), and the cosines are added in the order of j: at most 4 * NV + 3 roundings in a cosine and S in the sum.
//   rows: row_list[i] (gloc_sc_distances) or row_begin + i;  q_unit / q_mask: the first of this launch's nq queries
//   out_key  [nq][n_rows] (or null): distance bits << 32 | i << 8 | shift -- ascending keys = ascending (distance, row)
//   out_dist / out_shift [nq][n_rows], out_by_shift [nq][n_rows][S] (each may be null)
// LDS: (QB + DIST_WAVES) * S * CV float4; CV >= NV is the column stride (odd where it fits: conflict-free b128 reads).
template <int NV>
__global__ __launch_bounds__(256) void dist_kernel(const float4* __restrict__ q_unit, const uint64_t* __restrict__ q_mask,
                                                   uint32_t nq, const float4* __restrict__ db_unit,
                                                   const uint64_t* __restrict__ db_mask,
                                                   const uint32_t* __restrict__ row_list, uint32_t row_begin,
                                                   uint32_t n_rows, int S, int CV, uint32_t min_common,
                                                   uint64_t* __restrict__ out_key, float* __restrict__ out_dist,
                                                   uint32_t* __restrict__ out_shift, float* __restrict__ out_by_shift) {
  extern __shared__ float4 sc_lds[];
  float4* lq = sc_lds;                       // [QB][S][CV]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float4* lc = sc_lds + (size_t)(QB + wave) * S * CV;  // [S][CV], this wave's row
  const uint32_t q0 = blockIdx.y * QB;
  const int per = S * NV;
  for (int idx = tid; idx < QB * per; idx += 256) {
    const int qq = idx / per, rem = idx - qq * per, col = rem / NV, v = rem - col * NV;
    float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
    if (q0 + qq < nq) val = q_unit[(size_t)(q0 + qq) * per + rem];
    lq[(qq * S + col) * CV + v] = val;
  }
  uint64_t qm[QB];
#pragma unroll
  for (int q = 0; q < QB; ++q) qm[q] = q0 + q < nq ? q_mask[q0 + q] : 0ull;
  const int s = lane < S ? lane : 0;
  const int nqb = (int)(nq - q0 < (uint32_t)QB ? nq - q0 : (uint32_t)QB);
  const uint32_t need = min_common > 1u ? min_common : 1u;
  const uint64_t all = S == 64 ? ~0ull : ((1ull << S) - 1ull);

  for (int it = 0; it < ROWS_PER_WAVE; ++it) {
    const uint32_t i = blockIdx.x * ROWS_PER_BLOCK + it * DIST_WAVES + wave;
    const bool valid = i < n_rows;
    const uint32_t row = valid ? (row_list ? row_list[i] : row_begin + i) : 0u;
    __syncthreads();  // the previous row's reads are done (and, the first time, the queries are not yet needed)
    if (valid)
      for (int idx = lane; idx < per; idx += 64) {
        const int col = idx / NV, v = idx - col * NV;
        lc[col * CV + v] = db_unit[(size_t)row * per + idx];
      }
    __syncthreads();
    if (!valid) continue;  // (uniform per wave; every wave still meets both barriers of every round)
    float acc[QB];
#pragma unroll
    for (int q = 0; q < QB; ++q) acc[q] = 0.f;
    int col = s ? S - s : 0;  // (0 - s) mod S
    for (int j = 0; j < S; ++j) {
      float4 c[NV];
#pragma unroll
      for (int v = 0; v < NV; ++v) c[v] = lc[j * CV + v];
#pragma unroll
      for (int q = 0; q < QB; ++q) {
        if (q >= nqb) break;  // (uniform: the last group of a batch, or a lone query, leaves slots unused)
        const float4* a = lq + (q * S + col) * CV;
        float dot = 0.f;
#pragma unroll
        for (int v = 0; v < NV; ++v) {
          const float4 av = a[v];
          dot = fmaf(av.x, c[v].x, dot);
          dot = fmaf(av.y, c[v].y, dot);
          dot = fmaf(av.z, c[v].z, dot);
          dot = fmaf(av.w, c[v].w, dot);
        }
        acc[q] += dot;
      }
      col = col + 1 == S ? 0 : col + 1;
    }
    const uint64_t cm = db_mask[row];
#pragma unroll
    for (int q = 0; q < QB; ++q) {
      if (q0 + q >= nq) continue;
      // bit j of rot: the query's column (j - s) mod S is non-empty
      const uint64_t rot = s ? (((qm[q] << s) | (qm[q] >> (S - s))) & all) : qm[q];
      const uint32_t cnt = (uint32_t)__popcll(rot & cm);
      float d = cnt >= need ? 1.f - acc[q] / (float)cnt : 1.f;
      d = fmaxf(d, 0.f);  // (a cosine sum a rounding above its count would give -1e-7: the key wants a sign bit of 0)
      const size_t o = (size_t)(q0 + q) * n_rows + i;
      if (out_by_shift && lane < S) out_by_shift[o * S + lane] = d;
      int bs = lane;
      if (lane >= S) d = 2.f;  // never the minimum
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) {
        const float od = __shfl_xor(d, m, 64);
        const int os = __shfl_xor(bs, m, 64);
        if (od < d || (od == d && os < bs)) d = od, bs = os;
      }
      if (lane == 0) {
        if (out_key) out_key[o] = ((uint64_t)__float_as_uint(d) << 32) | ((uint64_t)i << 8) | (uint64_t)bs;
        if (out_dist) out_dist[o] = d;
        if (out_shift) out_shift[o] = (uint32_t)bs;
      }
    }
  }
}

// Block (b, q): the keys in[q][b * 256 .. + 256) (past n_in: NO_KEY) sorted, the first k to out[q][b * k ..].
__global__ __launch_bounds__(SORT_N / 2) void topk_step_kernel(const uint64_t* __restrict__ in, uint32_t n_in, size_t in_stride,
                                                        uint64_t* __restrict__ out, uint32_t k, size_t out_stride) {
  __shared__ uint64_t keys[SORT_N];
  const int tid = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * SORT_N;
  const uint64_t* src = in + blockIdx.y * in_stride;
  for (int i = tid; i < SORT_N; i += SORT_N / 2) keys[i] = base + i < n_in ? src[base + i] : NO_KEY;
  for (int size = 2; size <= SORT_N; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      const int lo = 2 * tid - (tid & (stride - 1)), hi = lo + stride;
      const uint64_t a = keys[lo], b = keys[hi];
      const bool up = (lo & size) == 0;
      if ((a > b) == up) keys[lo] = b, keys[hi] = a;
    }
  __syncthreads();
  uint64_t* dst = out + blockIdx.y * out_stride + (size_t)blockIdx.x * k;
  for (uint32_t i = tid; i < k; i += SORT_N / 2) dst[i] = keys[i];
}

}  // namespace sc
}  // namespace gloc
