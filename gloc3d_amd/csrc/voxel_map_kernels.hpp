// voxel_map_kernels.hpp -- the voxel map the voxel-based refinements build of their targets (gfx950): the points of every
// target keyed by the voxel they fall into, sorted, one cell per run of equal keys, and an open-addressing hash table per
// target from key to cell.  What a cell holds is its owner's: NDT's Cell and cell_stats_kernel (ndt_kernels.hpp), the
// voxelized generalized ICP's Voxel and voxel_stats_kernel (vgicp_kernels.hpp).  Included by both through voxel_map.hpp,
// the host side; the kernels are static, each translation unit carries its copy.
//
//   cell_keys_kernel -> segmented radix sort by packed key (seg_sort.hpp, stable) -> cell_flags_kernel (a run starts here)
//   -> flag scan -> cell_first_kernel (every target's first cell) -> the owner's statistics kernel, one thread per run
//   -> cell_hash_kernel (valid cells only)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gloc {
namespace voxmap {

constexpr int64_t KEY_BIAS = 1 << 20;         // packed cell key: 21 bits per axis
constexpr unsigned long long KEY_NONE = ~0ull;
constexpr int SCAN_BLOCK = 1024;

struct TgtDesc {  // a target scan of the batch: its points and its slice of the concatenated key / value arrays
  const float* xyz;
  uint32_t n, begin;
};

// ---- flag scan (exclusive prefix of 0 / 1 flags): block sums, one work-group over the block sums, block scan --------
__device__ inline uint32_t block_excl_scan(uint32_t v, uint32_t* sh, uint32_t* total) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int o = 1; o < SCAN_BLOCK; o <<= 1) {
    const uint32_t a = t >= o ? sh[t - o] : 0u;
    __syncthreads();
    sh[t] += a;
    __syncthreads();
  }
  const uint32_t incl = sh[t];
  if (total) *total = sh[SCAN_BLOCK - 1];
  __syncthreads();
  return incl - v;
}

static __global__ __launch_bounds__(SCAN_BLOCK) void scan_sum_kernel(const uint32_t* __restrict__ f, uint32_t n, uint32_t* __restrict__ bsum) {
  __shared__ uint32_t sh[SCAN_BLOCK];
  const uint32_t i = blockIdx.x * SCAN_BLOCK + threadIdx.x;
  uint32_t tot;
  block_excl_scan(i < n ? f[i] : 0u, sh, &tot);
  if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}

static __global__ __launch_bounds__(SCAN_BLOCK) void scan_top_kernel(uint32_t* __restrict__ bsum, uint32_t nb, uint32_t* __restrict__ total) {
  __shared__ uint32_t sh[SCAN_BLOCK];
  uint32_t carry = 0;
  for (uint32_t b0 = 0; b0 < nb; b0 += SCAN_BLOCK) {
    const uint32_t i = b0 + threadIdx.x;
    const uint32_t v = i < nb ? bsum[i] : 0u;
    uint32_t tot;
    const uint32_t ex = block_excl_scan(v, sh, &tot);
    if (i < nb) bsum[i] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) *total = carry;
}

static __global__ __launch_bounds__(SCAN_BLOCK) void scan_apply_kernel(const uint32_t* __restrict__ f, uint32_t n,
                                                                const uint32_t* __restrict__ boff, uint32_t* __restrict__ pos) {
  __shared__ uint32_t sh[SCAN_BLOCK];
  const uint32_t i = blockIdx.x * SCAN_BLOCK + threadIdx.x;
  const uint32_t ex = block_excl_scan(i < n ? f[i] : 0u, sh, nullptr);
  if (i < n) pos[i] = boff[blockIdx.x] + ex;
}

// ---- cells ---------------------------------------------------------------------------------------------------------------
__device__ inline unsigned long long pack_key(long long kx, long long ky, long long kz) {
  return ((unsigned long long)(kx + KEY_BIAS) << 42) | ((unsigned long long)(ky + KEY_BIAS) << 21) |
         (unsigned long long)(kz + KEY_BIAS);
}

static __global__ void cell_keys_kernel(const TgtDesc* __restrict__ tg, float inv, unsigned long long* __restrict__ key,
                                 uint32_t* __restrict__ val) {
  const TgtDesc d = tg[blockIdx.y];
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= d.n) return;
  long long k[3];
  bool ok = true;
  for (int a = 0; a < 3; ++a) {
    const float f = floorf(d.xyz[3 * i + a] * inv);
    ok = ok && fabsf(f) < (float)KEY_BIAS;
    k[a] = ok ? (long long)f : 0;
  }
  key[d.begin + i] = ok ? pack_key(k[0], k[1], k[2]) : KEY_NONE;
  val[d.begin + i] = i;
}

static __global__ void cell_flags_kernel(const TgtDesc* __restrict__ tg, const unsigned long long* __restrict__ key,
                                  uint32_t* __restrict__ flag) {
  const TgtDesc d = tg[blockIdx.y];
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= d.n) return;
  const unsigned long long k = key[d.begin + i];
  flag[d.begin + i] = (k != KEY_NONE && (i == 0 || key[d.begin + i - 1] != k)) ? 1u : 0u;
}

// first cell of every target (the scanned flag at its segment's start) and the total behind the last
static __global__ void cell_first_kernel(const TgtDesc* __restrict__ tg, uint32_t n_tgt, const uint32_t* __restrict__ pos,
                                  const uint32_t* __restrict__ total, uint32_t* __restrict__ first) {
  for (uint32_t t = threadIdx.x; t < n_tgt; t += blockDim.x)
    first[t] = tg[t].n ? pos[tg[t].begin] : 0u;  // (an empty target: fixed up on the host)
  if (threadIdx.x == 0) first[n_tgt] = *total;
}

__device__ __forceinline__ uint32_t hash_slot(unsigned long long k, uint32_t mask) {
  return (uint32_t)((k * 0x9E3779B97F4A7C15ull) >> 32) & mask;
}

// hash tables: target t owns slots [toff[t], toff[t] + tmask[t] + 1); valid cells only.  CellT: anything with a key and
// a valid flag (the cells of ndt_kernels.hpp, the voxels of vgicp_kernels.hpp)
template <class CellT>
static __global__ void cell_hash_kernel(const uint32_t* __restrict__ first, const CellT* __restrict__ cells,
                                 const uint32_t* __restrict__ toff, const uint32_t* __restrict__ tmask,
                                 unsigned long long* __restrict__ hkey, uint32_t* __restrict__ hval) {
  const uint32_t t = blockIdx.y;
  const uint32_t c = first[t] + blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= first[t + 1] || !cells[c].valid) return;
  const unsigned long long k = cells[c].key;
  const uint32_t mask = tmask[t];
  unsigned long long* hk = hkey + toff[t];
  uint32_t s = hash_slot(k, mask);
  while (true) {
    const unsigned long long prev = atomicCAS(&hk[s], KEY_NONE, k);
    if (prev == KEY_NONE) {
      hval[toff[t] + s] = c;
      return;
    }
    s = (s + 1) & mask;
  }
}

}  // namespace voxmap
}  // namespace gloc
