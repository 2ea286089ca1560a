// pillar_kernels.hpp -- device side of the PointPillar scan front end (pillar.hip): points_to_voxels and the traced
// model's [P][16] input (model/voxel.py:23-133, s2s_libtorch/gen_libtorch_pointpillar.py:47-62), then the PointNet +
// scatter-mean canvas of PointPillarTest.forward (model/s2s_merged.py:113-127,204-222).  Batched over scans: blockIdx.y
// is the scan, every scan has P rows (its first P points, then zero rows with mask 0).
//
// Launch order per batch:  classify -> segmented radix sort of (voxel index, row) -> runs -> voxel -> gather
//                          [canvas only:] partial -> canvas
// No float atomics anywhere: every sum runs in a fixed order, so two runs give the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gloc {
namespace pillar {

constexpr int FEAT = 64;    // PointNet output channels (s2s_merged.py:153)
constexpr int IN_CH = 14;   // PointNet input channels: the first 14 of the 16
constexpr int TILE = 64;    // sorted rows per wave of the canvas partials
constexpr int SHORT_RUN = 32;  // voxel kernel: runs up to this long are summed by one lane, longer ones by the wave

enum : uint32_t { FLAG_PAD = 1u, FLAG_REAL = 2u };  // per row: padding (Q2), a point of the scan (mask 1)

struct Grid {
  float off[3], res[3];
  int size[3];  // gx, gy, gz
  uint32_t nv;
};

struct Pn {  // PointNet with BatchNorm folded: y = relu((w . x) * scale + shift) * mask
  float w[FEAT][IN_CH];
  float scale[FEAT], shift[FEAT];
};

// float -> int32 as x86's cvttss2si, which the reference's .int() compiles to: toward zero, and NaN or |v| >= 2^31 give
// INT_MIN (Q9).  gfx950's v_cvt_i32_f32 gives 0 for NaN and saturates, so the out-of-range cases are spelled out.
__device__ __forceinline__ int trunc_x86(float v) {
  return (v >= -2147483648.f && v < 2147483648.f) ? (int)v : INT32_MIN;
}

// fp32 add / subtract with x86's NaN results, which the reference's tensors carry: a NaN operand comes back quieted with
// its sign (the first one when both are NaN), and an invalid operation (inf - inf) gives the default NaN 0xFFC00000.
// gfx950 subtracts by adding the negated operand (x - NaN flips the NaN's sign) and its default NaN is positive.
__device__ __forceinline__ float x86_nan(float a, float b, float r) {
  if (__builtin_expect(r == r, 1)) return r;
  if (a != a) return __int_as_float(__float_as_int(a) | 0x00400000);
  if (b != b) return __int_as_float(__float_as_int(b) | 0x00400000);
  return __int_as_float((int)0xFFC00000u);
}
__device__ __forceinline__ float add_x86(float a, float b) { return x86_nan(a, b, a + b); }
__device__ __forceinline__ float sub_x86(float a, float b) { return x86_nan(a, b, a - b); }

struct Row {
  float x, y, z, i;
  int c[3];
  uint32_t flags, index;
};

// One row of one scan: its point (zero past the scan's end), voxel coordinates, padding flag and index.
// voxel_xyz = (p - offset) / res is an fp32 division (Q1; HIP divides fp32 correctly rounded by default), the index is
// x-major x * gy * gz + y * gz + z (Q3, raval_index), a padded row gets index 0 (Q2).
__device__ __forceinline__ Row classify_row(const float* __restrict__ pts, uint64_t first, uint32_t n, int stride,
                                            uint32_t p, const Grid& g) {
  Row r;
  if (p < n) {
    const float* q = pts + (first + p) * (uint64_t)stride;
    r.x = q[0]; r.y = q[1]; r.z = q[2]; r.i = q[3];
  } else {
    r.x = r.y = r.z = r.i = 0.f;
  }
  const float v[3] = {r.x, r.y, r.z};
  bool out = false;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    r.c[k] = trunc_x86((v[k] - g.off[k]) / g.res[k]);
    out |= r.c[k] >= g.size[k] || r.c[k] < 0;
  }
  const bool pad = p >= n || out;
  r.flags = (pad ? FLAG_PAD : 0u) | (p < n ? FLAG_REAL : 0u);
  r.index = pad ? 0u : (uint32_t)((r.c[0] * g.size[1] + r.c[1]) * g.size[2] + r.c[2]);
  return r;
}

// ---- 1: classify: sort keys (voxel index), values (row) and flags ------------------------------------------------
__global__ __launch_bounds__(256) void pillar_classify_kernel(const float* __restrict__ pts,
                                                              const uint64_t* __restrict__ offsets, int stride,
                                                              uint32_t P, Grid g, uint32_t* __restrict__ keys,
                                                              uint32_t* __restrict__ vals, uint32_t* __restrict__ flags) {
  const uint32_t p = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (p >= P) return;
  const uint64_t first = offsets[b], cnt = offsets[b + 1] - first;
  const uint32_t n = cnt < P ? (uint32_t)cnt : P;
  const Row r = classify_row(pts, first, n, stride, p, g);
  const size_t o = (size_t)b * P + p;
  keys[o] = r.index;
  vals[o] = p;
  flags[o] = r.flags;
}

// ---- 2: runs: where each voxel's rows start and end in the sorted order (vrange zeroed before: empty = [0, 0)) ----
__global__ __launch_bounds__(256) void pillar_runs_kernel(const uint32_t* __restrict__ sk, uint32_t P, uint32_t nv,
                                                          uint2* __restrict__ vrange) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (i >= P) return;
  const uint32_t* k = sk + (size_t)b * P;
  const uint32_t v = k[i];
  uint2* vr = vrange + (size_t)b * nv;
  if (i == 0 || k[i - 1] != v) vr[v].x = i;
  if (i == P - 1 || k[i + 1] != v) vr[v].y = i + 1;
}

// ---- 3: voxel: real-row count (Q5) and centroid (Q6) per voxel ------------------------------------------------------
// The centroid is the sum of the xyz of EVERY row of the voxel in row order (the sort is stable, so a run lists its rows
// in row order), in fp32, divided by the number of rows.  The zero rows past a scan's end are not added: a running fp32
// sum that starts at +0 can never become -0 (x + y is -0 only when both are -0, and an exact cancellation gives +0 in
// round-to-nearest), and s + (+0) = s for every s that is not -0 -- so skipping them, or adding +0 for lanes past the end
// of a run, changes no bit.  They are the highest rows and all have index 0, so they are the tail of voxel 0's run.
// A lane per voxel sums runs up to SHORT_RUN rows; a longer run (voxel 0 with every out-of-range row, above all) is read
// 64 rows at a time by the whole wave, the next 64 loaded while the current ones go through the chain one lane at a time.
// Each scan's voxel 0 sits in its own wave, so the chains of a batch run side by side.
__global__ __launch_bounds__(256) void pillar_voxel_kernel(const float* __restrict__ pts, const uint64_t* __restrict__ offsets,
                                                           int stride, uint32_t P, uint32_t nv,
                                                           const uint32_t* __restrict__ sr, const uint32_t* __restrict__ flags,
                                                           const uint2* __restrict__ vrange, float4* __restrict__ vcent,
                                                           float* __restrict__ vcnt) {
  const uint32_t b = blockIdx.y, lane = threadIdx.x & 63;
  const uint32_t v = blockIdx.x * 256 + threadIdx.x;
  const uint64_t first = offsets[b], cnt = offsets[b + 1] - first;
  const uint32_t n = cnt < P ? (uint32_t)cnt : P;
  const float* q = pts + first * (uint64_t)stride;
  const uint32_t* rows = sr + (size_t)b * P;
  const uint32_t* fl = flags + (size_t)b * P;
  uint32_t s = 0, e = 0;
  if (v < nv) {
    const uint2 r = vrange[(size_t)b * nv + v];
    s = r.x; e = r.y;
  }
  const uint32_t n_all = e - s;
  const uint32_t e_sum = v == 0 ? e - (P - n) : e;  // voxel 0: without the zero rows past the scan's end
  float sx = 0.f, sy = 0.f, sz = 0.f;
  uint32_t real = 0;
  const bool is_long = n_all > (uint32_t)SHORT_RUN;
  if (!is_long) {
    for (uint32_t i = s; i < e_sum; ++i) {
      const uint32_t row = rows[i];
      const float* pp = q + (uint64_t)row * stride;
      sx = add_x86(sx, pp[0]); sy = add_x86(sy, pp[1]); sz = add_x86(sz, pp[2]);
      real += (fl[row] & FLAG_PAD) ? 0u : 1u;
    }
  }
  // long runs: the wave takes them one at a time, in lane order
  unsigned long long todo = __builtin_amdgcn_ballot_w64(is_long && v < nv);
  while (todo) {
    const int owner = __builtin_ctzll(todo);
    todo &= todo - 1;
    const uint32_t ls = __builtin_amdgcn_readlane(s, owner), le = __builtin_amdgcn_readlane(e_sum, owner);
    float ax = 0.f, ay = 0.f, az = 0.f;
    uint32_t acnt = 0;
    auto load = [&](uint32_t base, float& x, float& y, float& z, bool& unpadded) {
      const uint32_t i = base + lane;
      x = y = z = 0.f;
      unpadded = false;
      if (i < le) {
        const uint32_t row = rows[i];
        const float* pp = q + (uint64_t)row * stride;
        x = pp[0]; y = pp[1]; z = pp[2];
        unpadded = !(fl[row] & FLAG_PAD);
      }
    };
    float cx, cy, cz;
    bool cu;
    load(ls, cx, cy, cz, cu);
    for (uint32_t base = ls; base < le; base += 64) {
      float nx, ny, nz;
      bool nu;
      load(base + 64, nx, ny, nz, nu);  // the next 64 rows in flight while these go through the chain
      acnt += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(cu));
#pragma unroll
      for (int j = 0; j < 64; ++j) {  // row order; lanes past the run's end hold +0
        ax = add_x86(ax, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cx), j)));
        ay = add_x86(ay, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cy), j)));
        az = add_x86(az, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cz), j)));
      }
      cx = nx; cy = ny; cz = nz; cu = nu;
    }
    if (lane == (uint32_t)owner) {
      sx = ax; sy = ay; sz = az;
      real = acnt;
    }
  }
  if (v >= nv) return;
  const float d = (float)(n_all ? n_all : 1u);  // torch_scatter.scatter_mean: the count clamped at 1
  vcent[(size_t)b * nv + v] = make_float4(sx / d, sy / d, sz / d, 0.f);
  vcnt[(size_t)b * nv + v] = (float)real;
}

// ---- 4: gather: the [P][16] row (Q7), 64 B per thread, consecutive threads on consecutive rows ---------------------
__global__ __launch_bounds__(256) void pillar_gather_kernel(const float* __restrict__ pts, const uint64_t* __restrict__ offsets,
                                                            int stride, uint32_t P, Grid g,
                                                            const float4* __restrict__ vcent, const float* __restrict__ vcnt,
                                                            float4* __restrict__ out) {
  const uint32_t p = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (p >= P) return;
  const uint64_t first = offsets[b], cnt = offsets[b + 1] - first;
  const uint32_t n = cnt < P ? (uint32_t)cnt : P;
  const Row r = classify_row(pts, first, n, stride, p, g);
  const float4 c = vcent[(size_t)b * g.nv + r.index];
  const float count = vcnt[(size_t)b * g.nv + r.index];
  // the voxel centre from the coordinates before padding zeroes them (Q4): rows out of range get centres off the grid
  float ctr[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) ctr[k] = (0.5f + (float)r.c[k]) * g.res[k] + g.off[k];
  float4* o = out + ((size_t)b * P + p) * 4;
  o[0] = make_float4(r.x, r.y, r.z, r.i);
  o[1] = make_float4(count, sub_x86(r.x, c.x), sub_x86(r.y, c.y), sub_x86(r.z, c.z));
  o[2] = make_float4(c.x, c.y, c.z, sub_x86(r.x, ctr[0]));
  o[3] = make_float4(sub_x86(r.y, ctr[1]), sub_x86(r.z, ctr[2]), (float)r.index, (r.flags & FLAG_REAL) ? 1.f : 0.f);
}

// PointNet feature `lane` of one row (uniform across the wave: scalar loads), times the row mask (Q8).  The dot runs in
// channel order without contraction; ReLU keeps NaN, as torch.relu does.
template <int MASK_MODE>
__device__ __forceinline__ double feature(const float* __restrict__ row, uint32_t flag, const float (&w)[IN_CH],
                                          float scale, float shift) {
  float acc = row[0] * w[0];
#pragma unroll
  for (int k = 1; k < IN_CH; ++k) acc += row[k] * w[k];
  float y = acc * scale + shift;
  y = y < 0.f ? 0.f : y;
  const float m = MASK_MODE == 0 ? row[15] : ((flag & FLAG_PAD) ? 0.f : 1.f);
  return (double)(y * m);
}

template <int MASK_MODE>
__device__ __forceinline__ double sum_rows(const float* __restrict__ inp, const uint32_t* __restrict__ rows,
                                           const uint32_t* __restrict__ fl, uint32_t i0, uint32_t i1,
                                           const float (&w)[IN_CH], float scale, float shift) {
  double acc = 0.0;
  for (uint32_t i = i0; i < i1; ++i) {
    const uint32_t row = rows[i];
    acc += feature<MASK_MODE>(inp + (size_t)row * 16, fl[row], w, scale, shift);
  }
  return acc;
}

// ---- 5: partial: per tile of TILE sorted rows, the fp64 sums of the runs that cross its edges ---------------------
// head = the tile's first run, if it began in an earlier tile; tail = its last run, if it goes on into the next.
// part[b][tile][0 = head, 1 = tail][channel].  Lanes are the 64 channels; a wave per tile.
template <int MASK_MODE>
__global__ __launch_bounds__(256) void pillar_partial_kernel(const float* __restrict__ inputs, const uint32_t* __restrict__ sk,
                                                             const uint32_t* __restrict__ sr, const uint32_t* __restrict__ flags,
                                                             uint32_t P, uint32_t n_tiles, const Pn* __restrict__ pn,
                                                             double* __restrict__ part) {
  const uint32_t b = blockIdx.y, lane = threadIdx.x & 63;
  const uint32_t t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= n_tiles) return;
  const uint32_t* k = sk + (size_t)b * P;
  const uint32_t t0 = t * TILE, t1 = t0 + TILE < P ? t0 + TILE : P;
  const uint32_t kf = k[t0], kl = k[t1 - 1];
  const bool head = t0 > 0 && k[t0 - 1] == kf, tail = t1 < P && k[t1] == kl;
  if (!head && !tail) return;
  float w[IN_CH];
#pragma unroll
  for (int c = 0; c < IN_CH; ++c) w[c] = pn->w[lane][c];
  const float scale = pn->scale[lane], shift = pn->shift[lane];
  const float* inp = inputs + (size_t)b * P * 16;
  const uint32_t* rows = sr + (size_t)b * P;
  const uint32_t* fl = flags + (size_t)b * P;
  double* pt = part + ((size_t)b * n_tiles + t) * 2 * FEAT;
  if (head) {
    uint32_t i1 = t0 + 1;
    while (i1 < t1 && k[i1] == kf) ++i1;
    pt[lane] = sum_rows<MASK_MODE>(inp, rows, fl, t0, i1, w, scale, shift);
  }
  if (tail) {
    uint32_t i0 = t1 - 1;
    while (i0 > t0 && k[i0 - 1] == kl) --i0;
    pt[FEAT + lane] = sum_rows<MASK_MODE>(inp, rows, fl, i0, t1, w, scale, shift);
  }
}

// ---- 6: canvas: the mean per voxel into [B][64][nv]; a work-group per 64 voxels, staged in LDS -------------------
// A run inside one tile is summed here in row order; a run across tiles is the tail partial of its first tile plus the
// head partials of the others, in tile order.  Both in fp64, divided by every row of the voxel (padding included, Q8).
template <int MASK_MODE>
__global__ __launch_bounds__(1024) void pillar_canvas_kernel(const float* __restrict__ inputs, const uint32_t* __restrict__ sr,
                                                             const uint32_t* __restrict__ flags, const uint2* __restrict__ vrange,
                                                             uint32_t P, uint32_t nv, uint32_t n_tiles,
                                                             const Pn* __restrict__ pn, const double* __restrict__ part,
                                                             float* __restrict__ canvas) {
  __shared__ float tile[FEAT][64 + 1];
  const uint32_t b = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint32_t v0 = blockIdx.x * 64;
  float w[IN_CH];
#pragma unroll
  for (int c = 0; c < IN_CH; ++c) w[c] = pn->w[lane][c];
  const float scale = pn->scale[lane], shift = pn->shift[lane];
  const float* inp = inputs + (size_t)b * P * 16;
  const uint32_t* rows = sr + (size_t)b * P;
  const uint32_t* fl = flags + (size_t)b * P;
  const double* pb = part + (size_t)b * n_tiles * 2 * FEAT;
  for (uint32_t j = wv; j < 64; j += 16) {
    const uint32_t v = v0 + j;
    float mean = 0.f;
    if (v < nv) {
      const uint2 r = vrange[(size_t)b * nv + v];
      if (r.y > r.x) {
        const uint32_t ts = r.x / TILE, te = (r.y - 1) / TILE;
        double acc;
        if (ts == te) {
          acc = sum_rows<MASK_MODE>(inp, rows, fl, r.x, r.y, w, scale, shift);
        } else {
          acc = pb[(size_t)ts * 2 * FEAT + FEAT + lane];
          for (uint32_t t = ts + 1; t <= te; ++t) acc += pb[(size_t)t * 2 * FEAT + lane];
        }
        mean = (float)(acc / (double)(r.y - r.x));
      }
    }
    tile[lane][j] = mean;
  }
  __syncthreads();
  float* cb = canvas + (size_t)b * FEAT * nv;
  for (uint32_t c = wv; c < (uint32_t)FEAT; c += 16)
    if (v0 + lane < nv) cb[(size_t)c * nv + v0 + lane] = tile[c][lane];
}

}  // namespace pillar
}  // namespace gloc
