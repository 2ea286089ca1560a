// vgg_kernels.hpp -- VGG16 features[:-2] (the i2i place encoder) on gfx950.  Included only by vgg.hip.
//
// One kernel family: a 3x3 convolution (pad 1, stride 1) as an implicit GEMM on the bf16 matrix cores,
//   out[pixel][co] = bias[co] + sum_k A[pixel][k] W[co][k],   k = tap * Cin + c,  tap = 3 (dy + 1) + (dx + 1),
// M = output pixels, N = Cout, K = 9 Cin (27 padded to 32 for the 3-channel input layer).
//
// Precision: every fp32 operand x is cut in two bf16 values, h = bf16(x), m = bf16(x - h)
// (x - h is exact in fp32, both conversions round to nearest), and a product is taken as  ah bm + am bh + ah bh:
// three v_mfma_f32_32x32x16_bf16, the form of dist_bf16x3_tiled_kernel (knn_kernels.hpp).  The dropped terms, am bm and the
// residuals below m, are at most 3.03 * 2^-16 |a| |w| per product and of either sign.  The weights are split once
// when they are set (vgg_split_weights_kernel); the activations are split on their way into LDS.  The MFMA chain of one
// 32-k step starts from zero and is added to an fp32 total by the VALU after the step: at most six MFMA accumulations
// per rounding of the running sum.
//
// Work-group = 4 waves, 2 along the pixels x 2 along Cout; a wave owns WM x WN tiles of 32 x 32.  A pixel tile of 32 is
// two image rows of 16 columns, so a 2x2 pooling window is four registers of one lane (C/D map of the 32x32 MFMA:
// col = lane & 31 = output channel, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) = pixel: r, r + 1, r + 8, r + 9).
// The work-group covers 16 columns x (BM / 16) rows of one image: a batch gives the same bits as single images.
// Zero padding is the operand load's: taps outside the image are stored to LDS as zeros; no padded copy exists.
// LDS image [buffer][h | m][k / 8 plane][row]: one ds_read_b128 is a lane's K = 16 fragment half (row l % 32,
// k = 8 (l / 32) + j), pixel rows first, then Cout rows; PLANE = ROWS + 2 keeps the ds_write_b128 groups on distinct
// banks (as dist_bf16x3_tiled_kernel).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bf16x3.hpp"

namespace gloc {
namespace vgg {

using namespace bf16x3;  // f32x4, f32x16, bf16x8, u32x4, BK, bf16_split8, conv_lds_bytes (bf16x3.hpp)
enum { EPI_RELU = 1, EPI_POOL = 2, EPI_NCHW = 4 };

// Weights [Cout][Cin][3][3] (torch) -> [Cout][Kp / 8][h 16 B | m 16 B], k = tap * Cin + c, zero for k >= 9 Cin.
// One thread per (co, 8-k chunk).
__global__ __launch_bounds__(256) void vgg_split_weights_kernel(const float* __restrict__ w, int Cout, int Cin, int Kp,
                                                                u32x4* __restrict__ out) {
  const int K8 = Kp / 8;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= Cout * K8) return;
  const int co = i / K8, k0 = (i % K8) * 8;
  float v[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int k = k0 + e;
    const int tap = k / Cin, c = k % Cin;
    v[e] = k < 9 * Cin ? w[((size_t)co * Cin + c) * 9 + tap] : 0.f;
  }
  u32x4 h, m;
  bf16_split8(f32x4{v[0], v[1], v[2], v[3]}, f32x4{v[4], v[5], v[6], v[7]}, h, m);
  out[(size_t)i * 2] = h;
  out[(size_t)i * 2 + 1] = m;
}

// [n][C][HW] -> [n][HW][C]; the per-layer entry point's input for layers that read channels-last.
__global__ __launch_bounds__(256) void vgg_nchw_to_nhwc_kernel(const float* __restrict__ in, size_t n, int C, int HW,
                                                               float* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n * (size_t)C * HW) return;
  const int c = (int)(i % C);
  const size_t r = i / C;
  const int p = (int)(r % HW);
  const size_t img = r / HW;
  out[i] = in[(img * C + c) * HW + p];
}

// grid (tiles_x * tiles_y, Cout / BN, n); 256 threads.  CIN3: `in` is NCHW [n][3][H][W] (the BEV tensor) and Kp = 32;
// otherwise `in` is NHWC [n][H][W][Cin] with Cin % 32 == 0.  Output NHWC [n][Ho][Wo][Cout], or NCHW with EPI_NCHW;
// Ho, Wo = H, W or H / 2, W / 2 with EPI_POOL (H, W even).
template <int WM, int WN, bool CIN3>
__global__ __launch_bounds__(256) void vgg_conv_kernel(const float* __restrict__ in, const u32x4* __restrict__ wsplit,
                                                       const float* __restrict__ bias, float* __restrict__ out, int H,
                                                       int W, int Cin, int Cout, int Kp, int tiles_x, int epi) {
  constexpr int BM = 64 * WM, BN = 64 * WN;
  constexpr int ROWS = BM + BN;
  constexpr int PLANE = ROWS + 2;
  constexpr int KO = BK / 8;
  constexpr int NA = BM * KO / 256;  // A chunks (8 k of one pixel) per thread and step
  constexpr int NB = BN * KO / 256;  // B chunks (8 k of one output channel, h and m) per thread and step
  constexpr int TROWS = BM / 16;     // image rows of the tile
  extern __shared__ u32x4 lds[];

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wm = w & 1, wn = w >> 1;
  const int bx0 = (blockIdx.x % tiles_x) * 16, by0 = (blockIdx.x / tiles_x) * TROWS;
  const int co0 = blockIdx.y * BN;
  const size_t img = blockIdx.z;
  const int K8 = Kp / 8;
  const int nsteps = Kp / BK;

  // chunk j = tid + 256 i: tile row j / KO (pixel, then Cout), plane j % KO
  const int plane = tid % KO;
  int py[NA], px[NA];
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    const int m = (tid + 256 * i) / KO, s = m >> 5, q = m & 31;
    py[i] = by0 + 2 * s + (q >> 4);
    px[i] = bx0 + (q & 15);
  }
  const u32x4* wsrc[NB];
#pragma unroll
  for (int i = 0; i < NB; ++i) wsrc[i] = wsplit + ((size_t)(co0 + (tid + 256 * i) / KO) * K8 + plane) * 2;

  struct Pre {
    f32x4 a[NA][2];
    bool ok[NA];
    u32x4 bh[NB], bm[NB];
  };
  auto gload = [&](Pre& pre, int step) {
    if constexpr (CIN3) {
#pragma unroll
      for (int i = 0; i < NA; ++i) {
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int k = plane * 8 + e, tap = k / 3, c = k - 3 * tap;
          const int sy = py[i] + tap / 3 - 1, sx = px[i] + tap % 3 - 1;
          const bool ok = k < 27 && sy >= 0 && sy < H && sx >= 0 && sx < W;
          v[e] = ok ? in[((img * 3 + c) * H + sy) * W + sx] : 0.f;
        }
        pre.a[i][0] = f32x4{v[0], v[1], v[2], v[3]};
        pre.a[i][1] = f32x4{v[4], v[5], v[6], v[7]};
        pre.ok[i] = true;
      }
    } else {
      const int k0 = step * BK, tap = k0 / Cin, c = k0 - tap * Cin + plane * 8;
      const int dy = tap / 3 - 1, dx = tap % 3 - 1;
#pragma unroll
      for (int i = 0; i < NA; ++i) {
        const int sy = py[i] + dy, sx = px[i] + dx;
        // (the value is selected at the LDS store: a select here would wait for the load right behind it)
        pre.ok[i] = sy >= 0 && sy < H && sx >= 0 && sx < W;
        const float* src = pre.ok[i] ? in + ((img * H + sy) * W + sx) * Cin + c : in;
        pre.a[i][0] = *reinterpret_cast<const f32x4*>(src);
        pre.a[i][1] = *reinterpret_cast<const f32x4*>(src + 4);
      }
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      pre.bh[i] = wsrc[i][(size_t)step * KO * 2];
      pre.bm[i] = wsrc[i][(size_t)step * KO * 2 + 1];
    }
  };
  auto lstore = [&](const Pre& pre, int buf) {
    u32x4* Lh = lds + buf * 2 * KO * PLANE;
    u32x4* Lm = Lh + KO * PLANE;
    const int pl = plane * PLANE;
    const u32x4 z = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      u32x4 h, m;
      bf16_split8(pre.a[i][0], pre.a[i][1], h, m);
      const int row = (tid + 256 * i) / KO;
      Lh[pl + row] = pre.ok[i] ? h : z;
      Lm[pl + row] = pre.ok[i] ? m : z;
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int row = BM + (tid + 256 * i) / KO;
      Lh[pl + row] = pre.bh[i];
      Lm[pl + row] = pre.bm[i];
    }
  };

  f32x16 acc[WM][WN], tot[WM][WN];
#pragma unroll
  for (int i = 0; i < WM; ++i)
#pragma unroll
    for (int t = 0; t < WN; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) tot[i][t][r] = 0.f;
  const int a_row0 = wm * WM * 32 + (lane & 31);
  const int b_row0 = BM + wn * WN * 32 + (lane & 31);
  auto compute = [&](int buf) {
    const u32x4* Lh = lds + buf * 2 * KO * PLANE;
    const u32x4* Lm = Lh + KO * PLANE;
    const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < BK / 16; ++ks) {
      const int pl = (ks * 2 + (lane >> 5)) * PLANE;
      bf16x8 ah[WM], am[WM], bh[WN], bm[WN];
#pragma unroll
      for (int i = 0; i < WM; ++i) {
        ah[i] = __builtin_bit_cast(bf16x8, Lh[pl + a_row0 + i * 32]);
        am[i] = __builtin_bit_cast(bf16x8, Lm[pl + a_row0 + i * 32]);
      }
#pragma unroll
      for (int t = 0; t < WN; ++t) {
        bh[t] = __builtin_bit_cast(bf16x8, Lh[pl + b_row0 + t * 32]);
        bm[t] = __builtin_bit_cast(bf16x8, Lm[pl + b_row0 + t * 32]);
      }
#pragma unroll
      for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int t = 0; t < WN; ++t)
          acc[i][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bm[t], ks == 0 ? zero : acc[i][t], 0, 0, 0);
#pragma unroll
      for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int t = 0; t < WN; ++t) acc[i][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am[i], bh[t], acc[i][t], 0, 0, 0);
#pragma unroll
      for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int t = 0; t < WN; ++t) acc[i][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bh[t], acc[i][t], 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
      for (int t = 0; t < WN; ++t) tot[i][t] += acc[i][t];
  };

  Pre pre;
  gload(pre, 0);
  lstore(pre, 0);
  __syncthreads();
  for (int s = 0; s < nsteps; ++s) {
    const bool more = s + 1 < nsteps;  // uniform
    if (more) gload(pre, s + 1);
    compute(s & 1);
    if (more) lstore(pre, (s + 1) & 1);
    __syncthreads();
  }

  // epilogue: bias, ReLU, 2x2 max (ReLU and max commute with the per-channel bias add), store
  const bool relu = epi & EPI_RELU, pool = epi & EPI_POOL, nchw = epi & EPI_NCHW;
  const int Ho = pool ? H / 2 : H, Wo = pool ? W / 2 : W;
  const int h = lane >> 5;
#pragma unroll
  for (int i = 0; i < WM; ++i) {
    const int y0 = by0 + 2 * (wm * WM + i);  // the sub-tile's first image row
#pragma unroll
    for (int t = 0; t < WN; ++t) {
      const int co = co0 + (wn * WN + t) * 32 + (lane & 31);
      const float b = bias[co];
      float v[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        v[r] = tot[i][t][r] + b;
        if (relu) v[r] = fmaxf(v[r], 0.f);
      }
      if (pool) {
#pragma unroll
        for (int r = 0; r < 8; r += 2) {
          const int x = bx0 + (r & 3) + 8 * (r >> 2) + 4 * h;  // row y0: q = x - bx0 < 16
          if (y0 >= H || x >= W) continue;
          const float p = fmaxf(fmaxf(v[r], v[r + 1]), fmaxf(v[r + 8], v[r + 9]));
          const int yo = y0 / 2, xo = x / 2;
          const size_t o = nchw ? ((img * Cout + co) * Ho + yo) * Wo + xo : ((img * Ho + yo) * Wo + xo) * Cout + co;
          out[o] = p;
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int q = (r & 3) + 8 * (r >> 2) + 4 * h;
          const int y = y0 + (q >> 4), x = bx0 + (q & 15);
          if (y >= H || x >= W) continue;
          const size_t o = nchw ? ((img * Cout + co) * Ho + y) * Wo + x : ((img * Ho + y) * Wo + x) * Cout + co;
          out[o] = v[r];
        }
      }
    }
  }
}

}  // namespace vgg
}  // namespace gloc
