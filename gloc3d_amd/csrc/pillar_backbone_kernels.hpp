// pillar_backbone_kernels.hpp -- the PointPillar 2-D backbone (PointPillarTest after the scatter-mean,
// model/s2s_merged.py:152-188,219-247) on gfx950.  Included only by pillar_backbone.hip.
//
// A 3x3 convolution (pad 1, stride 1 or 2, no bias) with eval BatchNorm and optional ReLU as an implicit GEMM on the
// bf16 matrix cores, the form of vgg_conv_kernel (vgg_kernels.hpp):
//   acc[pixel][co] = sum_k A[pixel][k] W[co][k],  k = tap * Cin + c,  tap = 3 (dy + 1) + (dx + 1),
//   out = acc * scale[co] + shift[co]  (scale = gamma / sqrt(var + eps), shift = beta - mean * scale, per channel),
// M = output pixels, N = Cout, K = 9 Cin with Cin % 32 == 0 (64, 128, 256, 448): a 32-k step never crosses a tap.
// Precision is VGG's (DESIGN.md sections 8, 9): both operands split in bf16 hi + lo (bf16x3.hpp), three
// v_mfma_f32_32x32x16_bf16 per product, each 32-k chain from zero added to an fp32 total by the VALU.  BatchNorm is
// applied to that fp32 total in the epilogue, not folded into the weights.
//
// Work-group = 4 waves, 2 along the pixels x 2 along Cout, a wave owns WM x WN tiles of 32 x 32; a pixel tile of 32 is
// two output rows of 16 columns (C/D map of the 32x32 MFMA: col = lane & 31 = output channel, row = (r & 3) +
// 8 (r >> 2) + 4 (lane >> 5) = pixel).  A work-group covers 16 columns x (BM / 16) rows of one scan's output: a batch
// gives the same bits as single scans.  Output pixels past the map (widths 40 and 20 are not multiples of 16, heights
// 35 and 140 not of 8) are computed from in-bounds addresses and not stored.  Input taps outside the map are zeros at
// the LDS store (the padding): no padded copy exists.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bf16x3.hpp"

namespace gloc {
namespace pillar {

using namespace bf16x3;

// epilogue: ReLU; output layout (else NHWC [n][Ho][Wo][ldc] at channel offset c_off)
enum { BB_RELU = 1, BB_NCHW = 2, BB_NCWH = 4 };

// Weights [Cout][Cin][3][3] (torch) -> [Cout][9 Cin / 8][h 16 B | m 16 B], k = tap * Cin + c.
// One thread per (co, 8-k chunk).
__global__ __launch_bounds__(256) void bb_split_weights_kernel(const float* __restrict__ w, int Cout, int Cin,
                                                               u32x4* __restrict__ out) {
  const int K8 = 9 * Cin / 8;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= Cout * K8) return;
  const int co = i / K8, k0 = (i % K8) * 8;
  float v[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int k = k0 + e;
    const int tap = k / Cin, c = k % Cin;
    v[e] = w[((size_t)co * Cin + c) * 9 + tap];
  }
  u32x4 h, m;
  bf16_split8(f32x4{v[0], v[1], v[2], v[3]}, f32x4{v[4], v[5], v[6], v[7]}, h, m);
  out[(size_t)i * 2] = h;
  out[(size_t)i * 2 + 1] = m;
}

// [n][C][HW] -> [n][HW][C]: the canvas (and the per-layer call's NCHW input) to channels-last.  One thread per output.
__global__ __launch_bounds__(256) void bb_nchw_to_nhwc_kernel(const float* __restrict__ in, size_t n, int C, int HW,
                                                              float* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n * (size_t)C * HW) return;
  const int c = (int)(i % C);
  const size_t r = i / C;
  const int p = (int)(r % HW);
  const size_t img = r / HW;
  out[i] = in[(img * C + c) * HW + p];
}

// nn.Upsample(scale_factor=s, mode="bilinear", align_corners=True) on NHWC [n][H][W][C] -> [n][sH][sW][C], the
// arithmetic of torch's CPU kernel (UpSampleKernel.cpp, float opmath): src = ((in - 1) / (out - 1)) * dst,
// i0 = (int)src, i1 = i0 + (i0 < in - 1), l1 = src - i0, l0 = 1 - l1,
// out = h0 (w0 a00 + w1 a01) + h1 (w0 a10 + w1 a11).  One thread per output.
__global__ __launch_bounds__(256) void bb_upsample_kernel(const float* __restrict__ in, size_t n, int H, int W, int C,
                                                          int s, float* __restrict__ out) {
  const int Ho = H * s, Wo = W * s;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n * (size_t)Ho * Wo * C) return;
  const int c = (int)(i % C);
  size_t r = i / C;
  const int x = (int)(r % Wo);
  r /= Wo;
  const int y = (int)(r % Ho);
  const size_t img = r / Ho;
  const float sh = Ho > 1 ? (float)(H - 1) / (float)(Ho - 1) : 0.f;
  const float sw = Wo > 1 ? (float)(W - 1) / (float)(Wo - 1) : 0.f;
  const float fy = sh * (float)y, fx = sw * (float)x;
  const int y0 = (int)fy, x0 = (int)fx;
  const int y1 = y0 + (y0 < H - 1 ? 1 : 0), x1 = x0 + (x0 < W - 1 ? 1 : 0);
  const float h1 = fminf(fmaxf(fy - (float)y0, 0.f), 1.f), h0 = 1.f - h1;
  const float w1 = fminf(fmaxf(fx - (float)x0, 0.f), 1.f), w0 = 1.f - w1;
  const float* base = in + img * H * W * C + c;
  const float a00 = base[((size_t)y0 * W + x0) * C], a01 = base[((size_t)y0 * W + x1) * C];
  const float a10 = base[((size_t)y1 * W + x0) * C], a11 = base[((size_t)y1 * W + x1) * C];
  out[i] = h0 * (w0 * a00 + w1 * a01) + h1 * (w0 * a10 + w1 * a11);
}

// grid (tiles_x * tiles_y, Cout / BN, n); 256 threads.  `in` is NHWC [n][Hi][Wi][Cin], Cin % 32 == 0; output pixel
// (y, x) reads input (stride y + dy, stride x + dx).  Output [n][Ho][Wo][ldc] at channel c_off (NHWC), or
// [n][Cout][Ho][Wo] (BB_NCHW), or [n][Cout][Wo][Ho] (BB_NCWH, the backbone's final .transpose(3, 2)).
template <int WM, int WN>
__global__ __launch_bounds__(256) void bb_conv_kernel(const float* __restrict__ in, const u32x4* __restrict__ wsplit,
                                                      const float* __restrict__ scale, const float* __restrict__ shift,
                                                      float* __restrict__ out, int Hi, int Wi, int Ho, int Wo, int Cin,
                                                      int Cout, int stride, int tiles_x, int epi, int ldc, int c_off) {
  constexpr int BM = 64 * WM, BN = 64 * WN;
  constexpr int ROWS = BM + BN;
  constexpr int PLANE = ROWS + 2;
  constexpr int KO = BK / 8;
  constexpr int NA = BM * KO / 256;  // A chunks (8 k of one pixel) per thread and step
  constexpr int NB = BN * KO / 256;  // B chunks (8 k of one output channel, h and m) per thread and step
  constexpr int TROWS = BM / 16;     // output rows of the tile
  extern __shared__ u32x4 lds[];

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wm = w & 1, wn = w >> 1;
  const int bx0 = (blockIdx.x % tiles_x) * 16, by0 = (blockIdx.x / tiles_x) * TROWS;
  const int co0 = blockIdx.y * BN;
  const size_t img = blockIdx.z;
  const int K8 = 9 * Cin / 8;
  const int nsteps = 9 * Cin / BK;

  // chunk j = tid + 256 i: tile row j / KO (pixel, then Cout), plane j % KO
  const int plane = tid % KO;
  int py[NA], px[NA];  // the input position of the output pixel's centre tap
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    const int m = (tid + 256 * i) / KO, s = m >> 5, q = m & 31;
    py[i] = (by0 + 2 * s + (q >> 4)) * stride;
    px[i] = (bx0 + (q & 15)) * stride;
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
    const int k0 = step * BK, tap = k0 / Cin, c = k0 - tap * Cin + plane * 8;
    const int dy = tap / 3 - 1, dx = tap % 3 - 1;
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const int sy = py[i] + dy, sx = px[i] + dx;
      // (the value is selected at the LDS store: a select here would wait for the load right behind it)
      pre.ok[i] = sy >= 0 && sy < Hi && sx >= 0 && sx < Wi;
      const float* src = pre.ok[i] ? in + ((img * Hi + sy) * Wi + sx) * Cin + c : in;
      pre.a[i][0] = *reinterpret_cast<const f32x4*>(src);
      pre.a[i][1] = *reinterpret_cast<const f32x4*>(src + 4);
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

  // epilogue: BatchNorm, ReLU, store of the pixels inside the map
  const bool relu = epi & BB_RELU;
  const int h = lane >> 5;
#pragma unroll
  for (int i = 0; i < WM; ++i) {
    const int y0 = by0 + 2 * (wm * WM + i);  // the sub-tile's first output row
#pragma unroll
    for (int t = 0; t < WN; ++t) {
      const int co = co0 + (wn * WN + t) * 32 + (lane & 31);
      const float sc = scale[co], sh = shift[co];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int q = (r & 3) + 8 * (r >> 2) + 4 * h;
        const int y = y0 + (q >> 4), x = bx0 + (q & 15);
        if (y >= Ho || x >= Wo) continue;
        float v = tot[i][t][r] * sc + sh;
        if (relu) v = fmaxf(v, 0.f);
        size_t o;
        if (epi & BB_NCHW)
          o = ((img * Cout + co) * Ho + y) * Wo + x;
        else if (epi & BB_NCWH)
          o = ((img * Cout + co) * Wo + x) * Ho + y;
        else
          o = ((img * Ho + y) * Wo + x) * ldc + c_off + co;
        out[o] = v;
      }
    }
  }
}

}  // namespace pillar
}  // namespace gloc
