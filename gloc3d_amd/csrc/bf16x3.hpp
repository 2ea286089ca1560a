// bf16x3.hpp -- the split-bf16 operand helpers of the implicit-GEMM convolutions (vgg_kernels.hpp,
// pillar_backbone_kernels.hpp).  An fp32 value x is cut in two bf16 values, h = bf16(x), m = bf16(x - h) (x - h is
// exact in fp32, both conversions round to nearest); a product is taken as ah bm + am bh + ah bh on the matrix cores.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gloc {
namespace bf16x3 {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int BK = 32;  // k per pipeline step: four planes of 8

__device__ __forceinline__ uint32_t cvt_pk_bf16(float lo, float hi) {  // round to nearest even; lo in bits 0..15
  uint32_t r;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
  return r;
}
__device__ __forceinline__ void bf16_split2(float x0, float x1, uint32_t& h, uint32_t& m) {
  h = cvt_pk_bf16(x0, x1);
  const float r0 = x0 - __uint_as_float(h << 16), r1 = x1 - __uint_as_float(h & 0xffff0000u);  // exact
  m = cvt_pk_bf16(r0, r1);
}
__device__ __forceinline__ void bf16_split8(const f32x4& a, const f32x4& b, u32x4& h, u32x4& m) {
  uint32_t h0, h1, h2, h3, m0, m1, m2, m3;
  bf16_split2(a.x, a.y, h0, m0);
  bf16_split2(a.z, a.w, h1, m1);
  bf16_split2(b.x, b.y, h2, m2);
  bf16_split2(b.z, b.w, h3, m3);
  h = u32x4{h0, h1, h2, h3};
  m = u32x4{m0, m1, m2, m3};
}

// LDS bytes of a conv work-group of 4 waves with WM x WN tiles of 32 x 32 each: two buffers of [h | m][BK / 8 planes]
// [64 WM + 64 WN + 2 rows] of 16 B
template <int WM, int WN>
constexpr int conv_lds_bytes() {
  return 2 * 2 * (BK / 8) * (64 * WM + 64 * WN + 2) * 16;
}

}  // namespace bf16x3
}  // namespace gloc
