// ransac_sample.hpp -- the keyed 3-point sample of the RANSAC stage (F4), the one statement of it that ransac_hyp_kernel
// (reg_kernels.hpp) and the tuple test of the Fast Global Registration (fgr_kernels.hpp) compile.  oracle_ransac_sample
// is the checker's form of it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "math3.hpp"          // mulhi_idx
#include "synth_kernels.hpp"  // rng_key / rng_draw

namespace gloc {
namespace reg {

// Three indices in [0, n) of (seed, stream, h): the first draw, then up to 16 draws each for a second and a third that
// differ from those before.  false: two of them are still equal (the sample is skipped).
__device__ __forceinline__ bool ransac_sample(uint64_t seed, uint32_t stream, uint32_t h, uint32_t n, uint32_t s[3]) {
  const uint64_t key = synth::rng_key(seed, ((uint64_t)stream << 32) | (uint64_t)h);
  uint64_t ctr = 0;
  uint32_t s0 = mulhi_idx(synth::rng_draw(key, ctr++), n), s1 = s0, s2 = s0;
  for (int tries = 0; tries < 16 && s1 == s0; ++tries) s1 = mulhi_idx(synth::rng_draw(key, ctr++), n);
  for (int tries = 0; tries < 16 && (s2 == s0 || s2 == s1); ++tries)
    s2 = mulhi_idx(synth::rng_draw(key, ctr++), n);
  s[0] = s0;
  s[1] = s1;
  s[2] = s2;
  return !(s0 == s1 || s0 == s2 || s1 == s2);
}

}  // namespace reg
}  // namespace gloc
