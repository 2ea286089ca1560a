// robust.hpp -- the M-estimator weight of the Gauss-Newton refinements (include/gloc3d.h: "robust weighting"), the one
// statement of it that the accumulate kernels (p2l_kernels.hpp, gicp_kernels.hpp, vgicp_kernels.hpp), the host helpers
// gloc_robust_scale / gloc_robust_weight and gn6::run's table of scales all compile.  tests/robust_ref.py is the contract.
//
//   weight<KIND>(s2, c2)   t = s2 / c2 and the kind's function of t: one fp64 division, a square root for Huber
//   scale_at(prm, k)       c(k) of the schedule: c(0) = scale_start (or scale), c(k + 1) = max(scale, c(k) anneal), fp64
//
// The build has -ffp-contract=off, fp64 division and square root are IEEE on gfx950 as on the host, and nothing here adds
// behind a product: the host and the device give the same bits for the same (s2, c2).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gloc3d.h"

namespace gloc {
namespace robust {

template <int KIND>
__host__ __device__ __forceinline__ double weight(double s2, double c2) {
  const double t = s2 / c2;
  if (KIND == GLOC_ROBUST_HUBER) return t <= 1.0 ? 1.0 : 1.0 / sqrt(t);
  if (KIND == GLOC_ROBUST_CAUCHY) return 1.0 / (1.0 + t);
  if (KIND == GLOC_ROBUST_TUKEY) return t <= 1.0 ? (1.0 - t) * (1.0 - t) : 0.0;
  if (KIND == GLOC_ROBUST_GEMAN_MCCLURE) return 1.0 / ((1.0 + t) * (1.0 + t));
  return 1.0;
}

inline double weight_of(uint32_t kind, double s2, double c2) {
  switch (kind) {
    case GLOC_ROBUST_HUBER: return weight<GLOC_ROBUST_HUBER>(s2, c2);
    case GLOC_ROBUST_CAUCHY: return weight<GLOC_ROBUST_CAUCHY>(s2, c2);
    case GLOC_ROBUST_TUKEY: return weight<GLOC_ROBUST_TUKEY>(s2, c2);
    case GLOC_ROBUST_GEMAN_MCCLURE: return weight<GLOC_ROBUST_GEMAN_MCCLURE>(s2, c2);
    default: return 1.0;
  }
}

inline double scale_first(const gloc_robust_params* p) { return p->scale_start != 0.f ? (double)p->scale_start : (double)p->scale; }
inline double scale_next(const gloc_robust_params* p, double c) {
  const double n = c * (double)p->anneal, c_end = (double)p->scale;
  return n > c_end ? n : c_end;
}

// c(k); *settled, if given: the first update index whose scale IS `scale` (0xFFFFFFFF if that is beyond k)
inline double scale_at(const gloc_robust_params* p, uint32_t k, uint32_t* settled = nullptr) {
  const double c_end = (double)p->scale;
  double c = scale_first(p);
  uint32_t i = 0;
  for (; i < k && c != c_end; ++i) c = scale_next(p, c);
  if (settled) *settled = c == c_end ? i : 0xFFFFFFFFu;
  return c;
}

int check_params(const gloc_robust_params* p);  // p2l.hip

}  // namespace robust
}  // namespace gloc
