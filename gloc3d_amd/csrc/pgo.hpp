// pgo.hpp -- what pgo.hip's entries check before they look at the handle (include/gloc3d.h, gloc_pgo_*): host code only.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/gloc3d.h"

namespace gloc {
namespace pgo {

constexpr size_t MAX_NODES = (size_t)1 << 20, MAX_EDGES = (size_t)1 << 22;

// a graph as the two entries take it
struct Graph {
  const double* poses;
  const uint8_t* fixed;
  size_t n;
  const uint32_t *src, *tgt;
  const float* Z;
  const double* info;
  const uint8_t* mask;
  size_t m;
};

int check_params(const gloc_pgo_params* p);
int check_robust(const gloc_robust_params* r);  // null is fine; a schedule is not
int check_graph(const Graph& g);                // the arrays are not null: ranges, edge ends, a fixed node, finite values

}  // namespace pgo
}  // namespace gloc
