// Prints the plan of a coarse descriptor kNN search (gloc3d_amd/csrc/knn_plan.hpp: plan_search) for every shape read from
// standard input, one per line: nq n_range first_row dim k candidates fp32_only.  First the constants the test's bounds
// are stated in (SELQ_MAX_ROWS SRR_KC SRR_G MIR_ROWS), then one output line per shape: the seven
// inputs, then the plan's fields as integers in the order of COLUMNS in tests/test_knn_plan_cpu.py (the two rounding
// bounds as their bit patterns).  Host code only: built by the test with the host compiler, plain and under sanitizers.
#include <stdio.h>
#include <string.h>

#include "knn_plan.hpp"

using namespace gloc::knn;

static unsigned bits(float f) {
  unsigned u;
  memcpy(&u, &f, sizeof u);
  return u;
}

int main() {
  long long nq, n_range, first, dim, k, cand, fp32;
  printf("%d %d %d %d\n", SELQ_MAX_ROWS, SRR_KC, SRR_G, MIR_ROWS);  // the constants the test's bounds are stated in
  while (scanf("%lld %lld %lld %lld %lld %lld %lld", &nq, &n_range, &first, &dim, &k, &cand, &fp32) == 7) {
    const SearchPlan p = plan_search((int)nq, (int)n_range, (int)(first % MIR_ROWS), (int)dim, (int)k, (int)cand, fp32 != 0);
    printf("%lld %lld %lld %lld %lld %lld %lld", nq, n_range, first, dim, k, cand, fp32);
    printf(" %d %d %d %d %d %d %d", p.tile.b3, p.tile.t32, p.tile.WQ, p.tile.NT, p.tile.KS, p.tile.BQ, p.tile.BN);
    printf(" %d %u %u %u %zu %zu %zu %d", p.kps, p.gx, p.gy, p.gz, p.ld, p.qpad, p.strideP, p.KC);
    printf(" %d %d %d %d %d", (int)p.qraw, (int)p.use_bmin, p.n_blocks, (int)p.large, (int)p.fused);
    printf(" %d %d %d", (int)p.sel.form, p.sel.sl.S, p.sel.sl.L);
    printf(" %d %d %d %d", (int)p.how_redo, (int)p.redo.form, p.redo.sl.S, p.redo.sl.L);
    printf(" %u %u\n", bits(p.eps_rel_d), bits(p.eps_rel_n));
  }
  return 0;
}
