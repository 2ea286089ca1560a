// ndt.hpp -- what reg.hip (which owns the registration handle) calls of ndt.hip.
#pragma once
#include "common.hpp"
#include "scan_store.hpp"

namespace gloc {
namespace ndt {

struct Ws;  // a handle's NDT workspace (created on first use)
void ws_free(Ws* w);

// The handle's view: its store, stream, profiler and workspace slot.
struct Ctx {
  gloc_scan_store* store;
  hipStream_t stream;
  Profiler* prof;
  Ws** ws;
};

// NDT of the source scan (filtered once) against n target scans.  init_T: [n][16] or null (identity); p6 (instead of
// init_T): one evaluation of the derivatives at p6, written to out_sums43 = [score, gradient 6, Hessian 36] per candidate.
int run(const Ctx& x, uint32_t src_id, const uint32_t* tgt_ids, size_t n, const float* init_T, const double* p6,
        const gloc_ndt_params* prm, float* out_T, double* out_prob, uint32_t* out_iters, int* out_converged,
        double* out_sums43);
int cells(const Ctx& x, uint32_t scan_id, const gloc_ndt_params* prm, size_t capacity, int32_t* out_key3,
          uint32_t* out_count, double* out_mean3, double* out_icov9, size_t* n_cells);

}  // namespace ndt
}  // namespace gloc
