// ndt.hip -- NDT scan registration (the reference's ndt_match_3d, registration/global_registration.cpp:250-330) and the
// approximate voxel filter it thins the source with.  Host side of ndt_kernels.hpp; tests/ndt_ref.py is the contract.
// The C entry points that take a registration handle are in reg.hip (they own the handle's layout) and call run() here.
#include <algorithm>
#include <vector>

#include "ndt.hpp"
#include "ndt_kernels.hpp"
#include "voxel_map.hpp"

using namespace gloc;
using namespace gloc::ndt;
using gloc::voxmap::blocks;

namespace gloc {
namespace ndt {

struct Ws {
  voxmap::Ws map;  // cells of the batch's targets and their hash tables; its sort and scan buffers serve the filter too
  DevBuf filt;     // the filtered source, packed xyz
  DevBuf states, evals, outs, partials, cand_tgt, init_T, p6, done, exp;
  uint32_t* h_done = nullptr;  // pinned
  hipEvent_t ev = nullptr;
  ~Ws() {
    if (h_done) (void)hipHostFree(h_done);
    if (ev) (void)hipEventDestroy(ev);
  }
};

void ws_free(Ws* w) { delete w; }

namespace {

constexpr int CHUNK_ROUNDS = 8;  // rounds of (derivatives, state) enqueued between two looks at the done count

// The approximate voxel filter of n points (device, packed xyz) into filt; returns the output count (synchronises).
// leaf <= 0: the finite points, in order.
int approx_voxel(hipStream_t q, voxmap::Ws& w, DevBuf& filt, const float* xyz, uint32_t n, float leaf, uint32_t* m) {
  *m = 0;
  if (n == 0) return GLOC_OK;
  const bool keep_all = !(leaf > 0.f);
  const float inv = keep_all ? 0.f : 1.0f / leaf;
  GLOC_TRY(w.k0.ensure(4 * (size_t)n, q));
  GLOC_TRY(w.k1.ensure(4 * (size_t)n, q));
  GLOC_TRY(w.v0.ensure(4 * (size_t)n, q));
  GLOC_TRY(w.v1.ensure(4 * (size_t)n, q));
  GLOC_TRY(w.flag.ensure(4 * (size_t)n, q));
  GLOC_TRY(w.pos.ensure(4 * (size_t)n, q));
  GLOC_TRY(w.total.ensure(16, q));
  GLOC_TRY(w.hist.ensure(segsort::scratch_bytes(1, n), q));
  GLOC_TRY(w.segs.ensure(sizeof(segsort::Seg), q));
  const segsort::Seg sg{0, n};
  GLOC_HIP(hipMemcpyAsync(w.segs.p, &sg, sizeof(sg), hipMemcpyHostToDevice, q));
  hipLaunchKernelGGL(avf_keys_kernel, dim3(blocks(n, 256)), dim3(256), 0, q, xyz, n, keep_all ? 1.0f : inv,
                     w.k0.as<uint32_t>(), w.v0.as<uint32_t>());
  uint32_t *k[2] = {w.k0.as<uint32_t>(), w.k1.as<uint32_t>()}, *v[2] = {w.v0.as<uint32_t>(), w.v1.as<uint32_t>()};
  int cur = 0;
  if (keep_all) {
    // every finite point is a run of its own, in point order: slot keys are not needed (the keys kernel only marks the
    // points it skips; with inv = 1 its slot value is overwritten below by the flags kernel's view of validity)
  } else {
    cur = segsort::sort_pairs<uint32_t, 8>(q, k[0], k[1], v[0], v[1], w.segs.as<segsort::Seg>(), 1, n, 0, 16,
                                           w.hist.as<uint32_t>());
  }
  hipLaunchKernelGGL(avf_flags_kernel, dim3(blocks(n, 256)), dim3(256), 0, q, xyz, n, keep_all ? 1.0f : inv, k[cur], v[cur],
                     w.flag.as<uint32_t>(), keep_all ? 1 : 0);
  GLOC_TRY(voxmap::scan_flags(q, w, w.flag.as<uint32_t>(), n, w.pos.as<uint32_t>(), w.total.as<uint32_t>()));
  uint32_t cnt = 0;
  GLOC_HIP(hipMemcpyAsync(&cnt, w.total.p, 4, hipMemcpyDeviceToHost, q));
  GLOC_HIP(hipStreamSynchronize(q));
  GLOC_TRY(filt.ensure(12 * (size_t)std::max<uint32_t>(cnt, 1), q));
  hipLaunchKernelGGL(avf_emit_kernel, dim3(blocks(n, 256)), dim3(256), 0, q, xyz, n, k[cur], v[cur], w.flag.as<uint32_t>(),
                     w.pos.as<uint32_t>(), filt.as<float>(), keep_all ? 1 : 0);
  GLOC_HIP(hipGetLastError());
  *m = cnt;
  return GLOC_OK;
}

// Cells of every target and their hash tables (voxmap::build with NDT's statistics kernel)
int target_cells(hipStream_t q, voxmap::Ws& w, const std::vector<DevScan>& tg, const gloc_ndt_params* prm, voxmap::Maps* out) {
  return voxmap::build<Cell>(q, w, tg, prm->resolution, [&](dim3 g, const TgtDesc* d, const unsigned long long* key, const uint32_t* val,
                                                            const uint32_t* flag, const uint32_t* pos) {
    hipLaunchKernelGGL(cell_stats_kernel, g, dim3(256), 0, q, d, key, val, flag, pos, (double)prm->resolution, prm->min_points_per_cell,
                       (double)prm->min_covar_eigvalue_mult, w.cells.as<Cell>());
  }, out);
}

Consts consts_of(const gloc_ndt_params* prm) {
  const double r = prm->resolution, o = prm->outlier_ratio;
  const double c1 = 10.0 * (1.0 - o), c2 = o / (r * r * r);
  const double d3 = -log(c2);
  const double d1 = -log(c1 + c2) - d3;
  const double d2 = -2.0 * log((-log(c1 * exp(-0.5) + c2) - d3) / d1);
  return Consts{r, 1.0 / r, d1, d2};
}

int check_params(const gloc_ndt_params* p) {
  GLOC_REQUIRE(p, GLOC_ERR_INVALID, "params is null");
  GLOC_REQUIRE(p->resolution > 0.f, GLOC_ERR_INVALID, "resolution must be > 0");
  GLOC_REQUIRE(p->max_iters > 0 && p->max_iters <= 10000, GLOC_ERR_INVALID, "max_iters = %u outside [1, 10000]", p->max_iters);
  GLOC_REQUIRE(p->step_size > 0.f && p->trans_eps >= 0.f, GLOC_ERR_INVALID, "step_size must be > 0, trans_eps >= 0");
  GLOC_REQUIRE(p->outlier_ratio > 0.f && p->outlier_ratio < 1.f, GLOC_ERR_INVALID, "outlier_ratio outside (0, 1)");
  GLOC_REQUIRE(p->min_points_per_cell >= 3, GLOC_ERR_INVALID, "min_points_per_cell must be >= 3");
  GLOC_REQUIRE(p->min_covar_eigvalue_mult >= 0.f, GLOC_ERR_INVALID, "min_covar_eigvalue_mult must be >= 0");
  return GLOC_OK;
}

}  // namespace

int run(const Ctx& x, uint32_t src_id, const uint32_t* tgt_ids, size_t n, const float* init_T, const double* p6,
        const gloc_ndt_params* prm, float* out_T, double* out_prob, uint32_t* out_iters, int* out_converged,
        double* out_sums43) {
  GLOC_TRY(check_params(prm));
  GLOC_REQUIRE(tgt_ids && n >= 1 && n <= 4096, GLOC_ERR_INVALID, "n = %zu outside [1, 4096] or null target ids", n);
  GLOC_REQUIRE(x.store, GLOC_ERR_INVALID, "unknown scan id %u", src_id);
  GLOC_TRY(ensure_ws(x.ws));
  Ws& w = **x.ws;
  const hipStream_t q = x.stream;
  Profiler& prof = *x.prof;
  std::vector<uint32_t> uniq, cand_tgt;  // one set of cells per distinct target (the kernels read cand_tgt as int: < 4096)
  reg::distinct_in_order(tgt_ids, n, &uniq, &cand_tgt);
  std::vector<uint32_t> ids(1 + uniq.size());
  ids[0] = src_id;
  std::copy(uniq.begin(), uniq.end(), ids.begin() + 1);
  reg::ScopedPins pins(x.store, q);
  GLOC_TRY(pins.pin(ids.data(), nullptr, ids.size()));
  const std::vector<DevScan>& scans = pins.scans;
  GLOC_REQUIRE(scans[0].n < (1ull << 31), GLOC_ERR_INVALID, "source scan too large");
  uint32_t m = 0;
  {
    ProfScope ps(prof, "ndt_filter", q);
    GLOC_TRY(approx_voxel(q, w.map, w.filt, scans[0].xyz, (uint32_t)scans[0].n, prm->source_leaf, &m));
  }
  GLOC_REQUIRE(m > 0, GLOC_ERR_INVALID, "the filtered source scan is empty");
  voxmap::Maps tc;
  {
    ProfScope ps(prof, "ndt_cells", q);
    std::vector<DevScan> tg(scans.begin() + 1, scans.end());
    GLOC_TRY(target_cells(q, w.map, tg, prm, &tc));
  }
  const uint32_t n_blk = blocks(m, CHUNK);
  GLOC_TRY(w.states.ensure(sizeof(State) * n, q));
  GLOC_TRY(w.evals.ensure(sizeof(Eval) * n, q));
  GLOC_TRY(w.outs.ensure(sizeof(Out) * n, q));
  GLOC_TRY(w.partials.ensure(sizeof(double) * NACC * n_blk * n, q));
  GLOC_TRY(w.cand_tgt.ensure(sizeof(int) * n, q));
  GLOC_TRY(w.done.ensure(16, q));
  if (init_T) GLOC_TRY(w.init_T.ensure(64 * n, q));
  if (p6) GLOC_TRY(w.p6.ensure(48, q));
  if (out_sums43) GLOC_TRY(w.exp.ensure(sizeof(double) * 43 * n, q));
  if (!w.h_done) GLOC_HIP(hipHostMalloc(reinterpret_cast<void**>(&w.h_done), 16, hipHostMallocDefault));
  if (!w.ev) GLOC_HIP(hipEventCreateWithFlags(&w.ev, hipEventDisableTiming));
  GLOC_HIP(hipMemcpyAsync(w.cand_tgt.p, cand_tgt.data(), sizeof(int) * n, hipMemcpyHostToDevice, q));
  if (init_T) GLOC_HIP(hipMemcpyAsync(w.init_T.p, init_T, 64 * n, hipMemcpyHostToDevice, q));
  if (p6) GLOC_HIP(hipMemcpyAsync(w.p6.p, p6, 48, hipMemcpyHostToDevice, q));
  GLOC_HIP(hipMemsetAsync(w.done.p, 0, 16, q));
  const Consts K = consts_of(prm);
  {
    ProfScope ps(prof, "ndt_state", q);
    hipLaunchKernelGGL(ndt_init_kernel, dim3(blocks(n, 64)), dim3(64), 0, q, (uint32_t)n, init_T ? w.init_T.as<float>() : nullptr,
                       p6 ? w.p6.as<double>() : nullptr, w.cand_tgt.as<int>(), (double)m, (double)prm->step_size,
                       (double)prm->trans_eps / 2.0, (double)prm->trans_eps, (int)prm->max_iters, w.states.as<State>(),
                       w.evals.as<Eval>());
  }
  GLOC_HIP(hipGetLastError());
  auto round = [&](double* exp) -> int {
    {
      ProfScope ps(prof, "ndt_deriv", q);
      hipLaunchKernelGGL(ndt_deriv_kernel, dim3(n_blk, (uint32_t)n), dim3(DERIV_THREADS), 0, q, w.filt.as<float>(), m,
                         w.evals.as<Eval>(), w.cand_tgt.as<int>(), w.map.cells.as<Cell>(),
                         reinterpret_cast<unsigned long long*>(w.map.hkey.p), w.map.hval.as<uint32_t>(), w.map.toff.as<uint32_t>(),
                         w.map.tmask.as<uint32_t>(), K, w.partials.as<double>());
    }
    {
      ProfScope ps(prof, "ndt_state", q);
      hipLaunchKernelGGL(ndt_state_kernel, dim3((uint32_t)n), dim3(64), 0, q, w.partials.as<double>(), n_blk, w.states.as<State>(),
                         w.evals.as<Eval>(), w.outs.as<Out>(), w.done.as<uint32_t>(), exp);
    }
    GLOC_HIP(hipGetLastError());
    return GLOC_OK;
  };
  if (out_sums43) {
    GLOC_TRY(round(w.exp.as<double>()));
    GLOC_HIP(hipMemcpyAsync(out_sums43, w.exp.p, sizeof(double) * 43 * n, hipMemcpyDeviceToHost, q));
    GLOC_HIP(hipStreamSynchronize(q));
    return GLOC_OK;
  }
  // evaluations: 1 + per iteration at most 1 + 10 + 1 (first trial, further trials, the Hessian after them)
  const uint64_t max_rounds = 1 + ((uint64_t)prm->max_iters + 2) * 12;
  uint64_t rounds = 0;
  while (true) {
    for (int r = 0; r < CHUNK_ROUNDS; ++r) GLOC_TRY(round(nullptr));
    rounds += CHUNK_ROUNDS;
    GLOC_HIP(hipMemcpyAsync(w.h_done, w.done.p, 4, hipMemcpyDeviceToHost, q));
    GLOC_HIP(hipEventRecord(w.ev, q));
    GLOC_HIP(hipEventSynchronize(w.ev));
    if (*w.h_done >= n) break;
    GLOC_REQUIRE(rounds < max_rounds + CHUNK_ROUNDS, GLOC_ERR_STATE, "NDT did not finish within %llu rounds",
                 (unsigned long long)max_rounds);
  }
  std::vector<Out> o(n);
  GLOC_HIP(hipMemcpyAsync(o.data(), w.outs.p, sizeof(Out) * n, hipMemcpyDeviceToHost, q));
  GLOC_HIP(hipStreamSynchronize(q));
  for (size_t c = 0; c < n; ++c) {
    if (out_T) std::copy(o[c].T, o[c].T + 16, out_T + 16 * c);
    if (out_prob) out_prob[c] = o[c].prob;
    if (out_iters) out_iters[c] = o[c].iters;
    if (out_converged) out_converged[c] = o[c].converged;
  }
  return GLOC_OK;
}

int cells(const Ctx& x, uint32_t scan_id, const gloc_ndt_params* prm, size_t capacity, int32_t* out_key3, uint32_t* out_count,
          double* out_mean3, double* out_icov9, size_t* n_cells) {
  GLOC_TRY(check_params(prm));
  GLOC_REQUIRE(n_cells, GLOC_ERR_INVALID, "n_cells is null");
  GLOC_REQUIRE(x.store, GLOC_ERR_INVALID, "unknown scan id %u", scan_id);
  GLOC_TRY(ensure_ws(x.ws));
  Ws& w = **x.ws;
  const hipStream_t q = x.stream;
  reg::ScopedPins pins(x.store, q);
  GLOC_TRY(pins.pin(&scan_id, nullptr, 1));
  voxmap::Maps tc;
  {
    ProfScope ps(*x.prof, "ndt_cells", q);
    GLOC_TRY(target_cells(q, w.map, pins.scans, prm, &tc));
  }
  GLOC_TRY(voxmap::export_valid<Cell>(q, w.map, tc, capacity, out_key3, out_count, out_mean3, [&](const Cell& c, size_t row) {
    const double* I = c.icov;
    const double full[9] = {I[0], I[1], I[2], I[1], I[3], I[4], I[2], I[4], I[5]};
    if (out_icov9) std::copy(full, full + 9, out_icov9 + 9 * row);
  }, n_cells));
  GLOC_REQUIRE(*n_cells <= capacity || (!out_key3 && !out_count && !out_mean3 && !out_icov9), GLOC_ERR_INVALID,
               "buffers hold %zu cells, the scan has %zu valid cells", capacity, *n_cells);
  return GLOC_OK;
}

}  // namespace ndt
}  // namespace gloc

extern "C" {

void gloc_ndt_default_params(gloc_ndt_params* p) {
  if (!p) return;
  p->source_leaf = 0.2f;              // registration/global_registration.cpp:256
  p->resolution = 0.5f;               // :271
  p->step_size = 0.1f;                // :268
  p->trans_eps = 0.01f;               // :266
  p->max_iters = 35;                  // :274
  p->outlier_ratio = 0.55f;           // pcl::NormalDistributionsTransform's default [upstream]
  p->min_points_per_cell = 6;         // pcl::VoxelGridCovariance's default [upstream]
  p->min_covar_eigvalue_mult = 0.01f; // pcl::VoxelGridCovariance's default [upstream]
}

// Developer / test aid (not part of include/gloc3d.h): the line search's scalar pieces of ndt_kernels.hpp, run on the
// host (no device is touched).  I = [a_l, f_l, g_l, a_u, f_u, g_u] is updated in place where the piece does so.
//   op 0: *out = trial_value(I, x[0] = a_t, x[1] = f_t, x[2] = g_t)
//   op 1: *out = update_interval(I, x[0], x[1], x[2]) ? 1 : 0
//   op 2: close_interval(I, x[0] = phi_0, x[1] = dphi_0, x[2] = mu)
//   op 3: *out = clamp_step(x[0] = a, x[1] = step_min, x[2] = step_max)
int gloc_ndt_debug_line_search(int op, double* I, const double* x, double* out) {
  GLOC_REQUIRE(I && x && out && op >= 0 && op <= 3, GLOC_ERR_INVALID, "null argument or unknown op %d", op);
  *out = 0.0;
  if (op == 0) *out = trial_value(I, x[0], x[1], x[2]);
  if (op == 1) *out = update_interval(I, x[0], x[1], x[2]) ? 1.0 : 0.0;
  if (op == 2) close_interval(I, x[0], x[1], x[2]);
  if (op == 3) *out = clamp_step(x[0], x[1], x[2]);
  return GLOC_OK;
}

int gloc_scan_store_add_approx_voxel(gloc_scan_store* st, uint32_t base_id, float leaf, uint32_t* new_id) {
  GLOC_REQUIRE(st && new_id, GLOC_ERR_INVALID, "null argument");
  GLOC_HIP(hipSetDevice(st->device));
  std::lock_guard<std::mutex> lk(st->mu);
  GLOC_REQUIRE(base_id < st->scans.size() && st->scans[base_id].live, GLOC_ERR_INVALID, "unknown scan id %u", base_id);
  const DevScan base = st->scans[base_id];
  GLOC_REQUIRE(base.n < (1ull << 31), GLOC_ERR_INVALID, "scan too large");
  Ws w;
  uint32_t m = 0;
  GLOC_TRY(approx_voxel(st->stream, w.map, w.filt, base.xyz, (uint32_t)base.n, leaf, &m));
  DevScan s;
  GLOC_TRY(reg::store_make_scan(st, w.filt.as<float>(), m, 3, true, &s));
  return reg::store_insert_scan(st, s, new_id);
}

}  // extern "C"
