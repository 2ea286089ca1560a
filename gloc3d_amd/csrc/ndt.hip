// ndt.hip -- NDT scan registration (the reference's ndt_match_3d, registration/global_registration.cpp:250-330) and the
// approximate voxel filter it thins the source with.  Host side of ndt_kernels.hpp; tests/ndt_ref.py is the contract.
// The C entry points that take a registration handle are in reg.hip (they own the handle's layout) and call run() here.
#include <algorithm>
#include <vector>

#include "ndt.hpp"
#include "ndt_kernels.hpp"
#include "seg_sort.hpp"

using namespace gloc;
using namespace gloc::ndt;

namespace gloc {
namespace ndt {

struct Ws {
  DevBuf k0, k1, v0, v1, hist, segs, flag, pos, bsum, total;  // sorts and flag scans (filter and cells)
  DevBuf filt;                                                // the filtered source, packed xyz
  DevBuf tgt_desc, first, cells, hkey, hval, toff, tmask;     // cells of the batch's targets and their hash tables
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

uint32_t blocks(size_t n, uint32_t t) { return (uint32_t)((n + t - 1) / t); }

// exclusive prefix of n 0/1 flags into pos; *total (device) = their sum
int scan_flags(hipStream_t q, Ws& w, const uint32_t* flag, uint32_t n, uint32_t* pos, uint32_t* total) {
  const uint32_t nb = std::max<uint32_t>(1, blocks(n, SCAN_BLOCK));
  GLOC_TRY(w.bsum.ensure(sizeof(uint32_t) * nb, q));
  hipLaunchKernelGGL(scan_sum_kernel, dim3(nb), dim3(SCAN_BLOCK), 0, q, flag, n, w.bsum.as<uint32_t>());
  hipLaunchKernelGGL(scan_top_kernel, dim3(1), dim3(SCAN_BLOCK), 0, q, w.bsum.as<uint32_t>(), nb, total);
  hipLaunchKernelGGL(scan_apply_kernel, dim3(nb), dim3(SCAN_BLOCK), 0, q, flag, n, w.bsum.as<uint32_t>(), pos);
  GLOC_HIP(hipGetLastError());
  return GLOC_OK;
}

// The approximate voxel filter of n points (device, packed xyz) into w.filt; returns the output count (synchronises).
// leaf <= 0: the finite points, in order.
int approx_voxel(hipStream_t q, Ws& w, const float* xyz, uint32_t n, float leaf, uint32_t* m) {
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
  GLOC_TRY(scan_flags(q, w, w.flag.as<uint32_t>(), n, w.pos.as<uint32_t>(), w.total.as<uint32_t>()));
  uint32_t cnt = 0;
  GLOC_HIP(hipMemcpyAsync(&cnt, w.total.p, 4, hipMemcpyDeviceToHost, q));
  GLOC_HIP(hipStreamSynchronize(q));
  GLOC_TRY(w.filt.ensure(12 * (size_t)std::max<uint32_t>(cnt, 1), q));
  hipLaunchKernelGGL(avf_emit_kernel, dim3(blocks(n, 256)), dim3(256), 0, q, xyz, n, k[cur], v[cur], w.flag.as<uint32_t>(),
                     w.pos.as<uint32_t>(), w.filt.as<float>(), keep_all ? 1 : 0);
  GLOC_HIP(hipGetLastError());
  *m = cnt;
  return GLOC_OK;
}

struct TargetCells {
  std::vector<uint32_t> first;   // [n_tgt + 1] cell ranges
  std::vector<uint32_t> toff, tmask;
};

// Cells of every target and their hash tables (synchronises once, to size the tables).
int build_cells(hipStream_t q, Ws& w, const std::vector<DevScan>& tg, const gloc_ndt_params* prm, TargetCells* out) {
  const uint32_t T = (uint32_t)tg.size();
  std::vector<TgtDesc> desc(T);
  uint32_t N = 0, max_n = 0;
  for (uint32_t t = 0; t < T; ++t) {
    desc[t] = TgtDesc{tg[t].xyz, (uint32_t)tg[t].n, N};
    N += (uint32_t)tg[t].n;
    max_n = std::max(max_n, (uint32_t)tg[t].n);
  }
  const size_t NN = std::max<uint32_t>(N, 1);
  GLOC_TRY(w.tgt_desc.ensure(sizeof(TgtDesc) * T, q));
  GLOC_TRY(w.segs.ensure(sizeof(segsort::Seg) * T, q));
  GLOC_TRY(w.k0.ensure(8 * NN, q));
  GLOC_TRY(w.k1.ensure(8 * NN, q));
  GLOC_TRY(w.v0.ensure(4 * NN, q));
  GLOC_TRY(w.v1.ensure(4 * NN, q));
  GLOC_TRY(w.flag.ensure(4 * NN, q));
  GLOC_TRY(w.pos.ensure(4 * NN, q));
  GLOC_TRY(w.total.ensure(16, q));
  GLOC_TRY(w.first.ensure(4 * (T + 1), q));
  GLOC_TRY(w.cells.ensure(sizeof(Cell) * NN, q));
  GLOC_TRY(w.hist.ensure(segsort::scratch_bytes(T, std::max<uint32_t>(max_n, 1)), q));
  std::vector<segsort::Seg> segs(T);
  for (uint32_t t = 0; t < T; ++t) segs[t] = segsort::Seg{desc[t].begin, desc[t].n};
  GLOC_HIP(hipMemcpyAsync(w.tgt_desc.p, desc.data(), sizeof(TgtDesc) * T, hipMemcpyHostToDevice, q));
  GLOC_HIP(hipMemcpyAsync(w.segs.p, segs.data(), sizeof(segsort::Seg) * T, hipMemcpyHostToDevice, q));
  const float inv = 1.0f / (float)prm->resolution;
  const dim3 g(std::max<uint32_t>(1, blocks(max_n, 256)), T);
  auto* K = reinterpret_cast<unsigned long long*>(w.k0.p);
  auto* K1 = reinterpret_cast<unsigned long long*>(w.k1.p);
  hipLaunchKernelGGL(cell_keys_kernel, g, dim3(256), 0, q, w.tgt_desc.as<TgtDesc>(), inv, K, w.v0.as<uint32_t>());
  unsigned long long* kk[2] = {K, K1};
  uint32_t* vv[2] = {w.v0.as<uint32_t>(), w.v1.as<uint32_t>()};
  const int cur = max_n ? segsort::sort_pairs<unsigned long long, 8>(q, kk[0], kk[1], vv[0], vv[1], w.segs.as<segsort::Seg>(), T,
                                                                       max_n, 0, 64, w.hist.as<uint32_t>())
                        : 0;
  hipLaunchKernelGGL(cell_flags_kernel, g, dim3(256), 0, q, w.tgt_desc.as<TgtDesc>(), kk[cur], w.flag.as<uint32_t>());
  GLOC_TRY(scan_flags(q, w, w.flag.as<uint32_t>(), N, w.pos.as<uint32_t>(), w.total.as<uint32_t>()));
  hipLaunchKernelGGL(cell_first_kernel, dim3(1), dim3(256), 0, q,
                     w.tgt_desc.as<TgtDesc>(), T, w.pos.as<uint32_t>(), w.total.as<uint32_t>(), w.first.as<uint32_t>());
  hipLaunchKernelGGL(cell_stats_kernel, g, dim3(256), 0, q, w.tgt_desc.as<TgtDesc>(), kk[cur], vv[cur], w.flag.as<uint32_t>(),
                     w.pos.as<uint32_t>(), (double)prm->resolution, prm->min_points_per_cell, (double)prm->min_covar_eigvalue_mult,
                     w.cells.as<Cell>());
  GLOC_HIP(hipGetLastError());
  out->first.assign(T + 1, 0);
  GLOC_HIP(hipMemcpyAsync(out->first.data(), w.first.p, 4 * (T + 1), hipMemcpyDeviceToHost, q));
  GLOC_HIP(hipStreamSynchronize(q));
  for (uint32_t t = T; t-- > 0;)  // an empty target has no cells: its range starts where the next one does
    if (desc[t].n == 0) out->first[t] = out->first[t + 1];
  out->toff.assign(T, 0);
  out->tmask.assign(T, 0);
  size_t slots = 0, max_cells = 0;
  for (uint32_t t = 0; t < T; ++t) {
    const size_t nc = out->first[t + 1] - out->first[t];
    max_cells = std::max(max_cells, nc);
    size_t s = 16;
    while (s < 2 * nc) s <<= 1;
    out->toff[t] = (uint32_t)slots;
    out->tmask[t] = (uint32_t)(s - 1);
    slots += s;
  }
  GLOC_TRY(w.hkey.ensure(8 * slots, q));
  GLOC_TRY(w.hval.ensure(4 * slots, q));
  GLOC_TRY(w.toff.ensure(4 * T, q));
  GLOC_TRY(w.tmask.ensure(4 * T, q));
  GLOC_HIP(hipMemsetAsync(w.hkey.p, 0xFF, 8 * slots, q));
  GLOC_HIP(hipMemcpyAsync(w.toff.p, out->toff.data(), 4 * T, hipMemcpyHostToDevice, q));
  GLOC_HIP(hipMemcpyAsync(w.tmask.p, out->tmask.data(), 4 * T, hipMemcpyHostToDevice, q));
  GLOC_HIP(hipMemcpyAsync(w.first.p, out->first.data(), 4 * (T + 1), hipMemcpyHostToDevice, q));
  if (max_cells)
    hipLaunchKernelGGL(cell_hash_kernel<Cell>, dim3(blocks(max_cells, 256), T), dim3(256), 0, q, w.first.as<uint32_t>(),
                       w.cells.as<Cell>(), w.toff.as<uint32_t>(), w.tmask.as<uint32_t>(),
                       reinterpret_cast<unsigned long long*>(w.hkey.p), w.hval.as<uint32_t>());
  GLOC_HIP(hipGetLastError());
  return GLOC_OK;
}

Consts consts_of(const gloc_ndt_params* prm) {
  const double r = prm->resolution, o = prm->outlier_ratio;
  const double c1 = 10.0 * (1.0 - o), c2 = o / (r * r * r);
  const double d3 = -log(c2);
  const double d1 = -log(c1 + c2) - d3;
  const double d2 = -2.0 * log((-log(c1 * exp(-0.5) + c2) - d3) / d1);
  return Consts{r, 1.0 / r, d1, d2};
}

// Pins the scans for the duration of a call (store_get_pinned / store_pin)
struct Pins {
  gloc_scan_store* st;
  std::vector<uint32_t> ids;
  hipStream_t q;
  ~Pins() {
    if (!ids.empty()) {
      (void)hipStreamSynchronize(q);
      reg::store_pin(st, ids.data(), ids.size(), -1);
    }
  }
};

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
  if (!*x.ws) {
    *x.ws = new (std::nothrow) Ws;
    GLOC_REQUIRE(*x.ws, GLOC_ERR_NOMEM, "host allocation failed");
  }
  Ws& w = **x.ws;
  const hipStream_t q = x.stream;
  Profiler& prof = *x.prof;
  // distinct targets, in order of first appearance
  std::vector<uint32_t> uniq;
  std::vector<int> cand_tgt(n);
  for (size_t c = 0; c < n; ++c) {
    auto it = std::find(uniq.begin(), uniq.end(), tgt_ids[c]);
    cand_tgt[c] = (int)(it - uniq.begin());
    if (it == uniq.end()) uniq.push_back(tgt_ids[c]);
  }
  std::vector<uint32_t> ids(1 + uniq.size());
  ids[0] = src_id;
  std::copy(uniq.begin(), uniq.end(), ids.begin() + 1);
  std::vector<int> cs(ids.size(), 0);
  std::vector<DevScan> scans(ids.size());
  GLOC_TRY(reg::store_get_pinned(x.store, ids.data(), cs.data(), ids.size(), scans.data()));
  Pins pins{x.store, ids, q};
  GLOC_REQUIRE(scans[0].n < (1ull << 31), GLOC_ERR_INVALID, "source scan too large");
  uint32_t m = 0;
  {
    ProfScope ps(prof, "ndt_filter", q);
    GLOC_TRY(approx_voxel(q, w, scans[0].xyz, (uint32_t)scans[0].n, prm->source_leaf, &m));
  }
  GLOC_REQUIRE(m > 0, GLOC_ERR_INVALID, "the filtered source scan is empty");
  TargetCells tc;
  {
    ProfScope ps(prof, "ndt_cells", q);
    std::vector<DevScan> tg(scans.begin() + 1, scans.end());
    GLOC_TRY(build_cells(q, w, tg, prm, &tc));
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
                         w.evals.as<Eval>(), w.cand_tgt.as<int>(), w.cells.as<Cell>(),
                         reinterpret_cast<unsigned long long*>(w.hkey.p), w.hval.as<uint32_t>(), w.toff.as<uint32_t>(),
                         w.tmask.as<uint32_t>(), K, w.partials.as<double>());
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
  if (!*x.ws) {
    *x.ws = new (std::nothrow) Ws;
    GLOC_REQUIRE(*x.ws, GLOC_ERR_NOMEM, "host allocation failed");
  }
  Ws& w = **x.ws;
  const hipStream_t q = x.stream;
  const int cs0 = 0;
  std::vector<DevScan> tg(1);
  GLOC_TRY(reg::store_get_pinned(x.store, &scan_id, &cs0, 1, tg.data()));
  Pins pins{x.store, {scan_id}, q};
  TargetCells tc;
  {
    ProfScope ps(*x.prof, "ndt_cells", q);
    GLOC_TRY(build_cells(q, w, tg, prm, &tc));
  }
  const uint32_t nc = tc.first[1] - tc.first[0];
  std::vector<Cell> all(nc);
  if (nc) GLOC_HIP(hipMemcpyAsync(all.data(), w.cells.as<Cell>() + tc.first[0], sizeof(Cell) * nc, hipMemcpyDeviceToHost, q));
  GLOC_HIP(hipStreamSynchronize(q));
  size_t v = 0;
  for (const Cell& c : all) {
    if (!c.valid) continue;
    if (v < capacity) {
      if (out_key3)
        for (int a = 0; a < 3; ++a) out_key3[3 * v + a] = (int32_t)((long long)((c.key >> (42 - 21 * a)) & 0x1FFFFF) - KEY_BIAS);
      if (out_count) out_count[v] = c.count;
      if (out_mean3)
        for (int a = 0; a < 3; ++a) out_mean3[3 * v + a] = c.mean[a];
      if (out_icov9) {
        const double* I = c.icov;
        const double full[9] = {I[0], I[1], I[2], I[1], I[3], I[4], I[2], I[4], I[5]};
        std::copy(full, full + 9, out_icov9 + 9 * v);
      }
    }
    ++v;
  }
  *n_cells = v;
  GLOC_REQUIRE(v <= capacity || (!out_key3 && !out_count && !out_mean3 && !out_icov9), GLOC_ERR_INVALID,
               "buffers hold %zu cells, the scan has %zu valid cells", capacity, v);
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
  GLOC_TRY(approx_voxel(st->stream, w, base.xyz, (uint32_t)base.n, leaf, &m));
  DevScan s;
  GLOC_TRY(reg::store_make_scan(st, w.filt.as<float>(), m, 3, true, &s));
  return reg::store_insert_scan(st, s, new_id);
}

}  // extern "C"
