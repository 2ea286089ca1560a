// vgicp.hip -- voxelized generalized ICP refinement (Koide, Yokozuka, Oishi & Banno; fast_gicp's FastVGICP): generalized
// ICP's distribution-to-distribution cost against the voxels of the target instead of its nearest points.  Host side of
// vgicp_kernels.hpp; tests/vgicp_ref.py is the contract.  The C entry points that take a registration handle are in
// reg.hip (they own the handle's layout) and call run() and voxels() here.
//
// A call builds the voxel maps of its distinct targets as NDT builds its cells (ndt.hip: build_cells) -- keys, segmented
// sort, flag scan, one thread per voxel, open-addressing hash tables -- and then runs gn6.hpp's loop of passes WITHOUT a
// search: a pass is the accumulate kernel, which probes the tables, and the shared solve kernel.  Nothing of the 1-NN
// search's batch (job table, corr, d2, launch order) is set up, and a target needs no target index.
#include <algorithm>
#include <vector>

#include "gn6.hpp"
#include "seg_sort.hpp"
#include "vgicp.hpp"
#include "vgicp_kernels.hpp"

using namespace gloc;
using namespace gloc::vgicp;

namespace gloc {
namespace vgicp {

struct Ws {
  DevBuf k0, k1, v0, v1, hist, segs, flag, pos, bsum, total;  // the sort and the flag scan
  DevBuf tgt_desc, aux, first, vox, hkey, hval, toff, tmask;  // voxels of the batch's targets and their hash tables
  DevBuf pose;                                                // [job][12] fp32: what the accumulate kernel moves the source by
};

void ws_free(Ws* w) { delete w; }

namespace {

uint32_t blocks(size_t n, uint32_t t) { return (uint32_t)((n + t - 1) / t); }

// exclusive prefix of n 0/1 flags into pos; *total (device) = their sum
int scan_flags(hipStream_t q, Ws& w, const uint32_t* flag, uint32_t n, uint32_t* pos, uint32_t* total) {
  const uint32_t nb = std::max<uint32_t>(1, blocks(n, ndt::SCAN_BLOCK));
  GLOC_TRY(w.bsum.ensure(sizeof(uint32_t) * nb, q));
  hipLaunchKernelGGL(ndt::scan_sum_kernel, dim3(nb), dim3(ndt::SCAN_BLOCK), 0, q, flag, n, w.bsum.as<uint32_t>());
  hipLaunchKernelGGL(ndt::scan_top_kernel, dim3(1), dim3(ndt::SCAN_BLOCK), 0, q, w.bsum.as<uint32_t>(), nb, total);
  hipLaunchKernelGGL(ndt::scan_apply_kernel, dim3(nb), dim3(ndt::SCAN_BLOCK), 0, q, flag, n, w.bsum.as<uint32_t>(), pos);
  GLOC_HIP(hipGetLastError());
  return GLOC_OK;
}

struct TargetMaps {
  std::vector<uint32_t> first;  // [n_tgt + 1] voxel ranges
  std::vector<uint32_t> toff, tmask;
};

// Voxels of every target and their hash tables (synchronises once, to size the tables).
int build_voxels(hipStream_t q, Ws& w, const std::vector<DevScan>& tg, const gloc_vgicp_params* prm, TargetMaps* out) {
  const uint32_t T = (uint32_t)tg.size();
  std::vector<ndt::TgtDesc> desc(T);
  std::vector<TgtAux> aux(T);
  uint64_t total = 0;
  uint32_t N = 0, max_n = 0;
  for (uint32_t t = 0; t < T; ++t) total += tg[t].n;
  GLOC_REQUIRE(total < (1ull << 31), GLOC_ERR_INVALID, "the targets of one call hold %llu points, more than 2^31", (unsigned long long)total);
  for (uint32_t t = 0; t < T; ++t) {
    desc[t] = ndt::TgtDesc{tg[t].xyz, (uint32_t)tg[t].n, N};
    aux[t] = TgtAux{tg[t].idx.inv, tg[t].nrm};
    N += (uint32_t)tg[t].n;
    max_n = std::max(max_n, (uint32_t)tg[t].n);
  }
  const size_t NN = std::max<uint32_t>(N, 1);
  GLOC_TRY(w.tgt_desc.ensure(sizeof(ndt::TgtDesc) * T, q));
  GLOC_TRY(w.aux.ensure(sizeof(TgtAux) * T, q));
  GLOC_TRY(w.segs.ensure(sizeof(segsort::Seg) * T, q));
  GLOC_TRY(w.k0.ensure(8 * NN, q));
  GLOC_TRY(w.k1.ensure(8 * NN, q));
  GLOC_TRY(w.v0.ensure(4 * NN, q));
  GLOC_TRY(w.v1.ensure(4 * NN, q));
  GLOC_TRY(w.flag.ensure(4 * NN, q));
  GLOC_TRY(w.pos.ensure(4 * NN, q));
  GLOC_TRY(w.total.ensure(16, q));
  GLOC_TRY(w.first.ensure(4 * (T + 1), q));
  GLOC_TRY(w.vox.ensure(sizeof(Voxel) * NN, q));
  GLOC_TRY(w.hist.ensure(segsort::scratch_bytes(T, std::max<uint32_t>(max_n, 1)), q));
  std::vector<segsort::Seg> segs(T);
  for (uint32_t t = 0; t < T; ++t) segs[t] = segsort::Seg{desc[t].begin, desc[t].n};
  GLOC_HIP(hipMemcpyAsync(w.tgt_desc.p, desc.data(), sizeof(ndt::TgtDesc) * T, hipMemcpyHostToDevice, q));
  GLOC_HIP(hipMemcpyAsync(w.aux.p, aux.data(), sizeof(TgtAux) * T, hipMemcpyHostToDevice, q));
  GLOC_HIP(hipMemcpyAsync(w.segs.p, segs.data(), sizeof(segsort::Seg) * T, hipMemcpyHostToDevice, q));
  const float inv = 1.0f / prm->resolution;
  const dim3 g(std::max<uint32_t>(1, blocks(max_n, 256)), T);
  auto* K = reinterpret_cast<unsigned long long*>(w.k0.p);
  auto* K1 = reinterpret_cast<unsigned long long*>(w.k1.p);
  hipLaunchKernelGGL(ndt::cell_keys_kernel, g, dim3(256), 0, q, w.tgt_desc.as<ndt::TgtDesc>(), inv, K, w.v0.as<uint32_t>());
  unsigned long long* kk[2] = {K, K1};
  uint32_t* vv[2] = {w.v0.as<uint32_t>(), w.v1.as<uint32_t>()};
  const int cur = max_n ? segsort::sort_pairs<unsigned long long, 8>(q, kk[0], kk[1], vv[0], vv[1], w.segs.as<segsort::Seg>(), T,
                                                                       max_n, 0, 64, w.hist.as<uint32_t>())
                        : 0;
  hipLaunchKernelGGL(ndt::cell_flags_kernel, g, dim3(256), 0, q, w.tgt_desc.as<ndt::TgtDesc>(), kk[cur], w.flag.as<uint32_t>());
  GLOC_TRY(scan_flags(q, w, w.flag.as<uint32_t>(), N, w.pos.as<uint32_t>(), w.total.as<uint32_t>()));
  hipLaunchKernelGGL(ndt::cell_first_kernel, dim3(1), dim3(256), 0, q, w.tgt_desc.as<ndt::TgtDesc>(), T, w.pos.as<uint32_t>(),
                     w.total.as<uint32_t>(), w.first.as<uint32_t>());
  hipLaunchKernelGGL(voxel_stats_kernel, g, dim3(256), 0, q, w.tgt_desc.as<ndt::TgtDesc>(), w.aux.as<TgtAux>(), kk[cur], vv[cur],
                     w.flag.as<uint32_t>(), w.pos.as<uint32_t>(), (double)prm->resolution, prm->min_points, w.vox.as<Voxel>());
  GLOC_HIP(hipGetLastError());
  out->first.assign(T + 1, 0);
  GLOC_HIP(hipMemcpyAsync(out->first.data(), w.first.p, 4 * (T + 1), hipMemcpyDeviceToHost, q));
  GLOC_HIP(hipStreamSynchronize(q));
  for (uint32_t t = T; t-- > 0;)  // an empty target has no voxels: its range starts where the next one does
    if (desc[t].n == 0) out->first[t] = out->first[t + 1];
  out->toff.assign(T, 0);
  out->tmask.assign(T, 0);
  size_t slots = 0, max_vox = 0;
  for (uint32_t t = 0; t < T; ++t) {
    const size_t nc = out->first[t + 1] - out->first[t];
    max_vox = std::max(max_vox, nc);
    size_t s = 16;
    while (s < 2 * nc) s <<= 1;  // at most half full: a probe always ends at an empty slot
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
  if (max_vox)
    hipLaunchKernelGGL(ndt::cell_hash_kernel<Voxel>, dim3(blocks(max_vox, 256), T), dim3(256), 0, q, w.first.as<uint32_t>(),
                       w.vox.as<Voxel>(), w.toff.as<uint32_t>(), w.tmask.as<uint32_t>(),
                       reinterpret_cast<unsigned long long*>(w.hkey.p), w.hval.as<uint32_t>());
  GLOC_HIP(hipGetLastError());
  GLOC_HIP(hipStreamSynchronize(q));  // (out's vectors are the caller's)
  return GLOC_OK;
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

// scans without normals get them (an allocation beside the scan: nothing a batch in flight reads moves)
int ensure_normals(gloc_scan_store* st, const uint32_t* ids, size_t n, uint32_t k) {
  std::lock_guard<std::mutex> lk(st->mu);
  for (size_t c = 0; c < n; ++c) {
    GLOC_REQUIRE(ids[c] < st->scans.size() && st->scans[ids[c]].live, GLOC_ERR_INVALID, "unknown scan id %u", ids[c]);
    DevScan& s = st->scans[ids[c]];
    if (s.nrm_k == 0) GLOC_TRY(reg::store_build_normals(st, s, k));
  }
  return GLOC_OK;
}

Ws* workspace(Ws** slot) {
  if (!*slot) *slot = new (std::nothrow) Ws;
  return *slot;
}

}  // namespace

int check_params(const gloc_vgicp_params* p) {
  GLOC_REQUIRE(p, GLOC_ERR_INVALID, "params is null");
  GLOC_REQUIRE(p->max_iters >= 1 && p->max_iters <= 10000, GLOC_ERR_INVALID, "max_iters = %u outside [1, 10000]", p->max_iters);
  GLOC_REQUIRE(p->normal_k >= 3 && p->normal_k <= 16, GLOC_ERR_INVALID, "normal_k = %u outside [3, 16]", p->normal_k);
  GLOC_REQUIRE(p->plane_eps > 0.f && p->plane_eps <= 1.f, GLOC_ERR_INVALID, "plane_eps = %g outside (0, 1]", (double)p->plane_eps);
  GLOC_REQUIRE(p->resolution > 0.f && p->resolution <= 3.0e38f, GLOC_ERR_INVALID, "resolution = %g must be > 0 and finite", (double)p->resolution);
  GLOC_REQUIRE(p->neighbors == 1 || p->neighbors == 7 || p->neighbors == 27, GLOC_ERR_INVALID, "neighbors = %u is not one of 1, 7, 27",
               p->neighbors);
  GLOC_REQUIRE(p->min_points >= 1, GLOC_ERR_INVALID, "min_points must be >= 1");
  return GLOC_OK;
}

int run(const Ctx& x, uint32_t src_id, const uint32_t* tgt_ids, size_t n, const float* init_T, const gloc_vgicp_params* prm,
        float* out_T, float* out_rmse, uint32_t* out_iters, int* out_status, double* out_H36, double* out_g6, double* out_sum,
        uint64_t* out_count) {
  GLOC_TRY(check_params(prm));
  GLOC_REQUIRE(tgt_ids && n >= 1 && n <= 4096, GLOC_ERR_INVALID, "n = %zu outside [1, 4096] or null target ids", n);
  GLOC_REQUIRE(x.store, GLOC_ERR_INVALID, "unknown scan id %u", src_id);
  Ws* wp = workspace(x.ws);
  GLOC_REQUIRE(wp, GLOC_ERR_NOMEM, "host allocation failed");
  Ws& w = *wp;
  const hipStream_t q = x.stream;
  // distinct targets, in order of first appearance: one voxel map each
  std::vector<uint32_t> uniq;
  std::vector<uint32_t> job_tgt(n);
  for (size_t c = 0; c < n; ++c) {
    auto it = std::find(uniq.begin(), uniq.end(), tgt_ids[c]);
    job_tgt[c] = (uint32_t)(it - uniq.begin());
    if (it == uniq.end()) uniq.push_back(tgt_ids[c]);
  }
  std::vector<uint32_t> ids(1 + uniq.size());
  ids[0] = src_id;
  std::copy(uniq.begin(), uniq.end(), ids.begin() + 1);
  GLOC_TRY(ensure_normals(x.store, ids.data(), ids.size(), prm->normal_k));
  std::vector<int> cs(ids.size(), 0);  // (no launch order: nothing here searches)
  std::vector<DevScan> scans(ids.size());
  GLOC_TRY(reg::store_get_pinned(x.store, ids.data(), cs.data(), ids.size(), scans.data()));
  Pins pins{x.store, ids, q};
  const DevScan& src = scans[0];
  GLOC_REQUIRE(src.n >= 1 && src.n < (1ull << 31), GLOC_ERR_INVALID, "the source scan is empty or too large");
  GLOC_REQUIRE(src.nrm, GLOC_ERR_STATE, "scan %u lost its normals during the call", src_id);
  for (size_t t = 1; t < scans.size(); ++t)
    GLOC_REQUIRE(scans[t].n == 0 || scans[t].nrm, GLOC_ERR_STATE, "scan %u lost its normals during the call", ids[t]);
  TargetMaps tm;
  {
    ProfScope ps(*x.prof, "vgicp_voxels", q);
    std::vector<DevScan> tg(scans.begin() + 1, scans.end());
    GLOC_TRY(build_voxels(q, w, tg, prm, &tm));
  }
  // the fp32 poses the accumulate kernel reads and the solve kernel writes after every update
  static const float I16[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  std::vector<float> pose(12 * n);
  std::vector<Target> ht(n);
  for (size_t c = 0; c < n; ++c) {
    const float* T = init_T ? init_T + 16 * c : I16;
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) pose[12 * c + 3 * i + j] = T[4 * i + j];
      pose[12 * c + 9 + i] = T[4 * i + 3];
    }
    const uint32_t t = job_tgt[c];
    ht[c] = Target{reinterpret_cast<const unsigned long long*>(w.hkey.p) + tm.toff[t], w.hval.as<uint32_t>() + tm.toff[t], w.vox.as<Voxel>(),
                   tm.tmask[t], 0u};
  }
  GLOC_TRY(w.pose.ensure(sizeof(float) * 12 * n, q));
  GLOC_HIP(hipMemcpyAsync(w.pose.p, pose.data(), sizeof(float) * 12 * n, hipMemcpyHostToDevice, q));
  GLOC_HIP(hipStreamSynchronize(q));  // (pose is a host vector)
  p2l::Ctx g{};
  g.stream = q;
  g.prof = x.prof;
  g.ws = x.gn;
  g.src_pts = src.idx.pts;
  g.n_src = (uint32_t)src.n;
  g.n_jobs = (uint32_t)n;
  g.pose_f32 = w.pose.as<float>();
  g.pose_stride = 12;
  g.nn_pass = nullptr;  // no search: the accumulate kernel finds its own pairs
  const gn6::Loop lp{prm->max_iters, prm->max_corr_dist, prm->trans_eps, prm->rot_eps, "vgicp_accum", "vgicp_solve"};
  const double a = 1.0 - (double)prm->plane_eps;
  const double gate2 = prm->max_corr_dist > 0.f ? (double)prm->max_corr_dist * (double)prm->max_corr_dist : 0.0;
  const float inv_res = 1.0f / prm->resolution;
  const float* src_nrm = src.nrm;
  auto accum = [&](const Target* d_tgts, const gn6::State* states, float, bool skip_stopped, double* partials, uint32_t n_blk) {
    hipLaunchKernelGGL(vgicp_accum_kernel, dim3(n_blk, g.n_jobs), dim3(gn6::ACC_THREADS), 0, q, g.src_pts, src_nrm, g.n_src, d_tgts,
                       g.pose_f32, g.pose_stride, states, inv_res, prm->neighbors, gate2, a, skip_stopped, partials);
  };
  return gn6::run(g, lp, ht, init_T, accum, out_T, out_rmse, out_iters, out_status, out_H36, out_g6, out_sum, out_count);
}

int voxels(const Ctx& x, uint32_t scan_id, const gloc_vgicp_params* prm, size_t capacity, int32_t* out_key3, uint32_t* out_count,
           double* out_mean3, double* out_nn6, size_t* n_voxels) {
  GLOC_TRY(check_params(prm));
  GLOC_REQUIRE(n_voxels, GLOC_ERR_INVALID, "n_voxels is null");
  GLOC_REQUIRE(x.store, GLOC_ERR_INVALID, "unknown scan id %u", scan_id);
  Ws* wp = workspace(x.ws);
  GLOC_REQUIRE(wp, GLOC_ERR_NOMEM, "host allocation failed");
  Ws& w = *wp;
  const hipStream_t q = x.stream;
  GLOC_TRY(ensure_normals(x.store, &scan_id, 1, prm->normal_k));
  const int cs0 = 0;
  std::vector<DevScan> tg(1);
  GLOC_TRY(reg::store_get_pinned(x.store, &scan_id, &cs0, 1, tg.data()));
  Pins pins{x.store, {scan_id}, q};
  GLOC_REQUIRE(tg[0].n == 0 || tg[0].nrm, GLOC_ERR_STATE, "scan %u lost its normals during the call", scan_id);
  TargetMaps tm;
  {
    ProfScope ps(*x.prof, "vgicp_voxels", q);
    GLOC_TRY(build_voxels(q, w, tg, prm, &tm));
  }
  const uint32_t nc = tm.first[1] - tm.first[0];
  std::vector<Voxel> all(nc);
  if (nc) GLOC_HIP(hipMemcpyAsync(all.data(), w.vox.as<Voxel>() + tm.first[0], sizeof(Voxel) * nc, hipMemcpyDeviceToHost, q));
  GLOC_HIP(hipStreamSynchronize(q));
  size_t v = 0;
  for (const Voxel& c : all) {
    if (!c.valid) continue;
    if (v < capacity) {
      if (out_key3)
        for (int a = 0; a < 3; ++a) out_key3[3 * v + a] = (int32_t)((long long)((c.key >> (42 - 21 * a)) & 0x1FFFFF) - ndt::KEY_BIAS);
      if (out_count) out_count[v] = c.count;
      if (out_mean3) std::copy(c.mean, c.mean + 3, out_mean3 + 3 * v);
      if (out_nn6) std::copy(c.nn, c.nn + 6, out_nn6 + 6 * v);
    }
    ++v;
  }
  *n_voxels = v;
  GLOC_REQUIRE(v <= capacity || (!out_key3 && !out_count && !out_mean3 && !out_nn6), GLOC_ERR_INVALID,
               "buffers hold %zu voxels, the scan has %zu", capacity, v);
  return GLOC_OK;
}

}  // namespace vgicp
}  // namespace gloc

extern "C" {

void gloc_vgicp_default_params(gloc_vgicp_params* p) {
  if (!p) return;
  p->max_iters = 30;  // as the other refinements (registration/global_registration.cpp:242)
  p->max_corr_dist = 0.f;
  p->trans_eps = 0.f;
  p->rot_eps = 0.f;
  p->normal_k = 10;  // registration/ground_estimator.cpp:79
  p->plane_eps = 1e-3f;
  p->resolution = 1.0f;  // fast_gicp::FastVGICP's voxel_resolution_ [upstream default]
  p->neighbors = 7;      // fast_gicp's NeighborSearchMethod::DIRECT7
  p->min_points = 1;
  p->reserved_ = 0;
}

}  // extern "C"
