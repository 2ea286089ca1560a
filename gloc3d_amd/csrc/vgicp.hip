// vgicp.hip -- voxelized generalized ICP refinement (Koide, Yokozuka, Oishi & Banno; fast_gicp's FastVGICP): generalized
// ICP's distribution-to-distribution cost against the voxels of the target instead of its nearest points.  Host side of
// vgicp_kernels.hpp; tests/vgicp_ref.py is the contract.  The C entry points that take a registration handle are in
// reg.hip (they own the handle's layout) and call run() and voxels() here.
//
// A call builds the voxel maps of its distinct targets with the builder NDT builds its cells with (voxel_map.hpp) -- keys,
// segmented sort, flag scan, one thread per voxel, open-addressing hash tables -- and then runs gn6.hpp's loop of passes
// WITHOUT a search: a pass is the accumulate kernel, which probes the tables, and the shared solve kernel.  Nothing of
// the 1-NN search's batch (job table, corr, d2, launch order) is set up, and a target needs no target index.
//
// run() also takes its targets as views into resident voxel maps (vmap.hip), which outlive the call: then it builds nothing
// and resolves the sources alone; the poses, the loop and the kernels are the same.
#include <algorithm>
#include <vector>

#include "gn6.hpp"
#include "vgicp.hpp"
#include "vgicp_kernels.hpp"
#include "voxel_map.hpp"

using namespace gloc;
using namespace gloc::vgicp;

namespace gloc {
namespace vgicp {

struct Ws {
  voxmap::Ws map;  // voxels of the batch's targets and their hash tables
  DevBuf aux;      // [target] TgtAux
  DevBuf pose;     // [job][12] fp32: what the accumulate kernel moves the source by
};

void ws_free(Ws* w) { delete w; }

namespace {

// Voxels of every target and their hash tables (voxmap::build with the statistics kernel that reads the normals)
int target_voxels(hipStream_t q, Ws& w, const std::vector<DevScan>& tg, const gloc_vgicp_params* prm, voxmap::Maps* out) {
  std::vector<TgtAux> aux(tg.size());
  for (size_t t = 0; t < tg.size(); ++t) aux[t] = TgtAux{tg[t].idx.inv, tg[t].nrm};
  GLOC_TRY(w.aux.ensure(sizeof(TgtAux) * aux.size(), q));
  GLOC_HIP(hipMemcpyAsync(w.aux.p, aux.data(), sizeof(TgtAux) * aux.size(), hipMemcpyHostToDevice, q));  // (build() synchronises)
  return voxmap::build<Voxel>(q, w.map, tg, prm->resolution, [&](dim3 g, const voxmap::TgtDesc* d, const unsigned long long* key,
                                                                 const uint32_t* val, const uint32_t* flag, const uint32_t* pos) {
    hipLaunchKernelGGL(voxel_stats_kernel, g, dim3(256), 0, q, d, w.aux.as<TgtAux>(), key, val, flag, pos, (double)prm->resolution,
                       prm->min_points, w.map.cells.as<Voxel>());
  }, out);
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

int run(const Ctx& x, const gn6::Call& c, const gloc_vgicp_params* prm, const Target* resident) {
  const hipStream_t q = x.stream;
  const size_t n = c.n;
  // every distinct source, then every distinct target -- one voxel map each; no launch order: nothing here searches.
  // Against resident maps the call's targets are no scans: the sources alone are resolved, as those of rows without a target
  reg::CallScans rs(x.store, q);
  const std::vector<uint32_t> no_scans(resident ? n : 0, reg::NO_SCAN);
  gn6::Call cs = c;
  if (resident) cs.tgt_ids = no_scans.data();
  GLOC_TRY(rs.resolve(cs, prm->normal_k, true, 0));
  GLOC_TRY(ensure_ws(x.ws));
  Ws& w = **x.ws;
  voxmap::Maps tm;
  if (rs.pins.scans.size() > rs.n_srcs) {
    ProfScope ps(*x.prof, "vgicp_voxels", q);
    std::vector<DevScan> tg(rs.pins.scans.begin() + rs.n_srcs, rs.pins.scans.end());
    GLOC_TRY(target_voxels(q, w, tg, prm, &tm));
  }
  // the fp32 poses the accumulate kernel reads and the solve kernel writes after every update
  static const float I16[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  std::vector<float> pose(12 * n);
  std::vector<Target> ht(n, Target{nullptr, nullptr, nullptr, 0u, 0u});  // (a row without a target: no table to probe)
  for (size_t j = 0; j < n; ++j) {
    const float* T = c.init_T ? c.init_T + 16 * j : I16;
    for (int i = 0; i < 3; ++i) {
      for (int k = 0; k < 3; ++k) pose[12 * j + 3 * i + k] = T[4 * i + k];
      pose[12 * j + 9 + i] = T[4 * i + 3];
    }
    const uint32_t t = rs.job_tgt[j];
    if (t != reg::NO_SCAN)
      ht[j] = Target{reinterpret_cast<const unsigned long long*>(w.map.hkey.p) + tm.toff[t], w.map.hval.as<uint32_t>() + tm.toff[t],
                     w.map.cells.as<Voxel>(), tm.tmask[t], 0u};
    if (resident && resident[j].hkey) {  // (resolved as a row without a target: its source is summed after all)
      ht[j] = resident[j];
      rs.srcs[j].n = (uint32_t)rs.src(j).n;
    }
  }
  GLOC_TRY(w.pose.ensure(sizeof(float) * 12 * n, q));
  GLOC_HIP(hipMemcpyAsync(w.pose.p, pose.data(), sizeof(float) * 12 * n, hipMemcpyHostToDevice, q));
  GLOC_HIP(hipStreamSynchronize(q));  // (pose is a host vector)
  p2l::Ctx g{};
  g.stream = q;
  g.prof = x.prof;
  g.ws = x.gn;
  g.srcs = rs.srcs.data();
  g.n_jobs = (uint32_t)n;
  g.pose_f32 = w.pose.as<float>();
  g.pose_stride = 12;
  g.nn_pass = nullptr;  // no search: the accumulate kernel finds its own pairs
  const gn6::Loop lp{prm->max_iters, prm->max_corr_dist, prm->trans_eps, prm->rot_eps, "vgicp_accum", "vgicp_solve"};
  const double a = 1.0 - (double)prm->plane_eps;
  const double gate2 = prm->max_corr_dist > 0.f ? (double)prm->max_corr_dist * (double)prm->max_corr_dist : 0.0;
  const float inv_res = 1.0f / prm->resolution;
  auto accum = [&](const Target* d_tgts, const gn6::Source* d_srcs, const gn6::State* states, float, bool skip_stopped, double* partials,
                   uint32_t n_blk, const gn6::Scale2& sc) {
    gn6::for_kind(c.kind(), [&](auto kind) {
      hipLaunchKernelGGL(HIP_KERNEL_NAME(vgicp_accum_kernel<decltype(kind)::value>), dim3(n_blk, g.n_jobs), dim3(gn6::ACC_THREADS), 0, q,
                         d_srcs, d_tgts, g.pose_f32, g.pose_stride, states, inv_res, prm->neighbors, gate2, a, skip_stopped, partials, sc);
    });
  };
  return gn6::run(g, lp, ht.data(), c, accum);
}

int voxels(const Ctx& x, uint32_t scan_id, const gloc_vgicp_params* prm, size_t capacity, int32_t* out_key3, uint32_t* out_count,
           double* out_mean3, double* out_nn6, size_t* n_voxels) {
  GLOC_TRY(check_params(prm));
  GLOC_REQUIRE(n_voxels, GLOC_ERR_INVALID, "n_voxels is null");
  GLOC_REQUIRE(x.store, GLOC_ERR_INVALID, "unknown scan id %u", scan_id);
  GLOC_TRY(ensure_ws(x.ws));
  Ws& w = **x.ws;
  const hipStream_t q = x.stream;
  GLOC_TRY(reg::store_ensure_normals(x.store, &scan_id, 1, prm->normal_k));
  reg::ScopedPins pins(x.store, q);
  GLOC_TRY(pins.pin(&scan_id, nullptr, 1));
  GLOC_REQUIRE(pins.scans[0].n == 0 || pins.scans[0].nrm, GLOC_ERR_STATE, "scan %u lost its normals during the call", scan_id);
  voxmap::Maps tm;
  {
    ProfScope ps(*x.prof, "vgicp_voxels", q);
    GLOC_TRY(target_voxels(q, w, pins.scans, prm, &tm));
  }
  GLOC_TRY(voxmap::export_valid<Voxel>(q, w.map, tm, capacity, out_key3, out_count, out_mean3, [&](const Voxel& c, size_t row) {
    if (out_nn6) std::copy(c.nn, c.nn + 6, out_nn6 + 6 * row);
  }, n_voxels));
  GLOC_REQUIRE(*n_voxels <= capacity || (!out_key3 && !out_count && !out_mean3 && !out_nn6), GLOC_ERR_INVALID,
               "buffers hold %zu voxels, the scan has %zu", capacity, *n_voxels);
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
