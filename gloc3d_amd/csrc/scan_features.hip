// scan_features.hip -- the per-scan attributes of the resident scan store (scan_store.hpp): per-point normals and FPFH
// features, each an optional allocation beside a scan's block, built on the store's stream from one neighbourhood Support
// (ground_normals.hpp) -- the k nearest points or the points within a radius -- and tagged with it.  The builders, the
// store_ensure_* the registration handles call, and the gloc_scan_store_* entries that build and download them
// (include/gloc3d.h).  Indexing the scans, and re-ordering these attributes when a re-sort moves the points, is
// scan_store.hip's.
#include <string>

#include "fpfh.hpp"
#include "scan_store.hpp"

namespace gloc {
namespace reg {

// normals between original order and the order of the sorted points (pts[i].w = original index of sorted position i)
__global__ __launch_bounds__(256) void normals_reorder_kernel(const f32x4* __restrict__ pts, uint32_t n, const float* __restrict__ in,
                                                              float* __restrict__ out, bool to_sorted) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t o = __float_as_uint(pts[i].w);
  if (o >= n) return;
  const size_t src = 3 * (size_t)(to_sorted ? o : i), dst = 3 * (size_t)(to_sorted ? i : o);
  out[dst + 0] = in[src + 0];
  out[dst + 1] = in[src + 1];
  out[dst + 2] = in[src + 2];
}

int store_reorder_normals(hipStream_t q, const f32x4* pts, uint32_t n, const float* in, float* out, bool to_sorted) {
  hipLaunchKernelGGL(normals_reorder_kernel, dim3((n + 255) / 256), dim3(256), 0, q, pts, n, in, out, to_sorted);
  GLOC_HIP(hipGetLastError());
  return GLOC_OK;
}

static std::string describe(const Support& s) {
  char buf[96];
  if (s.by_radius())
    snprintf(buf, sizeof(buf), "radius = %g, max_nn = %u, min_nn = %u", (double)s.r, s.max_nn, s.min_nn);
  else
    snprintf(buf, sizeof(buf), "k = %u", s.k);
  return buf;
}

int store_build_normals(gloc_scan_store* st, DevScan& s, const Support& ns) {
  GLOC_TRY(check_support(ns, SupportOf::NORMALS, SupportNames{"k", "radius", "max_nn", "min_nn"}));
  if (s.has_normals(ns) || s.n == 0) {
    s.nrm_sup = ns;
    return GLOC_OK;
  }
  GLOC_REQUIRE(!s.nrm || s.pins == 0, GLOC_ERR_STATE, "the scan's normals (%s) may be read by %d batch(es) in flight: not rebuilt with %s",
               describe(s.nrm_sup).c_str(), s.pins, describe(ns).c_str());
  hipStream_t q = st->stream;
  const uint32_t n = (uint32_t)s.n;
  if (!s.nrm) {
    GLOC_HIP(hipMalloc(reinterpret_cast<void**>(&s.nrm), 12 * s.n));
    if (s.live) st->live_bytes += 12 * s.n;
  }
  s.nrm_sup = Support{};
  s.fpfh_nsup = s.fpfh_fsup = Support{};  // (features of the old normals: rebuilt on the next request)
  store_drop_keypoint_rows(st, s);        // (and the keypoints' rows gathered from them)
  GLOC_TRY(st->nrm_tmp.ensure(12 * s.n, q));
  GLOC_TRY(gloc::ground::scan_normals(q, st->nrm_ws, s.idx.pts, n, ns, st->nrm_tmp.as<float>()));
  GLOC_TRY(store_reorder_normals(q, s.idx.pts, n, st->nrm_tmp.as<float>(), s.nrm, true));
  GLOC_HIP(hipStreamSynchronize(q));
  s.nrm_sup = ns;
  return GLOC_OK;
}

// SPFH of a scan with normals over the lists of fs into st->spfh_tmp (original order); the lists stay in st->nrm_ws for
// build_fpfh.
static int store_spfh(gloc_scan_store* st, const DevScan& s, const Support& fs) {
  hipStream_t q = st->stream;
  const uint32_t n = (uint32_t)s.n;
  GLOC_TRY(st->nrm_tmp.ensure(12 * s.n, q));
  GLOC_TRY(st->spfh_tmp.ensure((size_t)gloc::fpfh::SPFH_BYTES * s.n, q));
  GLOC_TRY(store_reorder_normals(q, s.idx.pts, n, s.nrm, st->nrm_tmp.as<float>(), false));
  return gloc::fpfh::build_spfh(q, st->nrm_ws, s.idx.pts, st->nrm_tmp.as<float>(), n, fs, st->spfh_tmp.as<uint8_t>());
}

int store_build_fpfh(gloc_scan_store* st, DevScan& s, const Support& ns, const Support& fs) {
  GLOC_TRY(check_support(ns, SupportOf::NORMALS, SupportNames{"normal_k", "normal_radius", "normal_max_nn", "normal_min_nn"}));
  GLOC_TRY(check_support(fs, SupportOf::FEATURES, SupportNames{"feature_k", "feature_radius", "feature_max_nn"}));
  if (s.n == 0) {
    s.nrm_sup = s.fpfh_nsup = ns;
    s.fpfh_fsup = fs;
    return GLOC_OK;
  }
  if (s.has_fpfh(ns, fs)) return GLOC_OK;
  GLOC_REQUIRE(!s.fpfh || s.pins == 0, GLOC_ERR_STATE,
               "the scan's features (normals: %s; features: %s) may be read by %d batch(es) in flight: not rebuilt with %s; %s",
               describe(s.fpfh_nsup).c_str(), describe(s.fpfh_fsup).c_str(), s.pins, describe(ns).c_str(), describe(fs).c_str());
  GLOC_TRY(store_build_normals(st, s, ns));
  hipStream_t q = st->stream;
  const uint32_t n = (uint32_t)s.n;
  if (!s.fpfh) {
    GLOC_HIP(hipMalloc(reinterpret_cast<void**>(&s.fpfh), 132 * s.n));
    if (s.live) st->live_bytes += 132 * s.n;
  }
  s.fpfh_nsup = s.fpfh_fsup = Support{};
  store_drop_keypoint_rows(st, s);  // (gathered from the old features; the next keypoint request gathers from the new)
  GLOC_TRY(st->fpfh_tmp.ensure(132 * s.n, q));
  GLOC_TRY(store_spfh(st, s, fs));
  GLOC_TRY(gloc::fpfh::build_fpfh(q, st->nrm_ws, st->spfh_tmp.as<uint8_t>(), n, fs, st->fpfh_tmp.as<float>()));
  GLOC_TRY(gloc::fpfh::reorder_rows(q, s.idx.pts, n, st->fpfh_tmp.as<float>(), s.fpfh, gloc::fpfh::FEAT_DIM, true));
  GLOC_HIP(hipStreamSynchronize(q));
  s.fpfh_nsup = ns;  // (only now: a failure above leaves "no features", not stale tags)
  s.fpfh_fsup = fs;
  return GLOC_OK;
}

int store_ensure_normals(gloc_scan_store* st, const uint32_t* ids, size_t n, uint32_t k) {
  std::lock_guard<std::mutex> lk(st->mu);
  for (size_t c = 0; c < n; ++c) {
    GLOC_REQUIRE(ids[c] < st->scans.size() && st->scans[ids[c]].live, GLOC_ERR_INVALID, "unknown scan id %u", ids[c]);
    DevScan& s = st->scans[ids[c]];
    if (s.nrm_sup.none()) GLOC_TRY(store_build_normals(st, s, Support::nearest(k)));
  }
  return GLOC_OK;
}

int store_ensure_fpfh(gloc_scan_store* st, const uint32_t* ids, size_t n, const Support& ns, const Support& fs) {
  std::lock_guard<std::mutex> lk(st->mu);
  for (size_t c = 0; c < n; ++c) {
    GLOC_REQUIRE(ids[c] < st->scans.size() && st->scans[ids[c]].live, GLOC_ERR_INVALID, "unknown scan id %u", ids[c]);
    GLOC_TRY(store_build_fpfh(st, st->scans[ids[c]], ns, fs));
  }
  return GLOC_OK;
}

}  // namespace reg
}  // namespace gloc

using namespace gloc;
using namespace gloc::reg;

namespace {

// What every entry below does once its arguments have passed: the store's device current, the store locked, the scan found.
template <class F>
int on_scan(gloc_scan_store* st, uint32_t scan_id, F&& f) {
  GLOC_HIP(hipSetDevice(st->device));
  std::lock_guard<std::mutex> lk(st->mu);
  GLOC_REQUIRE(scan_id < st->scans.size() && st->scans[scan_id].live, GLOC_ERR_INVALID, "unknown scan id %u", scan_id);
  return f(st->scans[scan_id]);
}

// gloc_scan_store_spfh / _spfh_radius behind their checks: the SPFH of fs from the scan's normals, unpacked for the host.
int download_spfh(gloc_scan_store* st, uint32_t scan_id, const DevScan& s, const Support& fs, uint16_t* out_counts, uint32_t* out_used,
                  size_t capacity_points) {
  GLOC_REQUIRE(!s.nrm_sup.none(), GLOC_ERR_STATE, "scan %u has no normals: call gloc_scan_store_build_normals%s first", scan_id,
               fs.by_radius() ? "_radius" : "");
  GLOC_REQUIRE(capacity_points >= s.n, GLOC_ERR_INVALID, "buffer holds %zu points, the scan has %zu", capacity_points, s.n);
  if (s.n == 0) return GLOC_OK;
  GLOC_TRY(store_spfh(st, s, fs));
  std::vector<uint8_t> raw((size_t)gloc::fpfh::SPFH_BYTES * s.n);
  GLOC_HIP(hipMemcpyAsync(raw.data(), st->spfh_tmp.p, raw.size(), hipMemcpyDeviceToHost, st->stream));
  GLOC_HIP(hipStreamSynchronize(st->stream));
  for (size_t i = 0; i < s.n; ++i) {
    for (uint32_t b = 0; b < gloc::fpfh::FEAT_DIM; ++b) out_counts[i * gloc::fpfh::FEAT_DIM + b] = raw[i * gloc::fpfh::SPFH_BYTES + b];
    out_used[i] = raw[i * gloc::fpfh::SPFH_BYTES + gloc::fpfh::FEAT_DIM];
  }
  return GLOC_OK;
}

}  // namespace

// ---- C ABI (the parameters are looked at before the handle) ---------------------------------------------------------------
extern "C" {

int gloc_scan_store_build_normals(gloc_scan_store* st, uint32_t scan_id, uint32_t k) {
  const Support ns = Support::nearest(k);
  GLOC_TRY(check_support(ns, SupportOf::NORMALS, SupportNames{"k"}));
  GLOC_REQUIRE(st, GLOC_ERR_INVALID, "null store");
  return on_scan(st, scan_id, [&](DevScan& s) -> int { return store_build_normals(st, s, ns); });
}

int gloc_scan_store_build_normals_radius(gloc_scan_store* st, uint32_t scan_id, float radius, uint32_t max_nn, uint32_t min_nn) {
  const Support ns = Support::within(radius, max_nn, min_nn);
  GLOC_TRY(check_support(ns, SupportOf::NORMALS, SupportNames{nullptr, "radius", "max_nn", "min_nn"}));
  GLOC_REQUIRE(st, GLOC_ERR_INVALID, "null store");
  return on_scan(st, scan_id, [&](DevScan& s) -> int { return store_build_normals(st, s, ns); });
}

int gloc_scan_store_normals(gloc_scan_store* st, uint32_t scan_id, float* out_nxyz, size_t capacity_points) {
  GLOC_REQUIRE(st && out_nxyz, GLOC_ERR_INVALID, "null argument");
  return on_scan(st, scan_id, [&](const DevScan& s) -> int {
    GLOC_REQUIRE(!s.nrm_sup.none(), GLOC_ERR_STATE, "scan %u has no normals: call gloc_scan_store_build_normals first", scan_id);
    GLOC_REQUIRE(capacity_points >= s.n, GLOC_ERR_INVALID, "buffer holds %zu points, the scan has %zu", capacity_points, s.n);
    if (s.n == 0) return GLOC_OK;
    hipStream_t q = st->stream;
    GLOC_TRY(st->nrm_tmp.ensure(12 * s.n, q));
    GLOC_TRY(store_reorder_normals(q, s.idx.pts, (uint32_t)s.n, s.nrm, st->nrm_tmp.as<float>(), false));
    GLOC_HIP(hipMemcpyAsync(out_nxyz, st->nrm_tmp.p, 12 * s.n, hipMemcpyDeviceToHost, q));
    GLOC_HIP(hipStreamSynchronize(q));
    return GLOC_OK;
  });
}

int gloc_scan_store_build_fpfh(gloc_scan_store* st, uint32_t scan_id, uint32_t normal_k, uint32_t feature_k) {
  const Support ns = Support::nearest(normal_k), fs = Support::nearest(feature_k);
  GLOC_TRY(check_support(ns, SupportOf::NORMALS, SupportNames{"normal_k"}));
  GLOC_TRY(check_support(fs, SupportOf::FEATURES, SupportNames{"feature_k"}));
  GLOC_REQUIRE(st, GLOC_ERR_INVALID, "null store");
  return on_scan(st, scan_id, [&](DevScan& s) -> int { return store_build_fpfh(st, s, ns, fs); });
}

int gloc_scan_store_build_fpfh_radius(gloc_scan_store* st, uint32_t scan_id, const gloc_fpfh_radius_params* prm) {
  GLOC_TRY(gloc::fpfh::check_radius_params(prm));
  GLOC_REQUIRE(st, GLOC_ERR_INVALID, "null store");
  return on_scan(st, scan_id, [&](DevScan& s) -> int { return store_build_fpfh(st, s, Support::normals_of(*prm), Support::features_of(*prm)); });
}

int gloc_scan_store_fpfh(gloc_scan_store* st, uint32_t scan_id, float* out_feat, size_t capacity_points) {
  GLOC_REQUIRE(st && out_feat, GLOC_ERR_INVALID, "null argument");
  return on_scan(st, scan_id, [&](const DevScan& s) -> int {
    GLOC_REQUIRE(!s.fpfh_fsup.none(), GLOC_ERR_STATE, "scan %u has no features: call gloc_scan_store_build_fpfh first", scan_id);
    GLOC_REQUIRE(capacity_points >= s.n, GLOC_ERR_INVALID, "buffer holds %zu points, the scan has %zu", capacity_points, s.n);
    if (s.n == 0) return GLOC_OK;
    hipStream_t q = st->stream;
    GLOC_TRY(st->fpfh_tmp.ensure(132 * s.n, q));
    GLOC_TRY(gloc::fpfh::reorder_rows(q, s.idx.pts, (uint32_t)s.n, s.fpfh, st->fpfh_tmp.as<float>(), gloc::fpfh::FEAT_DIM, false));
    GLOC_HIP(hipMemcpyAsync(out_feat, st->fpfh_tmp.p, 132 * s.n, hipMemcpyDeviceToHost, q));
    GLOC_HIP(hipStreamSynchronize(q));
    return GLOC_OK;
  });
}

int gloc_scan_store_spfh(gloc_scan_store* st, uint32_t scan_id, uint32_t feature_k, uint16_t* out_counts, uint32_t* out_used,
                         size_t capacity_points) {
  const Support fs = Support::nearest(feature_k);
  GLOC_TRY(check_support(fs, SupportOf::FEATURES, SupportNames{"feature_k"}));
  GLOC_REQUIRE(st && out_counts && out_used, GLOC_ERR_INVALID, "null argument");
  return on_scan(st, scan_id, [&](const DevScan& s) -> int { return download_spfh(st, scan_id, s, fs, out_counts, out_used, capacity_points); });
}

int gloc_scan_store_spfh_radius(gloc_scan_store* st, uint32_t scan_id, float radius, uint32_t max_nn, uint16_t* out_counts,
                                uint32_t* out_used, size_t capacity_points) {
  const Support fs = Support::within(radius, max_nn);
  GLOC_TRY(check_support(fs, SupportOf::FEATURES, SupportNames{nullptr, "radius", "max_nn"}));
  GLOC_REQUIRE(st && out_counts && out_used, GLOC_ERR_INVALID, "null argument");
  return on_scan(st, scan_id, [&](const DevScan& s) -> int { return download_spfh(st, scan_id, s, fs, out_counts, out_used, capacity_points); });
}

int gloc_scan_store_radius_neighbors(gloc_scan_store* st, uint32_t scan_id, float radius, uint32_t max_nn, uint32_t* out_idx, float* out_d2,
                                     uint32_t* out_count, size_t capacity_points) {
  const Support sup = Support::within(radius, max_nn);
  GLOC_TRY(check_support(sup, SupportOf::SEARCH, SupportNames{nullptr, "radius", "max_nn"}));
  GLOC_REQUIRE(st, GLOC_ERR_INVALID, "null store");
  return on_scan(st, scan_id, [&](const DevScan& s) -> int {
    GLOC_REQUIRE(capacity_points >= s.n, GLOC_ERR_INVALID, "buffers hold %zu points, the scan has %zu", capacity_points, s.n);
    if (s.n == 0) return GLOC_OK;
    hipStream_t q = st->stream;
    GLOC_TRY(gloc::ground::scan_lists(q, st->nrm_ws, s.idx.pts, (uint32_t)s.n, sup));
    const size_t e = s.n * (size_t)max_nn;
    if (out_idx) GLOC_HIP(hipMemcpyAsync(out_idx, st->nrm_ws.knn_idx.p, sizeof(uint32_t) * e, hipMemcpyDeviceToHost, q));
    if (out_d2) GLOC_HIP(hipMemcpyAsync(out_d2, st->nrm_ws.knn_d2.p, sizeof(float) * e, hipMemcpyDeviceToHost, q));
    if (out_count) GLOC_HIP(hipMemcpyAsync(out_count, st->nrm_ws.knn_cnt.p, sizeof(uint32_t) * s.n, hipMemcpyDeviceToHost, q));
    GLOC_HIP(hipStreamSynchronize(q));
    return GLOC_OK;
  });
}

}  // extern "C"
