// iss.hip -- ISS keypoints of the resident scans (Intrinsic Shape Signatures, Zhong 2009; pcl::ISSKeypoint3D, Open3D's
// compute_iss_keypoints): host side of iss_kernels.hpp and the gloc_scan_store_* entries of I1 - I3 (include/gloc3d.h;
// tests/iss_ref.py is the contract).  The lists are ground::scan_lists' radius lists, the keypoints one more attribute a
// scan carries beside its normals and features (scan_features.hip); the entries that match on them are in reg.hip.
#include <cmath>
#include <vector>

#include "fpfh.hpp"
#include "iss_kernels.hpp"
#include "scan_store.hpp"

using namespace gloc;
using namespace gloc::iss;

static_assert(sizeof(gloc_iss_params) == 24, "gloc_iss_params is 24 bytes");
static_assert(ROW == (int)gloc::fpfh::FEAT_DIM, "one row layout");

namespace gloc {
namespace reg {

int check_iss_params(const gloc_iss_params* p) {
  GLOC_REQUIRE(p, GLOC_ERR_INVALID, "iss params is null");
  GLOC_TRY(check_support(Support::within(p->salient_radius, p->max_nn), SupportOf::SEARCH, SupportNames{nullptr, "salient_radius", "max_nn"}));
  GLOC_REQUIRE(p->min_nn >= 3 && p->min_nn <= p->max_nn, GLOC_ERR_INVALID, "min_nn = %u outside [3, max_nn = %u]", p->min_nn, p->max_nn);
  GLOC_REQUIRE(p->non_max_radius > 0.f && std::isfinite(p->non_max_radius), GLOC_ERR_INVALID, "non_max_radius = %g must be positive and finite",
               (double)p->non_max_radius);
  GLOC_REQUIRE(p->gamma_21 > 0.f && p->gamma_21 <= 1.f, GLOC_ERR_INVALID, "gamma_21 = %g outside (0, 1]", (double)p->gamma_21);
  GLOC_REQUIRE(p->gamma_32 > 0.f && p->gamma_32 <= 1.f, GLOC_ERR_INVALID, "gamma_32 = %g outside (0, 1]", (double)p->gamma_32);
  return GLOC_OK;
}

void store_drop_keypoint_rows(gloc_scan_store* st, DevScan& s) {
  if (!s.kp_feat) return;
  if (s.live) st->live_bytes -= 132 * s.kp_n;
  (void)hipFree(s.kp_feat);
  s.kp_feat = nullptr;
}

// I1 of a scan into st->iss_sal (and st->iss_eig when asked), original order; the lists and the chunk boxes of the sorted
// copy stay in st->nrm_ws for the suppression.  Enqueued on the store's stream.
static int store_saliency(gloc_scan_store* st, const DevScan& s, const gloc_iss_params& p, bool with_eig) {
  hipStream_t q = st->stream;
  const uint32_t n = (uint32_t)s.n;
  GLOC_TRY(st->iss_sal.ensure(sizeof(float) * s.n, q));
  if (with_eig) GLOC_TRY(st->iss_eig.ensure(sizeof(double) * 3 * s.n, q));
  GLOC_TRY(gloc::ground::scan_lists(q, st->nrm_ws, s.idx.pts, n, Support::within(p.salient_radius, p.max_nn)));
  hipLaunchKernelGGL(iss_saliency_kernel, dim3((n + 255) / 256), dim3(256), 0, q, st->nrm_ws.pts.as<f32x4>(), n, st->nrm_ws.knn_idx.as<uint32_t>(),
                     (int)p.max_nn, p.min_nn, p.gamma_21, p.gamma_32, st->iss_sal.as<float>(), with_eig ? st->iss_eig.as<double>() : nullptr);
  GLOC_HIP(hipGetLastError());
  return GLOC_OK;
}

// The table of the keypoints' feature rows, when the scan has keypoints and features and no table yet.
static int store_gather_keypoint_rows(gloc_scan_store* st, DevScan& s) {
  const bool features = s.fpfh && !s.fpfh_fsup.none() && s.nrm_sup == s.fpfh_nsup;
  if (!s.kp_built || s.kp_n == 0 || s.kp_feat || !features) return GLOC_OK;
  hipStream_t q = st->stream;
  GLOC_HIP(hipMalloc(reinterpret_cast<void**>(&s.kp_feat), 132 * s.kp_n));
  if (s.live) st->live_bytes += 132 * s.kp_n;
  const size_t e = s.kp_n * (size_t)ROW;
  hipLaunchKernelGGL(iss_gather_rows_kernel, dim3((unsigned)((e + 255) / 256)), dim3(256), 0, q, s.kp, (uint32_t)s.kp_n, (uint32_t)s.n, s.idx.inv,
                     s.fpfh, s.kp_feat);
  GLOC_HIP(hipGetLastError());
  GLOC_HIP(hipStreamSynchronize(q));
  return GLOC_OK;
}

int store_build_keypoints(gloc_scan_store* st, DevScan& s, const gloc_iss_params& prm) {
  GLOC_TRY(check_iss_params(&prm));
  if (s.has_keypoints(prm)) return store_gather_keypoint_rows(st, s);
  GLOC_REQUIRE(!s.kp_built || s.pins == 0, GLOC_ERR_STATE, "the scan's keypoints may be read by %d batch(es) in flight: not rebuilt", s.pins);
  store_drop_keypoint_rows(st, s);
  if (s.kp) {
    if (s.live) st->live_bytes -= 4 * s.kp_n;
    (void)hipFree(s.kp);
    s.kp = nullptr;
  }
  s.kp_n = 0;
  s.kp_built = false;
  if (s.n) {
    hipStream_t q = st->stream;
    const uint32_t n = (uint32_t)s.n, nch = (n + CHUNK - 1) / CHUNK;
    GLOC_TRY(st->iss_sal_sorted.ensure(sizeof(float) * s.n, q));
    GLOC_TRY(st->iss_flag.ensure(s.n, q));
    GLOC_TRY(st->iss_list.ensure(sizeof(uint32_t) * s.n, q));
    GLOC_TRY(st->iss_count.ensure(sizeof(uint32_t), q));
    GLOC_TRY(store_saliency(st, s, prm, false));
    GLOC_HIP(hipMemsetAsync(st->iss_flag.p, 0, s.n, q));
    hipLaunchKernelGGL(iss_sort_saliency_kernel, dim3((n + 255) / 256), dim3(256), 0, q, s.idx.pts, n, st->iss_sal.as<float>(),
                       st->iss_sal_sorted.as<float>());
    hipLaunchKernelGGL(iss_nms_kernel, dim3((nch + 3) / 4), dim3(256), 0, q, s.idx.pts, n, st->iss_sal_sorted.as<float>(),
                       st->nrm_ws.cbox_lo.as<f32x4>(), st->nrm_ws.cbox_hi.as<f32x4>(), nch, prm.non_max_radius * prm.non_max_radius,
                       st->iss_flag.as<uint8_t>());
    hipLaunchKernelGGL(iss_compact_kernel, dim3(1), dim3(1024), 0, q, st->iss_flag.as<uint8_t>(), n, st->iss_list.as<uint32_t>(),
                       st->iss_count.as<uint32_t>());
    GLOC_HIP(hipGetLastError());
    uint32_t K = 0;
    GLOC_HIP(hipMemcpyAsync(&K, st->iss_count.p, sizeof(K), hipMemcpyDeviceToHost, q));
    GLOC_HIP(hipStreamSynchronize(q));
    GLOC_REQUIRE(K <= n, GLOC_ERR_STATE, "%u keypoints of %u points", K, n);
    if (K) {
      GLOC_HIP(hipMalloc(reinterpret_cast<void**>(&s.kp), sizeof(uint32_t) * K));
      s.kp_n = K;
      if (s.live) st->live_bytes += 4 * s.kp_n;
      GLOC_HIP(hipMemcpyAsync(s.kp, st->iss_list.p, sizeof(uint32_t) * K, hipMemcpyDeviceToDevice, q));
      GLOC_HIP(hipStreamSynchronize(q));
    }
  }
  s.kp_prm = prm;  // (only now: a failure above leaves "no keypoints")
  s.kp_built = true;
  return store_gather_keypoint_rows(st, s);
}

int store_ensure_keypoints(gloc_scan_store* st, const uint32_t* ids, size_t n, const gloc_iss_params& prm) {
  std::lock_guard<std::mutex> lk(st->mu);
  for (size_t c = 0; c < n; ++c) {
    GLOC_REQUIRE(ids[c] < st->scans.size() && st->scans[ids[c]].live, GLOC_ERR_INVALID, "unknown scan id %u", ids[c]);
    GLOC_TRY(store_build_keypoints(st, st->scans[ids[c]], prm));
  }
  return GLOC_OK;
}

}  // namespace reg
}  // namespace gloc

using namespace gloc::reg;

namespace {

template <class F>
int on_scan(gloc_scan_store* st, uint32_t scan_id, F&& f) {
  GLOC_HIP(hipSetDevice(st->device));
  std::lock_guard<std::mutex> lk(st->mu);
  GLOC_REQUIRE(scan_id < st->scans.size() && st->scans[scan_id].live, GLOC_ERR_INVALID, "unknown scan id %u", scan_id);
  return f(st->scans[scan_id]);
}

}  // namespace

// ---- C ABI (the parameters are looked at before the handle) ---------------------------------------------------------------
extern "C" {

void gloc_iss_default_params(gloc_iss_params* p) {
  if (!p) return;
  p->salient_radius = 3.0f;  // 6 x the 0.5 m leaf the stage runs behind (Open3D's default: 6 x the resolution)
  p->max_nn = 128;
  p->min_nn = 5;
  p->non_max_radius = 2.0f;  // 4 x the leaf
  p->gamma_21 = 0.975f;
  p->gamma_32 = 0.975f;
}

int gloc_scan_store_iss_saliency(gloc_scan_store* st, uint32_t scan_id, const gloc_iss_params* prm, float* out_saliency, double* out_eig,
                                 size_t capacity_points) {
  GLOC_TRY(check_iss_params(prm));
  GLOC_REQUIRE(st, GLOC_ERR_INVALID, "null store");
  return on_scan(st, scan_id, [&](const DevScan& s) -> int {
    GLOC_REQUIRE(capacity_points >= s.n, GLOC_ERR_INVALID, "buffers hold %zu points, the scan has %zu", capacity_points, s.n);
    if (s.n == 0) return GLOC_OK;
    hipStream_t q = st->stream;
    GLOC_TRY(store_saliency(st, s, *prm, out_eig != nullptr));
    if (out_saliency) GLOC_HIP(hipMemcpyAsync(out_saliency, st->iss_sal.p, sizeof(float) * s.n, hipMemcpyDeviceToHost, q));
    if (out_eig) GLOC_HIP(hipMemcpyAsync(out_eig, st->iss_eig.p, sizeof(double) * 3 * s.n, hipMemcpyDeviceToHost, q));
    GLOC_HIP(hipStreamSynchronize(q));
    return GLOC_OK;
  });
}

int gloc_scan_store_build_keypoints(gloc_scan_store* st, uint32_t scan_id, const gloc_iss_params* prm) {
  GLOC_TRY(check_iss_params(prm));
  GLOC_REQUIRE(st, GLOC_ERR_INVALID, "null store");
  return on_scan(st, scan_id, [&](DevScan& s) -> int { return store_build_keypoints(st, s, *prm); });
}

int gloc_scan_store_keypoint_count(gloc_scan_store* st, uint32_t scan_id, size_t* out_k) {
  GLOC_REQUIRE(st && out_k, GLOC_ERR_INVALID, "null argument");
  return on_scan(st, scan_id, [&](const DevScan& s) -> int {
    GLOC_REQUIRE(s.kp_built, GLOC_ERR_STATE, "scan %u has no keypoints: call gloc_scan_store_build_keypoints first", scan_id);
    *out_k = s.kp_n;
    return GLOC_OK;
  });
}

int gloc_scan_store_keypoints(gloc_scan_store* st, uint32_t scan_id, uint32_t* out_idx, size_t capacity) {
  GLOC_REQUIRE(st && (out_idx || capacity == 0), GLOC_ERR_INVALID, "null argument");
  return on_scan(st, scan_id, [&](const DevScan& s) -> int {
    GLOC_REQUIRE(s.kp_built, GLOC_ERR_STATE, "scan %u has no keypoints: call gloc_scan_store_build_keypoints first", scan_id);
    GLOC_REQUIRE(capacity >= s.kp_n, GLOC_ERR_INVALID, "buffer holds %zu indices, the scan has %zu keypoints", capacity, s.kp_n);
    if (s.kp_n == 0) return GLOC_OK;
    GLOC_HIP(hipMemcpyAsync(out_idx, s.kp, sizeof(uint32_t) * s.kp_n, hipMemcpyDeviceToHost, st->stream));
    GLOC_HIP(hipStreamSynchronize(st->stream));
    return GLOC_OK;
  });
}

int gloc_scan_store_keypoint_fpfh(gloc_scan_store* st, uint32_t scan_id, float* out_feat, size_t capacity) {
  GLOC_REQUIRE(st && (out_feat || capacity == 0), GLOC_ERR_INVALID, "null argument");
  return on_scan(st, scan_id, [&](DevScan& s) -> int {
    GLOC_REQUIRE(s.kp_built, GLOC_ERR_STATE, "scan %u has no keypoints: call gloc_scan_store_build_keypoints first", scan_id);
    GLOC_REQUIRE(s.n == 0 || (!s.fpfh_fsup.none() && s.nrm_sup == s.fpfh_nsup), GLOC_ERR_STATE,
                 "scan %u has no features: call gloc_scan_store_build_fpfh first", scan_id);
    GLOC_REQUIRE(capacity >= s.kp_n, GLOC_ERR_INVALID, "buffer holds %zu rows, the scan has %zu keypoints", capacity, s.kp_n);
    if (s.kp_n == 0) return GLOC_OK;
    GLOC_TRY(store_gather_keypoint_rows(st, s));
    GLOC_REQUIRE(s.kp_feat, GLOC_ERR_STATE, "scan %u has no features: call gloc_scan_store_build_fpfh first", scan_id);
    GLOC_HIP(hipMemcpyAsync(out_feat, s.kp_feat, 132 * s.kp_n, hipMemcpyDeviceToHost, st->stream));
    GLOC_HIP(hipStreamSynchronize(st->stream));
    return GLOC_OK;
  });
}

}  // extern "C"
