// m2dp.hip -- C ABI of the M2DP place descriptor (include/gloc3d.h, gloc_m2dp_*): a training-free descriptor that is a
// plain L2 vector, built from resident or host scans, and the PCA frame it is built in.  No counterpart in the reference;
// the contract is stated in the header and restated in numpy by tests/m2dp_ref.py.
#include <algorithm>
#include <cmath>
#include <vector>

#include "common.hpp"
#include "m2dp_kernels.hpp"
#include "scan_store.hpp"

using namespace gloc;
using namespace gloc::m2dp;

struct gloc_m2dp : Handle {
  gloc_m2dp_params prm{};
  int P = 0, L = 0, T = 0, B = 0;  // planes, rings, sectors, bins per plane
  float max_range2 = 0.f;
  bool tab_up = false;
  Tables h_tables{};
  DevBuf tables, stage_pts, scan_tab, info, part, counts, n_used, frames, desc, sigma;
  std::vector<ScanRef> h_tab;
  size_t dim() const { return (size_t)P + B; }
};

namespace {

int check_params(const gloc_m2dp_params* p) {
  GLOC_REQUIRE(p, GLOC_ERR_INVALID, "params is NULL");
  GLOC_REQUIRE(p->n_azimuth >= 1 && p->n_elevation >= 1 && (uint64_t)p->n_azimuth * p->n_elevation <= (uint64_t)MAX_PLANES,
               GLOC_ERR_INVALID, "n_azimuth x n_elevation = %u x %u: each >= 1, at most %d planes", p->n_azimuth,
               p->n_elevation, MAX_PLANES);
  GLOC_REQUIRE(p->n_rings >= 1 && p->n_sectors >= 2 && (uint64_t)p->n_rings * p->n_sectors <= (uint64_t)MAX_BINS,
               GLOC_ERR_INVALID, "n_rings x n_sectors = %u x %u: rings >= 1, sectors >= 2, at most %d bins", p->n_rings,
               p->n_sectors, MAX_BINS);
  GLOC_REQUIRE(std::isfinite(p->max_range) && p->max_range > 0.f, GLOC_ERR_INVALID, "max_range must be finite and positive");
  GLOC_REQUIRE(p->min_points >= 4, GLOC_ERR_INVALID, "min_points = %u: at least 4", p->min_points);
  GLOC_REQUIRE(p->reserved_ == 0, GLOC_ERR_INVALID, "reserved_ must be 0");
  return GLOC_OK;
}

// the unit pairs of the planes, the ring thresholds and the sector borders, in fp64
void make_tables(const gloc_m2dp_params& p, Tables* t) {
  memset(t, 0, sizeof(*t));
  for (uint32_t a = 0; a < p.n_azimuth; ++a)
    for (uint32_t b = 0; b < p.n_elevation; ++b) {
      const double th = -M_PI / 2 + (double)a * M_PI / (double)p.n_azimuth, ph = (double)b * (M_PI / 2) / (double)p.n_elevation;
      double* u = t->u[a * p.n_elevation + b];
      double* v = t->v[a * p.n_elevation + b];
      u[0] = -sin(th), u[1] = cos(th), u[2] = 0.0;
      v[0] = -sin(ph) * cos(th), v[1] = -sin(ph) * sin(th), v[2] = cos(ph);
    }
  for (uint32_t k = 0; k < p.n_rings; ++k) {
    const double f = (double)k / (double)p.n_rings;
    t->ring_thr[k] = (f * f) * (f * f);
  }
  for (uint32_t k = 0; k < p.n_sectors; ++k) {
    const double a = 2.0 * M_PI * (double)k / (double)p.n_sectors;
    t->sec_cos[k] = cos(a), t->sec_sin[k] = sin(a);
  }
}

int check_store(const gloc_m2dp* h, const gloc_scan_store* store, const uint32_t* scan_ids, size_t n) {
  GLOC_REQUIRE(h && store && (n == 0 || scan_ids), GLOC_ERR_INVALID, "null argument");
  GLOC_REQUIRE(store->device == h->device, GLOC_ERR_INVALID, "store on device %d, descriptor handle on %d", store->device,
               h->device);
  GLOC_REQUIRE(n <= 4096, GLOC_ERR_INVALID, "at most 4096 scans per call (%zu)", n);
  return GLOC_OK;
}

int ensure_outputs(gloc_m2dp* h, size_t count) {
  hipStream_t s = h->stream;
  GLOC_TRY(h->counts.ensure(sizeof(uint32_t) * h->P * h->B * count, s));
  GLOC_TRY(h->n_used.ensure(sizeof(uint32_t) * count, s));
  GLOC_TRY(h->desc.ensure(sizeof(float) * h->dim() * count, s));
  GLOC_TRY(h->sigma.ensure(sizeof(double) * 2 * count, s));
  if (!h->tab_up) {
    GLOC_TRY(h->tables.ensure(sizeof(Tables), s));
    GLOC_HIP(hipMemcpyAsync(h->tables.p, &h->h_tables, sizeof(Tables), hipMemcpyHostToDevice, s));
    h->tab_up = true;
  }
  return GLOC_OK;
}

int launch_svd(gloc_m2dp* h, size_t count, float* d_desc, double* d_sigma) {
  ProfScope ps(h->prof, "m2dp_svd", h->stream);
  hipLaunchKernelGGL(svd_kernel, dim3((unsigned)count), dim3(128), 0, h->stream, h->counts.as<uint32_t>(),
                     h->n_used.as<uint32_t>(), h->P, h->B, d_desc, d_sigma);
  GLOC_HIP(hipGetLastError());
  return GLOC_OK;
}

// The scans of h->h_tab -> h->frames [count][12], h->counts [count][P][B], d_desc [count][dim].  Eight launches whatever
// the number of scans.
int describe_tab(gloc_m2dp* h, float* d_desc) {
  hipStream_t s = h->stream;
  const size_t count = h->h_tab.size();
  uint32_t most = 0;
  for (const ScanRef& r : h->h_tab) most = std::max(most, r.n);
  const uint32_t nb = std::max<uint32_t>(1, (most + SLICE - 1) / SLICE);
  GLOC_TRY(ensure_outputs(h, count));
  GLOC_TRY(h->scan_tab.ensure(sizeof(ScanRef) * count, s));
  GLOC_TRY(h->info.ensure(sizeof(Info) * count, s));
  GLOC_TRY(h->frames.ensure(sizeof(double) * 12 * count, s));
  GLOC_TRY(h->part.ensure(sizeof(double) * PART_W * nb * count, s));
  GLOC_HIP(hipMemcpyAsync(h->scan_tab.p, h->h_tab.data(), sizeof(ScanRef) * count, hipMemcpyHostToDevice, s));
  GLOC_HIP(hipMemsetAsync(h->counts.p, 0, sizeof(uint32_t) * h->P * h->B * count, s));
  const ScanRef* tab = h->scan_tab.as<ScanRef>();
  Info* info = h->info.as<Info>();
  double* part = h->part.as<double>();
  {
    ProfScope ps(h->prof, "m2dp_frame", s);
    const dim3 grid(nb, (unsigned)count), one((unsigned)count);
#define GLOC_M2DP_STAGE(S_)                                                                                            \
  hipLaunchKernelGGL(moments_kernel<S_>, grid, dim3(256), 0, s, tab, h->max_range2, info, part, nb);                   \
  hipLaunchKernelGGL(combine_kernel<S_>, one, dim3(256), 0, s, tab, part, nb, h->prm.min_points, info,                 \
                     h->frames.as<double>(), h->n_used.as<uint32_t>());
    GLOC_M2DP_STAGE(0) GLOC_M2DP_STAGE(1) GLOC_M2DP_STAGE(2)
#undef GLOC_M2DP_STAGE
    GLOC_HIP(hipGetLastError());
  }
  {
    ProfScope ps(h->prof, "m2dp_project", s);
    // the largest chunk that still gives the batch ~4 blocks per compute unit; a scan's counts do not depend on it
    uint32_t chunk = MAX_CHUNK;
    while (chunk > 1024 && (size_t)((most + chunk - 1) / chunk) * count < 1024) chunk >>= 1;
    const dim3 grid(std::max<uint32_t>(1, (most + chunk - 1) / chunk), (unsigned)count);
    hipLaunchKernelGGL(project_kernel, grid, dim3(64 * PROJ_WAVES), 0, s, tab, info, h->tables.as<Tables>(), h->P, h->L, h->T,
                       h->max_range2, chunk, h->counts.as<uint32_t>());
    GLOC_HIP(hipGetLastError());
  }
  return launch_svd(h, count, d_desc, nullptr);
}

int download(gloc_m2dp* h, size_t count, float* out_desc, double* out_frame12, uint32_t* out_counts) {
  hipStream_t s = h->stream;
  GLOC_HIP(hipMemcpyAsync(out_desc, h->desc.p, sizeof(float) * h->dim() * count, hipMemcpyDeviceToHost, s));
  if (out_frame12) GLOC_HIP(hipMemcpyAsync(out_frame12, h->frames.p, sizeof(double) * 12 * count, hipMemcpyDeviceToHost, s));
  if (out_counts)
    GLOC_HIP(hipMemcpyAsync(out_counts, h->counts.p, sizeof(uint32_t) * h->P * h->B * count, hipMemcpyDeviceToHost, s));
  GLOC_HIP(hipStreamSynchronize(s));
  return GLOC_OK;
}

int pin_scans(gloc_m2dp* h, reg::ScopedPins& pins, const uint32_t* scan_ids, size_t n) {
  GLOC_TRY(pins.pin(scan_ids, nullptr, n));
  h->h_tab.clear();
  for (const DevScan& sc : pins.scans) {
    GLOC_REQUIRE(sc.n < (1ull << 31), GLOC_ERR_INVALID, "scan too large");
    h->h_tab.push_back(ScanRef{sc.xyz, (uint32_t)sc.n, 3u});  // the original-order points: nothing depends on an index
  }
  return GLOC_OK;
}

}  // namespace

extern "C" {

int gloc_m2dp_default_params(gloc_m2dp_params* p) {
  GLOC_REQUIRE(p, GLOC_ERR_INVALID, "params is NULL");
  p->n_azimuth = 4;  // He, Wang & Zhang, IROS 2016: 4 x 16 planes, 8 rings x 16 sectors
  p->n_elevation = 16;
  p->n_rings = 8;
  p->n_sectors = 16;
  p->max_range = 80.f;
  p->min_points = 16;
  p->reserved_ = 0;
  return GLOC_OK;
}

int gloc_m2dp_dim(const gloc_m2dp_params* params, size_t* dim) {
  GLOC_REQUIRE(dim, GLOC_ERR_INVALID, "null argument");
  GLOC_TRY(check_params(params));
  *dim = (size_t)params->n_azimuth * params->n_elevation + (size_t)params->n_rings * params->n_sectors;
  return GLOC_OK;
}

int gloc_m2dp_create(int device, const gloc_m2dp_params* params, gloc_m2dp** out) {
  GLOC_REQUIRE(out, GLOC_ERR_INVALID, "out is NULL");
  *out = nullptr;
  GLOC_TRY(check_params(params));  // (before the device is looked at: a bad block is refused on any machine)
  GLOC_TRY(create_handle(device, out));
  gloc_m2dp* h = *out;
  h->prm = *params;
  h->P = (int)(params->n_azimuth * params->n_elevation);
  h->L = (int)params->n_rings, h->T = (int)params->n_sectors, h->B = h->L * h->T;
  h->max_range2 = params->max_range * params->max_range;
  make_tables(h->prm, &h->h_tables);
  return GLOC_OK;
}

int gloc_m2dp_destroy(gloc_m2dp* h) { return destroy_handle(h); }

int gloc_m2dp_set_stream(gloc_m2dp* h, void* hip_stream) { return handle_set_stream(h, hip_stream); }

int gloc_m2dp_synchronize(gloc_m2dp* h) { return handle_synchronize(h); }

int gloc_m2dp_set_profile(gloc_m2dp* h, int enable) { return handle_set_profile(h, enable); }

int gloc_m2dp_profile(gloc_m2dp* h, const char* kernel, double* total_ms, uint64_t* launches) {
  return handle_profile(h, kernel, total_ms, launches);
}

int gloc_m2dp_profile_reset(gloc_m2dp* h) { return handle_profile_reset(h); }

int gloc_m2dp_describe(gloc_m2dp* h, const float* xyz, size_t n, size_t stride_floats, float* out_desc, double* out_frame12,
                       uint32_t* out_counts) {
  GLOC_REQUIRE(h && out_desc && (xyz || n == 0), GLOC_ERR_INVALID, "null argument");
  GLOC_REQUIRE(stride_floats >= 3 && stride_floats <= 16, GLOC_ERR_INVALID, "stride_floats = %zu outside [3,16]", stride_floats);
  GLOC_REQUIRE(n < (1ull << 31), GLOC_ERR_INVALID, "scan too large");
  GLOC_HIP(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  GLOC_TRY(h->stage_pts.ensure(std::max<size_t>(16, sizeof(float) * stride_floats * n), s));
  if (n) GLOC_HIP(hipMemcpyAsync(h->stage_pts.p, xyz, sizeof(float) * stride_floats * n, hipMemcpyHostToDevice, s));
  h->h_tab.assign(1, ScanRef{h->stage_pts.as<float>(), (uint32_t)n, (uint32_t)stride_floats});
  GLOC_TRY(ensure_outputs(h, 1));
  GLOC_TRY(describe_tab(h, h->desc.as<float>()));
  return download(h, 1, out_desc, out_frame12, out_counts);
}

int gloc_m2dp_describe_store_scans(gloc_m2dp* h, gloc_scan_store* store, const uint32_t* scan_ids, size_t n, float* out_desc,
                                   double* out_frame12, uint32_t* out_counts) {
  GLOC_TRY(check_store(h, store, scan_ids, n));
  GLOC_REQUIRE(out_desc || n == 0, GLOC_ERR_INVALID, "null argument");
  if (!n) return GLOC_OK;
  GLOC_HIP(hipSetDevice(h->device));
  reg::ScopedPins pins(store, h->stream);
  GLOC_TRY(pin_scans(h, pins, scan_ids, n));
  GLOC_TRY(ensure_outputs(h, n));  // (h->desc is sized before its pointer is taken)
  GLOC_TRY(describe_tab(h, h->desc.as<float>()));
  return download(h, n, out_desc, out_frame12, out_counts);
}

int gloc_m2dp_describe_store_scans_device(gloc_m2dp* h, gloc_scan_store* store, const uint32_t* scan_ids, size_t n,
                                          float* d_out_desc) {
  GLOC_TRY(check_store(h, store, scan_ids, n));
  GLOC_REQUIRE(d_out_desc || n == 0, GLOC_ERR_INVALID, "null argument");
  if (!n) return GLOC_OK;
  GLOC_HIP(hipSetDevice(h->device));
  reg::ScopedPins pins(store, h->stream);
  GLOC_TRY(pin_scans(h, pins, scan_ids, n));
  return describe_tab(h, d_out_desc);  // (the pins' release waits for the stream: the points have been read)
}

int gloc_m2dp_signature_svd(gloc_m2dp* h, const uint32_t* counts, const uint32_t* n_points, size_t n_sig, float* out_desc,
                            double* out_sigma2) {
  GLOC_REQUIRE(h && ((counts && n_points && out_desc) || n_sig == 0), GLOC_ERR_INVALID, "null argument");
  GLOC_REQUIRE(n_sig <= 4096, GLOC_ERR_INVALID, "at most 4096 signatures per call (%zu)", n_sig);
  if (!n_sig) return GLOC_OK;
  GLOC_HIP(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  GLOC_TRY(ensure_outputs(h, n_sig));
  GLOC_HIP(hipMemcpyAsync(h->counts.p, counts, sizeof(uint32_t) * h->P * h->B * n_sig, hipMemcpyHostToDevice, s));
  GLOC_HIP(hipMemcpyAsync(h->n_used.p, n_points, sizeof(uint32_t) * n_sig, hipMemcpyHostToDevice, s));
  GLOC_TRY(launch_svd(h, n_sig, h->desc.as<float>(), h->sigma.as<double>()));
  if (out_sigma2) GLOC_HIP(hipMemcpyAsync(out_sigma2, h->sigma.p, sizeof(double) * 2 * n_sig, hipMemcpyDeviceToHost, s));
  return download(h, n_sig, out_desc, nullptr, nullptr);
}

int gloc_m2dp_frame_to_seed(const double* frame_q, const double* frame_db, float* T16) {
  GLOC_REQUIRE(frame_q && frame_db && T16, GLOC_ERR_INVALID, "null argument");
  double R[9], t[3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      double s = 0.0;
      for (int k = 0; k < 3; ++k) s += frame_db[3 * i + k] * frame_q[3 * j + k];  // R_db R_q^T
      R[3 * i + j] = s;
    }
  for (int i = 0; i < 3; ++i)
    t[i] = frame_db[9 + i] - ((R[3 * i] * frame_q[9] + R[3 * i + 1] * frame_q[10]) + R[3 * i + 2] * frame_q[11]);
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) T16[4 * i + j] = (float)R[3 * i + j];
    T16[4 * i + 3] = (float)t[i];
  }
  T16[12] = T16[13] = T16[14] = 0.f, T16[15] = 1.f;
  return GLOC_OK;
}

}  // extern "C"
