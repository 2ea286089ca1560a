// sc.hip -- C ABI of the Scan Context place descriptor (include/gloc3d.h, gloc_sc_*): a training-free descriptor built
// from resident or host scans, a resident database of them, and the exhaustive rotation-aligned search over it.  No
// counterpart in the reference; the contract is stated in the header and restated in numpy by tests/sc_ref.py.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <vector>

#include "common.hpp"
#include "sc_kernels.hpp"
#include "scan_store.hpp"

using namespace gloc;
using namespace gloc::sc;

struct gloc_sc : Handle {
  gloc_sc_params prm{};
  int R = 0, S = 0, NV = 0, CV = 0;  // rings, sectors, float4 per stored column, float4 per LDS column
  size_t n = 0;                      // rows of the database
  DevBuf raw, unit, mask, rkeys;     // [n][R * S] heights, [n][S][4 NV] unit columns, [n] masks, [n][R] ring keys
  DevBuf q_raw, q_unit, q_mask;      // the queries of a search / the descriptors of a describe call
  DevBuf stage_pts, scan_tab, row_ids, keys[3], o_dist, o_shift, o_by;
  std::vector<ScanRef> h_tab;
  std::vector<uint64_t> h_keys;
  size_t desc_len() const { return (size_t)R * S; }
  size_t unit_len() const { return (size_t)S * NV * 4; }
};

namespace {

int check_params(const gloc_sc_params* p) {
  GLOC_REQUIRE(p, GLOC_ERR_INVALID, "params is NULL");
  GLOC_REQUIRE(p->n_rings >= 1 && p->n_rings <= (uint32_t)MAX_RINGS, GLOC_ERR_INVALID, "n_rings = %u outside [1,%d]",
               p->n_rings, MAX_RINGS);
  GLOC_REQUIRE(p->n_sectors >= 2 && p->n_sectors <= (uint32_t)MAX_SECTORS, GLOC_ERR_INVALID,
               "n_sectors = %u outside [2,%d]", p->n_sectors, MAX_SECTORS);
  GLOC_REQUIRE(std::isfinite(p->max_radius) && p->max_radius > 0.f, GLOC_ERR_INVALID,
               "max_radius must be finite and positive");
  GLOC_REQUIRE(std::isfinite(p->sensor_height), GLOC_ERR_INVALID, "sensor_height must be finite");
  return GLOC_OK;
}

int check_rows(const gloc_sc* h, const float* desc, size_t n) {
  const size_t len = n * h->desc_len();
  for (size_t i = 0; i < len; ++i)
    GLOC_REQUIRE(std::isfinite(desc[i]) && desc[i] >= 0.f, GLOC_ERR_INVALID,
                 "descriptor %zu holds %g at bin %zu: heights are finite and not negative", i / h->desc_len(),
                 (double)desc[i], i % h->desc_len());
  return GLOC_OK;
}

int grow(gloc_sc* h, size_t rows) {
  hipStream_t s = h->stream;
  GLOC_TRY(h->raw.ensure(sizeof(float) * h->desc_len() * rows, s, true, sizeof(float) * h->desc_len() * h->n));
  GLOC_TRY(h->unit.ensure(sizeof(float) * h->unit_len() * rows, s, true, sizeof(float) * h->unit_len() * h->n));
  GLOC_TRY(h->mask.ensure(sizeof(uint64_t) * rows, s, true, sizeof(uint64_t) * h->n));
  GLOC_TRY(h->rkeys.ensure(sizeof(float) * h->R * rows, s, true, sizeof(float) * h->R * h->n));
  return GLOC_OK;
}

int ensure_queries(gloc_sc* h, size_t nq) {
  hipStream_t s = h->stream;
  GLOC_TRY(h->q_raw.ensure(sizeof(float) * h->desc_len() * nq, s));
  GLOC_TRY(h->q_unit.ensure(sizeof(float) * h->unit_len() * nq, s));
  GLOC_TRY(h->q_mask.ensure(sizeof(uint64_t) * nq, s));
  return GLOC_OK;
}

// the scans of h->h_tab -> d_bins [count][R * S]
int scatter(gloc_sc* h, float* d_bins) {
  hipStream_t s = h->stream;
  const size_t count = h->h_tab.size();
  uint32_t most = 0;
  for (const ScanRef& r : h->h_tab) most = std::max(most, r.n);
  GLOC_HIP(hipMemsetAsync(d_bins, 0, sizeof(float) * h->desc_len() * count, s));
  if (!most) return GLOC_OK;
  GLOC_TRY(h->scan_tab.ensure(sizeof(ScanRef) * count, s));
  GLOC_HIP(hipMemcpyAsync(h->scan_tab.p, h->h_tab.data(), sizeof(ScanRef) * count, hipMemcpyHostToDevice, s));
  ProfScope ps(h->prof, "sc_scatter", s);
  const unsigned gx = (unsigned)std::min<size_t>(((size_t)most + 1023) / 1024, 64);  // >= 4 points per thread
  hipLaunchKernelGGL(scatter_kernel, dim3(gx, (unsigned)count), dim3(256), 0, s, h->scan_tab.as<ScanRef>(), h->R, h->S,
                     h->prm.max_radius, h->prm.sensor_height, reinterpret_cast<uint32_t*>(d_bins));
  GLOC_HIP(hipGetLastError());
  return GLOC_OK;
}

int scatter_host_scan(gloc_sc* h, const float* xyz, size_t n, size_t stride, float* d_bins) {
  GLOC_REQUIRE(xyz || n == 0, GLOC_ERR_INVALID, "null argument");
  GLOC_REQUIRE(stride >= 3 && stride <= 16, GLOC_ERR_INVALID, "stride_floats = %zu outside [3,16]", stride);
  GLOC_REQUIRE(n < (1ull << 31), GLOC_ERR_INVALID, "scan too large");
  hipStream_t s = h->stream;
  GLOC_TRY(h->stage_pts.ensure(std::max<size_t>(16, sizeof(float) * stride * n), s));
  if (n) GLOC_HIP(hipMemcpyAsync(h->stage_pts.p, xyz, sizeof(float) * stride * n, hipMemcpyHostToDevice, s));
  h->h_tab.assign(1, ScanRef{h->stage_pts.as<float>(), (uint32_t)n, (uint32_t)stride});
  return scatter(h, d_bins);
}

int check_store(const gloc_sc* h, const gloc_scan_store* store, const uint32_t* scan_ids, size_t n) {
  GLOC_REQUIRE(h && store && (n == 0 || scan_ids), GLOC_ERR_INVALID, "null argument");
  GLOC_REQUIRE(store->device == h->device, GLOC_ERR_INVALID, "store on device %d, descriptor handle on %d", store->device,
               h->device);
  GLOC_REQUIRE(n <= 4096, GLOC_ERR_INVALID, "at most 4096 scans per call (%zu)", n);
  return GLOC_OK;
}

// (the pins are the caller's: they outlive the kernels that read the scans)
int scatter_store_scans(gloc_sc* h, reg::ScopedPins& pins, const uint32_t* scan_ids, size_t n, float* d_bins) {
  GLOC_TRY(pins.pin(scan_ids, nullptr, n));
  h->h_tab.clear();
  for (const DevScan& sc : pins.scans) {
    GLOC_REQUIRE(sc.n < (1ull << 31), GLOC_ERR_INVALID, "scan too large");
    h->h_tab.push_back(ScanRef{sc.xyz, (uint32_t)sc.n, 3u});
  }
  return scatter(h, d_bins);
}

int finish(gloc_sc* h, const float* d_raw, size_t count, float* d_unit, uint64_t* d_mask, float* d_rkeys) {
  if (!count) return GLOC_OK;
  ProfScope ps(h->prof, "sc_finish", h->stream);
  hipLaunchKernelGGL(finish_kernel, dim3((unsigned)count), dim3(64), 0, h->stream, d_raw, h->R, h->S, h->NV * 4, d_unit,
                     d_mask, d_rkeys);
  GLOC_HIP(hipGetLastError());
  return GLOC_OK;
}

// rows [first, first + count) of the database hold their heights: the derived layout, then they count
int finish_rows(gloc_sc* h, size_t first, size_t count) {
  GLOC_TRY(finish(h, h->raw.as<float>() + first * h->desc_len(), count, h->unit.as<float>() + first * h->unit_len(),
                  h->mask.as<uint64_t>() + first, h->rkeys.as<float>() + first * h->R));
  GLOC_HIP(hipStreamSynchronize(h->stream));
  h->n = first + count;
  return GLOC_OK;
}

int launch_dist(gloc_sc* h, const float* d_qunit, const uint64_t* d_qmask, uint32_t nq, const uint32_t* d_row_list,
                uint32_t row_begin, uint32_t n_rows, uint64_t* d_key, float* d_dist, uint32_t* d_shift, float* d_by) {
  ProfScope ps(h->prof, "sc_dist", h->stream);
  const dim3 grid((n_rows + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK, (nq + QB - 1) / QB), block(256);
  const size_t lds = sizeof(float4) * (QB + DIST_WAVES) * h->S * h->CV;
#define GLOC_SC_DIST(NV_)                                                                                             \
  case NV_:                                                                                                           \
    hipLaunchKernelGGL(dist_kernel<NV_>, grid, block, lds, h->stream, reinterpret_cast<const float4*>(d_qunit), d_qmask, \
                       nq, h->unit.as<float4>(), h->mask.as<uint64_t>(), d_row_list, row_begin, n_rows, h->S, h->CV,  \
                       h->prm.min_common_columns, d_key, d_dist, d_shift, d_by);                                      \
    break;
  switch (h->NV) {
    GLOC_SC_DIST(1) GLOC_SC_DIST(2) GLOC_SC_DIST(3) GLOC_SC_DIST(4) GLOC_SC_DIST(5) GLOC_SC_DIST(6) GLOC_SC_DIST(7)
    GLOC_SC_DIST(8)
  }
#undef GLOC_SC_DIST
  GLOC_HIP(hipGetLastError());
  return GLOC_OK;
}

// h->q_unit / q_mask hold nq queries: the k best rows of [row_begin, row_end) each.  Queries go through in groups that keep
// the key table below 2^25 entries; a query's result does not depend on its group.
int search_prepared(gloc_sc* h, size_t nq, size_t k, size_t row_begin, size_t row_end, uint64_t* out_idx, float* out_dist,
                    uint32_t* out_shift) {
  hipStream_t s = h->stream;
  row_end = std::min(row_end, h->n);
  row_begin = std::min(row_begin, row_end);
  const size_t n_rows = row_end - row_begin;
  GLOC_REQUIRE(n_rows < (1u << 24), GLOC_ERR_INVALID, "a window of %zu rows: at most 2^24 - 1", n_rows);
  h->h_keys.assign(nq * k, NO_KEY);
  if (n_rows) {
    const size_t group = std::max<size_t>(1, std::min<size_t>({nq, (size_t)4096, ((size_t)1 << 25) / n_rows}));
    const size_t lists = (n_rows + SORT_N - 1) / SORT_N;
    GLOC_TRY(h->keys[0].ensure(sizeof(uint64_t) * group * n_rows, s));
    GLOC_TRY(h->keys[1].ensure(sizeof(uint64_t) * group * lists * k, s));
    GLOC_TRY(h->keys[2].ensure(sizeof(uint64_t) * group * ((lists * k + SORT_N - 1) / SORT_N) * k, s));
    for (size_t q0 = 0; q0 < nq; q0 += group) {
      const uint32_t g = (uint32_t)std::min(group, nq - q0);
      GLOC_TRY(launch_dist(h, h->q_unit.as<float>() + q0 * h->unit_len(), h->q_mask.as<uint64_t>() + q0, g, nullptr,
                           (uint32_t)row_begin, (uint32_t)n_rows, h->keys[0].as<uint64_t>(), nullptr, nullptr, nullptr));
      const uint64_t* in = h->keys[0].as<uint64_t>();
      size_t n_in = n_rows, in_stride = n_rows;
      int to = 1;
      {
        ProfScope ps(h->prof, "sc_select", s);
        for (;;) {
          const size_t nb = (n_in + SORT_N - 1) / SORT_N;
          uint64_t* out = h->keys[to].as<uint64_t>();
          hipLaunchKernelGGL(topk_step_kernel, dim3((unsigned)nb, g), dim3(SORT_N / 2), 0, s, in, (uint32_t)n_in, in_stride, out,
                             (uint32_t)k, nb * k);
          GLOC_HIP(hipGetLastError());
          in = out, n_in = in_stride = nb * k, to = to == 1 ? 2 : 1;
          if (nb == 1) break;
        }
      }
      GLOC_HIP(hipMemcpyAsync(h->h_keys.data() + q0 * k, in, sizeof(uint64_t) * g * k, hipMemcpyDeviceToHost, s));
      GLOC_HIP(hipStreamSynchronize(s));
    }
  } else {
    GLOC_HIP(hipStreamSynchronize(s));  // (the queries' upload: the caller's buffer is free when the call returns)
  }
  for (size_t i = 0; i < nq * k; ++i) {
    const uint64_t key = h->h_keys[i];
    const bool none = key == NO_KEY;
    const uint32_t bits = (uint32_t)(key >> 32);
    float d;
    memcpy(&d, &bits, sizeof(d));
    out_idx[i] = none ? UINT64_MAX : row_begin + ((key >> 8) & 0xFFFFFFu);
    out_dist[i] = none ? FLT_MAX : d;
    if (out_shift) out_shift[i] = none ? 0u : (uint32_t)(key & 0xFFu);
  }
  return GLOC_OK;
}

int check_search(const gloc_sc* h, size_t nq, size_t k, const void* out_idx, const void* out_dist) {
  GLOC_REQUIRE(h && out_idx && out_dist, GLOC_ERR_INVALID, "null argument");
  GLOC_REQUIRE(k >= 1 && k <= (size_t)MAX_K, GLOC_ERR_INVALID, "k = %zu outside [1,%d]", k, MAX_K);
  GLOC_REQUIRE(nq >= 1 && nq <= (1u << 20), GLOC_ERR_INVALID, "nq = %zu outside [1,2^20]", nq);
  return GLOC_OK;
}

}  // namespace

extern "C" {

int gloc_sc_default_params(gloc_sc_params* p) {
  GLOC_REQUIRE(p, GLOC_ERR_INVALID, "params is NULL");
  p->n_rings = 20;  // Kim & Kim, IROS 2018: 20 rings x 60 sectors out to 80 m, heights above a ground 2 m below the sensor
  p->n_sectors = 60;
  p->max_radius = 80.f;
  p->sensor_height = 2.f;
  p->min_common_columns = 1;
  p->reserved_ = 0;
  return GLOC_OK;
}

int gloc_sc_create(int device, const gloc_sc_params* params, gloc_sc** out) {
  GLOC_REQUIRE(out, GLOC_ERR_INVALID, "out is NULL");
  *out = nullptr;
  GLOC_TRY(check_params(params));  // (before the device is looked at: a bad block is refused on any machine)
  GLOC_TRY(create_handle(device, out));
  gloc_sc* h = *out;
  h->prm = *params;
  h->R = (int)params->n_rings, h->S = (int)params->n_sectors;
  h->NV = (h->R + 3) / 4;
  h->CV = h->NV | 1;  // an odd stride in 16-byte slots: the 16 lanes of a b128 read group fall on 16 different slots
  if (sizeof(float4) * (QB + DIST_WAVES) * h->S * h->CV > 65536) h->CV = h->NV;  // (30+ rings x 57+ sectors: unpadded)
  return GLOC_OK;
}

int gloc_sc_destroy(gloc_sc* h) { return destroy_handle(h); }

int gloc_sc_set_stream(gloc_sc* h, void* hip_stream) { return handle_set_stream(h, hip_stream); }

int gloc_sc_synchronize(gloc_sc* h) { return handle_synchronize(h); }

int gloc_sc_set_profile(gloc_sc* h, int enable) { return handle_set_profile(h, enable); }

int gloc_sc_profile(gloc_sc* h, const char* kernel, double* total_ms, uint64_t* launches) {
  return handle_profile(h, kernel, total_ms, launches);
}

int gloc_sc_profile_reset(gloc_sc* h) { return handle_profile_reset(h); }

int gloc_sc_describe(gloc_sc* h, const float* xyz, size_t n, size_t stride_floats, float* out_desc) {
  GLOC_REQUIRE(h && out_desc, GLOC_ERR_INVALID, "null argument");
  GLOC_HIP(hipSetDevice(h->device));
  GLOC_TRY(ensure_queries(h, 1));
  GLOC_TRY(scatter_host_scan(h, xyz, n, stride_floats, h->q_raw.as<float>()));
  GLOC_HIP(hipMemcpyAsync(out_desc, h->q_raw.p, sizeof(float) * h->desc_len(), hipMemcpyDeviceToHost, h->stream));
  GLOC_HIP(hipStreamSynchronize(h->stream));
  return GLOC_OK;
}

int gloc_sc_describe_store_scans(gloc_sc* h, gloc_scan_store* store, const uint32_t* scan_ids, size_t n, float* out_desc) {
  GLOC_TRY(check_store(h, store, scan_ids, n));
  GLOC_REQUIRE(out_desc || n == 0, GLOC_ERR_INVALID, "null argument");
  if (!n) return GLOC_OK;
  GLOC_HIP(hipSetDevice(h->device));
  GLOC_TRY(ensure_queries(h, n));
  reg::ScopedPins pins(store, h->stream);
  GLOC_TRY(scatter_store_scans(h, pins, scan_ids, n, h->q_raw.as<float>()));
  GLOC_HIP(hipMemcpyAsync(out_desc, h->q_raw.p, sizeof(float) * h->desc_len() * n, hipMemcpyDeviceToHost, h->stream));
  GLOC_HIP(hipStreamSynchronize(h->stream));
  return GLOC_OK;
}

int gloc_sc_add(gloc_sc* h, const float* desc, size_t n) {
  GLOC_REQUIRE(h && (desc || n == 0), GLOC_ERR_INVALID, "null argument");
  if (!n) return GLOC_OK;
  GLOC_TRY(check_rows(h, desc, n));
  GLOC_HIP(hipSetDevice(h->device));
  GLOC_TRY(grow(h, h->n + n));
  GLOC_HIP(hipMemcpyAsync(h->raw.as<float>() + h->n * h->desc_len(), desc, sizeof(float) * h->desc_len() * n,
                          hipMemcpyHostToDevice, h->stream));
  return finish_rows(h, h->n, n);
}

int gloc_sc_add_scan(gloc_sc* h, const float* xyz, size_t n, size_t stride_floats, uint64_t* row) {
  GLOC_REQUIRE(h, GLOC_ERR_INVALID, "null handle");
  GLOC_HIP(hipSetDevice(h->device));
  GLOC_TRY(grow(h, h->n + 1));
  GLOC_TRY(scatter_host_scan(h, xyz, n, stride_floats, h->raw.as<float>() + h->n * h->desc_len()));
  if (row) *row = h->n;
  return finish_rows(h, h->n, 1);
}

int gloc_sc_add_store_scans(gloc_sc* h, gloc_scan_store* store, const uint32_t* scan_ids, size_t n, uint64_t* first_row) {
  GLOC_TRY(check_store(h, store, scan_ids, n));
  if (first_row) *first_row = h->n;
  if (!n) return GLOC_OK;
  GLOC_HIP(hipSetDevice(h->device));
  GLOC_TRY(grow(h, h->n + n));
  reg::ScopedPins pins(store, h->stream);
  GLOC_TRY(scatter_store_scans(h, pins, scan_ids, n, h->raw.as<float>() + h->n * h->desc_len()));
  return finish_rows(h, h->n, n);
}

int gloc_sc_size(const gloc_sc* h, size_t* n_rows) {
  GLOC_REQUIRE(h && n_rows, GLOC_ERR_INVALID, "null argument");
  *n_rows = h->n;
  return GLOC_OK;
}

int gloc_sc_clear(gloc_sc* h) {
  GLOC_REQUIRE(h, GLOC_ERR_INVALID, "null handle");
  h->n = 0;
  return GLOC_OK;
}

int gloc_sc_reserve(gloc_sc* h, size_t n_rows) {
  GLOC_REQUIRE(h, GLOC_ERR_INVALID, "null handle");
  GLOC_REQUIRE(n_rows < (1u << 24), GLOC_ERR_INVALID, "n_rows = %zu: at most 2^24 - 1", n_rows);
  GLOC_HIP(hipSetDevice(h->device));
  return grow(h, n_rows);
}

int gloc_sc_rows(gloc_sc* h, size_t first, size_t n, float* out_desc) {
  GLOC_REQUIRE(h && (out_desc || n == 0), GLOC_ERR_INVALID, "null argument");
  GLOC_REQUIRE(first <= h->n && n <= h->n - first, GLOC_ERR_INVALID, "rows [%zu, %zu) of %zu", first, first + n, h->n);
  if (!n) return GLOC_OK;
  GLOC_HIP(hipSetDevice(h->device));
  GLOC_HIP(hipMemcpyAsync(out_desc, h->raw.as<float>() + first * h->desc_len(), sizeof(float) * h->desc_len() * n,
                          hipMemcpyDeviceToHost, h->stream));
  GLOC_HIP(hipStreamSynchronize(h->stream));
  return GLOC_OK;
}

int gloc_sc_ring_keys(gloc_sc* h, size_t first, size_t n, float* out_keys) {
  GLOC_REQUIRE(h && (out_keys || n == 0), GLOC_ERR_INVALID, "null argument");
  GLOC_REQUIRE(first <= h->n && n <= h->n - first, GLOC_ERR_INVALID, "rows [%zu, %zu) of %zu", first, first + n, h->n);
  if (!n) return GLOC_OK;
  GLOC_HIP(hipSetDevice(h->device));
  GLOC_HIP(hipMemcpyAsync(out_keys, h->rkeys.as<float>() + first * h->R, sizeof(float) * h->R * n, hipMemcpyDeviceToHost,
                          h->stream));
  GLOC_HIP(hipStreamSynchronize(h->stream));
  return GLOC_OK;
}

// File: "GLOCSCTX", u32 version (1), u32 rows, the gloc_sc_params block (24 bytes), rows x n_rings x n_sectors fp32.
int gloc_sc_save(gloc_sc* h, const char* path) {
  GLOC_REQUIRE(h && path, GLOC_ERR_INVALID, "null argument");
  std::vector<float> buf(h->n * h->desc_len());
  GLOC_TRY(gloc_sc_rows(h, 0, h->n, buf.data()));
  FILE* f = fopen(path, "wb");
  GLOC_REQUIRE(f, GLOC_ERR_INVALID, "cannot open %s for writing", path);
  const uint32_t hdr[2] = {1u, (uint32_t)h->n};
  bool ok = fwrite("GLOCSCTX", 1, 8, f) == 8 && fwrite(hdr, 4, 2, f) == 2 && fwrite(&h->prm, sizeof(h->prm), 1, f) == 1 &&
            fwrite(buf.data(), sizeof(float), buf.size(), f) == buf.size();
  ok = (fclose(f) == 0) && ok;
  GLOC_REQUIRE(ok, GLOC_ERR_STATE, "writing %s failed", path);
  return GLOC_OK;
}

int gloc_sc_load(gloc_sc* h, const char* path) {
  GLOC_REQUIRE(h && path, GLOC_ERR_INVALID, "null argument");
  FILE* f = fopen(path, "rb");
  GLOC_REQUIRE(f, GLOC_ERR_INVALID, "cannot open %s", path);
  char magic[8];
  uint32_t hdr[2] = {0, 0};
  gloc_sc_params fp;
  std::vector<float> buf;
  const char* why = nullptr;
  if (fread(magic, 1, 8, f) != 8 || memcmp(magic, "GLOCSCTX", 8) != 0 || fread(hdr, 4, 2, f) != 2 || hdr[0] != 1u ||
      fread(&fp, sizeof(fp), 1, f) != 1)
    why = "is not a GLOCSCTX file of version 1";
  else if (fp.n_rings != h->prm.n_rings || fp.n_sectors != h->prm.n_sectors ||
           memcmp(&fp.max_radius, &h->prm.max_radius, 4) != 0 || memcmp(&fp.sensor_height, &h->prm.sensor_height, 4) != 0 ||
           fp.min_common_columns != h->prm.min_common_columns)
    why = "was written with other parameters than the handle's";
  else {
    buf.resize((size_t)hdr[1] * h->desc_len());
    if (fread(buf.data(), sizeof(float), buf.size(), f) != buf.size()) why = "is truncated";
  }
  fclose(f);
  GLOC_REQUIRE(!why, GLOC_ERR_INVALID, "%s %s", path, why);
  return gloc_sc_add(h, buf.data(), hdr[1]);
}

int gloc_sc_search(gloc_sc* h, const float* q_desc, size_t nq, size_t k, size_t row_begin, size_t row_end,
                   uint64_t* out_idx, float* out_dist, uint32_t* out_shift) {
  GLOC_TRY(check_search(h, nq, k, out_idx, out_dist));
  GLOC_REQUIRE(q_desc, GLOC_ERR_INVALID, "null argument");
  GLOC_TRY(check_rows(h, q_desc, nq));
  GLOC_HIP(hipSetDevice(h->device));
  GLOC_TRY(ensure_queries(h, nq));
  GLOC_HIP(hipMemcpyAsync(h->q_raw.p, q_desc, sizeof(float) * h->desc_len() * nq, hipMemcpyHostToDevice, h->stream));
  GLOC_TRY(finish(h, h->q_raw.as<float>(), nq, h->q_unit.as<float>(), h->q_mask.as<uint64_t>(), nullptr));
  return search_prepared(h, nq, k, row_begin, row_end, out_idx, out_dist, out_shift);
}

int gloc_sc_search_store_scans(gloc_sc* h, gloc_scan_store* store, const uint32_t* q_scan_ids, size_t nq, size_t k,
                               size_t row_begin, size_t row_end, uint64_t* out_idx, float* out_dist, uint32_t* out_shift) {
  GLOC_TRY(check_search(h, nq, k, out_idx, out_dist));
  GLOC_TRY(check_store(h, store, q_scan_ids, nq));
  GLOC_HIP(hipSetDevice(h->device));
  GLOC_TRY(ensure_queries(h, nq));
  {
    reg::ScopedPins pins(store, h->stream);
    GLOC_TRY(scatter_store_scans(h, pins, q_scan_ids, nq, h->q_raw.as<float>()));
  }  // (the pins' release waits for the stream: the points have been read)
  GLOC_TRY(finish(h, h->q_raw.as<float>(), nq, h->q_unit.as<float>(), h->q_mask.as<uint64_t>(), nullptr));
  return search_prepared(h, nq, k, row_begin, row_end, out_idx, out_dist, out_shift);
}

int gloc_sc_distances(gloc_sc* h, const float* q_desc, const uint64_t* rows, size_t n, float* out_dist,
                      uint32_t* out_shift, float* out_by_shift) {
  GLOC_REQUIRE(h && q_desc && rows && out_dist && out_shift, GLOC_ERR_INVALID, "null argument");
  GLOC_REQUIRE(n >= 1 && n <= (1u << 20), GLOC_ERR_INVALID, "n = %zu outside [1,2^20]", n);
  GLOC_TRY(check_rows(h, q_desc, 1));
  std::vector<uint32_t> ids(n);
  for (size_t i = 0; i < n; ++i) {
    GLOC_REQUIRE(rows[i] < h->n, GLOC_ERR_INVALID, "row %llu of %zu", (unsigned long long)rows[i], h->n);
    ids[i] = (uint32_t)rows[i];
  }
  GLOC_HIP(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  GLOC_TRY(ensure_queries(h, 1));
  GLOC_TRY(h->row_ids.ensure(sizeof(uint32_t) * n, s));
  GLOC_TRY(h->o_dist.ensure(sizeof(float) * n, s));
  GLOC_TRY(h->o_shift.ensure(sizeof(uint32_t) * n, s));
  if (out_by_shift) GLOC_TRY(h->o_by.ensure(sizeof(float) * n * h->S, s));
  GLOC_HIP(hipMemcpyAsync(h->q_raw.p, q_desc, sizeof(float) * h->desc_len(), hipMemcpyHostToDevice, s));
  GLOC_HIP(hipMemcpyAsync(h->row_ids.p, ids.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice, s));
  GLOC_TRY(finish(h, h->q_raw.as<float>(), 1, h->q_unit.as<float>(), h->q_mask.as<uint64_t>(), nullptr));
  GLOC_TRY(launch_dist(h, h->q_unit.as<float>(), h->q_mask.as<uint64_t>(), 1, h->row_ids.as<uint32_t>(), 0, (uint32_t)n,
                       nullptr, h->o_dist.as<float>(), h->o_shift.as<uint32_t>(),
                       out_by_shift ? h->o_by.as<float>() : nullptr));
  GLOC_HIP(hipMemcpyAsync(out_dist, h->o_dist.p, sizeof(float) * n, hipMemcpyDeviceToHost, s));
  GLOC_HIP(hipMemcpyAsync(out_shift, h->o_shift.p, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, s));
  if (out_by_shift) GLOC_HIP(hipMemcpyAsync(out_by_shift, h->o_by.p, sizeof(float) * n * h->S, hipMemcpyDeviceToHost, s));
  GLOC_HIP(hipStreamSynchronize(s));  // (ids goes out of scope)
  return GLOC_OK;
}

int gloc_sc_shift_to_yaw(const gloc_sc_params* params, uint32_t shift, float* yaw) {
  GLOC_REQUIRE(yaw, GLOC_ERR_INVALID, "null argument");
  GLOC_TRY(check_params(params));
  GLOC_REQUIRE(shift < params->n_sectors, GLOC_ERR_INVALID, "shift = %u of %u sectors", shift, params->n_sectors);
  const double a = 2.0 * M_PI * (double)shift / (double)params->n_sectors;
  *yaw = (float)(a > M_PI ? a - 2.0 * M_PI : a);
  return GLOC_OK;
}

}  // extern "C"
