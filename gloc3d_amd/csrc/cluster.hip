// cluster.hip -- Euclidean clusters and outlier filters of the resident scans (E1 - E7 of include/gloc3d.h;
// tests/cluster_ref.py is the contract): host side of cluster_kernels.hpp and the entries gloc_scan_store_cluster,
// gloc_scan_store_add_filtered and gloc_scan_store_add_subset.  The traversal runs over the store's own sorted copy of a
// scan and the chunk boxes of ground::scan_chunk_boxes; the two neighbourhood filters read ground::scan_lists' counts and
// k-NN lists.  A filter stage leaves byte flags; its survivors are gathered on the device and become a scan through
// store_make_scan, as gloc_scan_store_add_device makes them -- a chain of stages is literally that, stage after stage,
// with the intermediate scans never given an id and their blocks handed back to the store's cache.
// The components' sizes and roots come to the host to be ranked (labels, not points); no point data does.
#include <algorithm>
#include <cmath>
#include <new>
#include <vector>

#include "cluster_kernels.hpp"
#include "scan_store.hpp"
#include "seg_sort.hpp"

static_assert(sizeof(gloc_cluster_params) == 16, "gloc_cluster_params is 16 bytes");
static_assert(sizeof(gloc_scan_filter_params) == 40, "gloc_scan_filter_params is 40 bytes");
static_assert(sizeof(gloc_scan_filter_info) == 20, "gloc_scan_filter_info is 20 bytes");

namespace gloc {
namespace cluster {

struct Ws {
  DevBuf parent, csize, root, label;         // [n] each, by upload index
  DevBuf k0, k1, v0, v1, hist, segs, first;  // E4: the sort by cluster and the clusters' runs
  DevBuf cent, lo, hi;                       // E4: [n_kept][3]
  DevBuf runfirst, psum, pmin, pmax;         // the first level of an ordered sum: per run of 64 terms (E4; E6: psum and counts)
  DevBuf flag, sel, count, tile_cnt, rows;   // a stage's survivors: flags, index list, how many (and the compaction's scratch), their xyz
  DevBuf mean, fin, stats;                   // E6
};

void free_ws(Ws* w) { delete w; }

namespace {

inline unsigned blocks(uint32_t n) { return (n + 255u) / 256u; }

// tolerance 0 = "no cluster stage": fine in a filter block, refused by gloc_scan_store_cluster itself
int check_tolerance(const gloc_cluster_params& c) {
  GLOC_REQUIRE(c.tolerance >= 0.f && std::isfinite(c.tolerance), GLOC_ERR_INVALID, "tolerance = %g must be finite and not negative",
               (double)c.tolerance);
  return GLOC_OK;
}

int check_sizes(const gloc_cluster_params& c) {
  GLOC_REQUIRE(c.max_size == 0 || c.min_size <= c.max_size, GLOC_ERR_INVALID, "min_size = %u above max_size = %u", c.min_size, c.max_size);
  return GLOC_OK;
}

int check_cluster_params(const gloc_cluster_params* p) {
  GLOC_REQUIRE(p, GLOC_ERR_INVALID, "cluster params is null");
  GLOC_TRY(check_tolerance(*p));
  GLOC_REQUIRE(p->tolerance > 0.f, GLOC_ERR_INVALID, "tolerance must be positive");
  GLOC_TRY(check_sizes(*p));
  GLOC_REQUIRE(p->reserved_ == 0, GLOC_ERR_INVALID, "reserved_ = %u must be 0", p->reserved_);
  return GLOC_OK;
}

int check_filter_params(const gloc_scan_filter_params* p) {
  GLOC_REQUIRE(p, GLOC_ERR_INVALID, "filter params is null");
  GLOC_REQUIRE(p->ror_radius >= 0.f && std::isfinite(p->ror_radius), GLOC_ERR_INVALID, "ror_radius = %g must be finite and not negative",
               (double)p->ror_radius);
  GLOC_TRY(check_tolerance(p->cluster));
  GLOC_TRY(check_sizes(p->cluster));
  GLOC_REQUIRE(p->sor_mean_k <= 15, GLOC_ERR_INVALID, "sor_mean_k = %u above 15", p->sor_mean_k);
  GLOC_REQUIRE(std::isfinite(p->sor_std_mul), GLOC_ERR_INVALID, "sor_std_mul is not finite");
  GLOC_REQUIRE(p->cluster.reserved_ == 0, GLOC_ERR_INVALID, "cluster.reserved_ = %u must be 0", p->cluster.reserved_);
  GLOC_REQUIRE(std::isfinite(p->min_range) && std::isfinite(p->max_range), GLOC_ERR_INVALID, "a range is not finite");
  GLOC_REQUIRE(!(p->min_range > 0.f && p->max_range > 0.f && p->min_range > p->max_range), GLOC_ERR_INVALID,
               "min_range = %g above max_range = %g", (double)p->min_range, (double)p->max_range);
  return GLOC_OK;
}

// E1 + E2 of a scan of n >= 1 points: w.root [n] and w.csize [n] (a component's size at its root) on the device.
int components(gloc_scan_store* st, Ws& w, const DevScan& s, float tolerance) {
  hipStream_t q = st->stream;
  const uint32_t n = (uint32_t)s.n, nch = (n + CHUNK - 1) / CHUNK;
  GLOC_TRY(w.parent.ensure(4 * s.n, q));
  GLOC_TRY(w.csize.ensure(4 * s.n, q));
  GLOC_TRY(w.root.ensure(4 * s.n, q));
  GLOC_TRY(ground::scan_chunk_boxes(q, st->nrm_ws, s.idx.pts, n));
  hipLaunchKernelGGL(cluster_init_kernel, dim3(blocks(n)), dim3(256), 0, q, w.parent.as<uint32_t>(), w.csize.as<uint32_t>(), n);
  hipLaunchKernelGGL(cluster_link_kernel, dim3((nch + 3) / 4), dim3(256), 0, q, s.idx.pts, n, st->nrm_ws.cbox_lo.as<f32x4>(),
                     st->nrm_ws.cbox_hi.as<f32x4>(), nch, tolerance * tolerance, w.parent.as<uint32_t>());
  hipLaunchKernelGGL(cluster_flatten_kernel, dim3(blocks(n)), dim3(256), 0, q, s.xyz, n, w.parent.as<uint32_t>(), w.root.as<uint32_t>(),
                     w.csize.as<uint32_t>());
  GLOC_HIP(hipGetLastError());
  return GLOC_OK;
}

struct Ranked {  // E3 on the host
  std::vector<uint32_t> root, label;  // [n]
  std::vector<uint32_t> size, croot;  // [n_kept], rank order
  uint32_t n_components = 0;
};

// E1 - E3: the roots and sizes come down, the kept components are ranked, and the labels go up again into w.label when
// something on the device is going to read them.
int rank_components(gloc_scan_store* st, Ws& w, const DevScan& s, const gloc_cluster_params& prm, bool labels_to_device, Ranked* out) {
  hipStream_t q = st->stream;
  const size_t n = s.n;
  GLOC_TRY(components(st, w, s, prm.tolerance));
  std::vector<uint32_t> csize(n);
  out->root.resize(n);
  GLOC_HIP(hipMemcpyAsync(out->root.data(), w.root.p, 4 * n, hipMemcpyDeviceToHost, q));
  GLOC_HIP(hipMemcpyAsync(csize.data(), w.csize.p, 4 * n, hipMemcpyDeviceToHost, q));
  GLOC_HIP(hipStreamSynchronize(q));
  const uint32_t lo = std::max(prm.min_size, 1u);
  out->n_components = 0;
  out->croot.clear();
  for (uint32_t i = 0; i < n; ++i) {
    if (out->root[i] != i) continue;
    ++out->n_components;
    if (csize[i] >= lo && (prm.max_size == 0 || csize[i] <= prm.max_size)) out->croot.push_back(i);
  }
  std::sort(out->croot.begin(), out->croot.end(), [&](uint32_t a, uint32_t b) { return csize[a] != csize[b] ? csize[a] > csize[b] : a < b; });
  const size_t K = out->croot.size();
  out->size.resize(K);
  std::vector<uint32_t> rank_of(n, NONE);
  for (size_t c = 0; c < K; ++c) {
    out->size[c] = csize[out->croot[c]];
    rank_of[out->croot[c]] = (uint32_t)c;
  }
  out->label.resize(n);
  for (size_t i = 0; i < n; ++i) out->label[i] = out->root[i] == NONE ? NONE : rank_of[out->root[i]];
  if (labels_to_device) {
    GLOC_TRY(w.label.ensure(4 * n, q));
    GLOC_HIP(hipMemcpyAsync(w.label.p, out->label.data(), 4 * n, hipMemcpyHostToDevice, q));
    GLOC_HIP(hipStreamSynchronize(q));  // (the vector may go before the stream gets there)
  }
  return GLOC_OK;
}

// E4 of the K >= 1 kept clusters of w.label: centroids, corners to the host arrays (each may be null).
int figures(gloc_scan_store* st, Ws& w, const DevScan& s, const Ranked& r, double* out_centroid3, float* out_lo3, float* out_hi3) {
  hipStream_t q = st->stream;
  const uint32_t n = (uint32_t)s.n, K = (uint32_t)r.size.size();
  GLOC_TRY(w.k0.ensure(4 * s.n, q));
  GLOC_TRY(w.k1.ensure(4 * s.n, q));
  GLOC_TRY(w.v0.ensure(4 * s.n, q));
  GLOC_TRY(w.v1.ensure(4 * s.n, q));
  GLOC_TRY(w.hist.ensure(segsort::scratch_bytes(1, n), q));
  GLOC_TRY(w.segs.ensure(sizeof(segsort::Seg), q));
  GLOC_TRY(w.first.ensure(4 * ((size_t)K + 1), q));
  GLOC_TRY(w.cent.ensure(24 * (size_t)K, q));
  GLOC_TRY(w.lo.ensure(12 * (size_t)K, q));
  GLOC_TRY(w.hi.ensure(12 * (size_t)K, q));
  std::vector<uint32_t> first(K + 1, 0u), runfirst(K + 1, 0u);  // where a cluster's points and its runs of 64 points begin
  for (uint32_t c = 0; c < K; ++c) {
    first[c + 1] = first[c] + r.size[c];
    runfirst[c + 1] = runfirst[c] + (r.size[c] + RUN - 1) / RUN;
  }
  const uint32_t runs = runfirst[K];
  GLOC_TRY(w.runfirst.ensure(4 * ((size_t)K + 1), q));
  GLOC_TRY(w.psum.ensure(24 * (size_t)runs, q));
  GLOC_TRY(w.pmin.ensure(12 * (size_t)runs, q));
  GLOC_TRY(w.pmax.ensure(12 * (size_t)runs, q));
  const segsort::Seg seg{0u, n};
  GLOC_HIP(hipMemcpyAsync(w.segs.p, &seg, sizeof(seg), hipMemcpyHostToDevice, q));
  GLOC_HIP(hipMemcpyAsync(w.first.p, first.data(), 4 * ((size_t)K + 1), hipMemcpyHostToDevice, q));
  GLOC_HIP(hipMemcpyAsync(w.runfirst.p, runfirst.data(), 4 * ((size_t)K + 1), hipMemcpyHostToDevice, q));
  uint32_t* kk[2] = {w.k0.as<uint32_t>(), w.k1.as<uint32_t>()};
  uint32_t* vv[2] = {w.v0.as<uint32_t>(), w.v1.as<uint32_t>()};
  hipLaunchKernelGGL(cluster_keys_kernel, dim3(blocks(n)), dim3(256), 0, q, w.label.as<uint32_t>(), n, K, kk[0], vv[0]);
  int bits = 1;  // of the largest key, K
  while (bits < 32 && (K >> bits) != 0u) ++bits;
  const int cur = segsort::sort_pairs<uint32_t, 8>(q, kk[0], kk[1], vv[0], vv[1], w.segs.as<segsort::Seg>(), 1, n, 0, bits, w.hist.as<uint32_t>());
  hipLaunchKernelGGL(cluster_run_sums_kernel, dim3(blocks(runs)), dim3(256), 0, q, s.xyz, vv[cur], w.first.as<uint32_t>(), w.runfirst.as<uint32_t>(), K,
                     w.psum.as<double>(), w.pmin.as<uint32_t>(), w.pmax.as<uint32_t>());
  hipLaunchKernelGGL(cluster_figures_kernel, dim3((K + 3) / 4), dim3(256), 0, q, w.first.as<uint32_t>(), w.runfirst.as<uint32_t>(), K,
                     w.psum.as<double>(), w.pmin.as<uint32_t>(), w.pmax.as<uint32_t>(), w.cent.as<double>(), w.lo.as<float>(), w.hi.as<float>());
  GLOC_HIP(hipGetLastError());
  if (out_centroid3) GLOC_HIP(hipMemcpyAsync(out_centroid3, w.cent.p, 24 * (size_t)K, hipMemcpyDeviceToHost, q));
  if (out_lo3) GLOC_HIP(hipMemcpyAsync(out_lo3, w.lo.p, 12 * (size_t)K, hipMemcpyDeviceToHost, q));
  if (out_hi3) GLOC_HIP(hipMemcpyAsync(out_hi3, w.hi.p, 12 * (size_t)K, hipMemcpyDeviceToHost, q));
  GLOC_HIP(hipStreamSynchronize(q));  // (seg and first are locals: the copies must have been consumed)
  return GLOC_OK;
}

// ---- the stages of E7: each leaves w.flag [n] of a scan of n >= 1 points --------------------------------------------------
int range_stage(gloc_scan_store* st, Ws& w, const DevScan& s, float min_range, float max_range) {
  const uint32_t n = (uint32_t)s.n;
  hipLaunchKernelGGL(range_flags_kernel, dim3(blocks(n)), dim3(256), 0, st->stream, s.xyz, n, min_range > 0.f ? min_range * min_range : -1.f,
                     max_range > 0.f ? max_range * max_range : -1.f, w.flag.as<uint8_t>());
  GLOC_HIP(hipGetLastError());
  return GLOC_OK;
}

int ror_stage(gloc_scan_store* st, Ws& w, const DevScan& s, float radius, uint32_t min_neighbors) {
  const uint32_t n = (uint32_t)s.n;
  GLOC_TRY(ground::scan_lists(st->stream, st->nrm_ws, s.idx.pts, n, Support::within(radius, 1u)));  // (the narrowest lists: the counts are what is read)
  hipLaunchKernelGGL(ror_flags_kernel, dim3(blocks(n)), dim3(256), 0, st->stream, s.xyz, n, st->nrm_ws.knn_cnt.as<uint32_t>(), min_neighbors,
                     w.flag.as<uint8_t>());
  GLOC_HIP(hipGetLastError());
  return GLOC_OK;
}

int sor_stage(gloc_scan_store* st, Ws& w, const DevScan& s, uint32_t mean_k, float std_mul) {
  hipStream_t q = st->stream;
  const uint32_t n = (uint32_t)s.n;
  const uint32_t W = std::max(mean_k + 1u, 3u);  // (the shortest list scan_lists makes; a longer list begins with the shorter one)
  GLOC_TRY(w.mean.ensure(8 * s.n, q));
  GLOC_TRY(w.fin.ensure(s.n, q));
  GLOC_TRY(w.stats.ensure(24, q));
  GLOC_TRY(ground::scan_lists(q, st->nrm_ws, s.idx.pts, n, Support::nearest(W)));
  hipLaunchKernelGGL(sor_mean_kernel, dim3(blocks(n)), dim3(256), 0, q, s.xyz, n, st->nrm_ws.knn_idx.as<uint32_t>(), st->nrm_ws.knn_d2.as<float>(),
                     (int)W, (int)mean_k, w.mean.as<double>(), w.fin.as<uint8_t>());
  const uint32_t runs = (n + RUN - 1) / RUN;
  GLOC_TRY(w.psum.ensure(8 * (size_t)runs, q));
  GLOC_TRY(w.pmin.ensure(4 * (size_t)runs, q));
  for (int pass = 0; pass < 2; ++pass) {  // the sum of m_i, then of (m_i - mu)^2
    hipLaunchKernelGGL(sor_run_sums_kernel, dim3(blocks(runs)), dim3(256), 0, q, w.mean.as<double>(), w.fin.as<uint8_t>(), n,
                       pass ? w.stats.as<double>() : nullptr, w.psum.as<double>(), w.pmin.as<uint32_t>());
    hipLaunchKernelGGL(sor_total_kernel, dim3(1), dim3(64), 0, q, w.psum.as<double>(), w.pmin.as<uint32_t>(), runs, pass, w.stats.as<double>());
  }
  hipLaunchKernelGGL(sor_flags_kernel, dim3(blocks(n)), dim3(256), 0, q, w.mean.as<double>(), w.fin.as<uint8_t>(), n, w.stats.as<double>(), std_mul,
                     w.flag.as<uint8_t>());
  GLOC_HIP(hipGetLastError());
  double stats[3] = {0.0, 0.0, 0.0};
  GLOC_HIP(hipMemcpyAsync(stats, w.stats.p, sizeof(stats), hipMemcpyDeviceToHost, q));
  GLOC_HIP(hipStreamSynchronize(q));
  GLOC_REQUIRE(stats[2] >= (double)(mean_k + 1u), GLOC_ERR_INVALID, "statistical outlier removal over %u neighbours: the scan has %.0f finite points",
               mean_k, stats[2]);
  return GLOC_OK;
}

int cluster_stage(gloc_scan_store* st, Ws& w, const DevScan& s, const gloc_cluster_params& prm) {
  Ranked r;
  GLOC_TRY(rank_components(st, w, s, prm, true, &r));
  const uint32_t n = (uint32_t)s.n;
  hipLaunchKernelGGL(label_flags_kernel, dim3(blocks(n)), dim3(256), 0, st->stream, w.label.as<uint32_t>(), n, w.flag.as<uint8_t>());
  GLOC_HIP(hipGetLastError());
  return GLOC_OK;
}

// Rows w.sel[0 .. m) of s as a scan of their own (not inserted).
int gather_scan(gloc_scan_store* st, Ws& w, const DevScan& s, uint32_t m, DevScan* out) {
  hipStream_t q = st->stream;
  GLOC_TRY(w.rows.ensure(12 * (size_t)m, q));
  hipLaunchKernelGGL(gather_rows_kernel, dim3(blocks(m)), dim3(256), 0, q, s.xyz, w.sel.as<uint32_t>(), m, w.rows.as<float>());
  GLOC_HIP(hipGetLastError());
  return reg::store_make_scan(st, w.rows.as<float>(), m, 3, true, out);
}

// The survivors of w.flag as a scan of their own; *m = 0 and no scan when there are none.
int derive(gloc_scan_store* st, Ws& w, const DevScan& s, DevScan* out, uint32_t* m) {
  hipStream_t q = st->stream;
  GLOC_TRY(w.sel.ensure(4 * s.n, q));
  GLOC_TRY(w.count.ensure(4, q));
  GLOC_TRY(ground::select_flagged(q, w.flag.as<uint8_t>(), (uint32_t)s.n, w.tile_cnt, w.sel.as<uint32_t>(), w.count.as<uint32_t>()));
  GLOC_HIP(hipMemcpyAsync(m, w.count.p, 4, hipMemcpyDeviceToHost, q));
  GLOC_HIP(hipStreamSynchronize(q));
  GLOC_REQUIRE(*m <= s.n, GLOC_ERR_STATE, "%u survivors of %zu points", *m, s.n);
  if (*m == 0) return GLOC_OK;
  return gather_scan(st, w, s, *m, out);
}

int add_filtered(gloc_scan_store* st, uint32_t base_id, const gloc_scan_filter_params& p, uint32_t* new_id, gloc_scan_filter_info* info) {
  GLOC_HIP(hipSetDevice(st->device));
  std::lock_guard<std::mutex> lk(st->mu);
  GLOC_REQUIRE(base_id < st->scans.size() && st->scans[base_id].live, GLOC_ERR_INVALID, "unknown scan id %u", base_id);
  const DevScan base = st->scans[base_id];  // (by value: read only, and the lock is held to the end)
  GLOC_REQUIRE(base.n < (1ull << 31), GLOC_ERR_INVALID, "scan too large");
  GLOC_TRY(ensure_ws(&st->cluster_ws));
  Ws& w = *st->cluster_ws;
  gloc_scan_filter_info inf{(uint32_t)base.n, (uint32_t)base.n, (uint32_t)base.n, (uint32_t)base.n, (uint32_t)base.n};
  uint32_t* const after[4] = {&inf.after_range, &inf.after_ror, &inf.after_sor, &inf.after_cluster};
  const bool on[4] = {p.min_range > 0.f || p.max_range > 0.f, p.ror_radius > 0.f, p.sor_mean_k > 0, p.cluster.tolerance > 0.f};
  DevScan cur = base;
  bool mine = false;  // cur is an intermediate scan of this call
  int rc = GLOC_OK;
  for (int stage = 0; stage < 4 && rc == GLOC_OK; ++stage) {
    uint32_t m = 0;
    if (on[stage] && cur.n != 0) {
      rc = w.flag.ensure(cur.n, st->stream);
      if (rc == GLOC_OK)
        rc = stage == 0   ? range_stage(st, w, cur, p.min_range, p.max_range)
             : stage == 1 ? ror_stage(st, w, cur, p.ror_radius, p.ror_min_neighbors)
             : stage == 2 ? sor_stage(st, w, cur, p.sor_mean_k, p.sor_std_mul)
                          : cluster_stage(st, w, cur, p.cluster);
      DevScan next;
      if (rc == GLOC_OK) rc = derive(st, w, cur, &next, &m);
      if (rc == GLOC_OK && m != 0) {
        if (mine) reg::store_free_scan(st, cur, true);
        cur = next;
        mine = true;
      }
    } else {
      m = (uint32_t)cur.n;
    }
    if (rc != GLOC_OK) break;
    for (int t = stage; t < 4; ++t) *after[t] = m;
    if (m == 0) {
      set_err("nothing survives the %s", stage == 0 ? "range crop" : stage == 1 ? "radius outlier removal" : stage == 2 ? "statistical outlier removal" : "cluster stage");
      rc = GLOC_ERR_INVALID;
    }
  }
  if (rc == GLOC_OK && !mine) {  // every stage off: a copy of the base scan
    DevScan copy;
    rc = reg::store_make_scan(st, base.xyz, base.n, 3, true, &copy);
    if (rc == GLOC_OK) {
      cur = copy;
      mine = true;
    }
  }
  if (info) *info = inf;
  if (rc != GLOC_OK) {
    (void)hipStreamSynchronize(st->stream);
    if (mine) reg::store_free_scan(st, cur, true);
    return rc;
  }
  return reg::store_insert_scan(st, cur, new_id);
}

}  // namespace
}  // namespace cluster
}  // namespace gloc

using namespace gloc;
using namespace gloc::cluster;

extern "C" {

void gloc_cluster_default_params(gloc_cluster_params* p) {
  if (!p) return;
  p->tolerance = 0.5f;
  p->min_size = 1;
  p->max_size = 0;
  p->reserved_ = 0;
}

void gloc_scan_filter_default_params(gloc_scan_filter_params* p) {
  if (!p) return;
  p->min_range = p->max_range = 0.f;
  p->ror_radius = 0.f;
  p->ror_min_neighbors = 0;
  p->sor_mean_k = 0;
  p->sor_std_mul = 1.0f;
  gloc_cluster_default_params(&p->cluster);
  p->cluster.tolerance = 0.f;
}

int gloc_scan_store_cluster(gloc_scan_store* st, uint32_t scan_id, const gloc_cluster_params* prm, uint32_t* out_root, uint32_t* out_cluster,
                            size_t capacity_points, uint32_t* out_size, uint32_t* out_cluster_root, double* out_centroid3, float* out_lo3,
                            float* out_hi3, size_t capacity_clusters, uint32_t* n_components, uint32_t* n_kept) {
  GLOC_TRY(check_cluster_params(prm));
  GLOC_REQUIRE(st, GLOC_ERR_INVALID, "null store");
  GLOC_HIP(hipSetDevice(st->device));
  std::lock_guard<std::mutex> lk(st->mu);
  GLOC_REQUIRE(scan_id < st->scans.size() && st->scans[scan_id].live, GLOC_ERR_INVALID, "unknown scan id %u", scan_id);
  const DevScan& s = st->scans[scan_id];
  GLOC_REQUIRE(s.n < (1ull << 31), GLOC_ERR_INVALID, "scan too large");
  const bool want_points = out_root || out_cluster, want_figures = out_centroid3 || out_lo3 || out_hi3;
  const bool want_clusters = out_size || out_cluster_root || want_figures;
  Ranked r;
  if (s.n) {
    GLOC_TRY(ensure_ws(&st->cluster_ws));
    GLOC_TRY(rank_components(st, *st->cluster_ws, s, *prm, want_figures, &r));
  }
  const size_t K = r.size.size();
  if (n_components) *n_components = r.n_components;
  if (n_kept) *n_kept = (uint32_t)K;
  const bool points_fit = capacity_points >= s.n, clusters_fit = capacity_clusters >= K;
  if (want_points && points_fit && s.n) {
    if (out_root) std::copy(r.root.begin(), r.root.end(), out_root);
    if (out_cluster) std::copy(r.label.begin(), r.label.end(), out_cluster);
  }
  if (want_clusters && clusters_fit && K) {
    if (out_size) std::copy(r.size.begin(), r.size.end(), out_size);
    if (out_cluster_root) std::copy(r.croot.begin(), r.croot.end(), out_cluster_root);
    if (want_figures) GLOC_TRY(figures(st, *st->cluster_ws, s, r, out_centroid3, out_lo3, out_hi3));
  }
  GLOC_REQUIRE(!want_points || points_fit, GLOC_ERR_INVALID, "buffers hold %zu points, the scan has %zu", capacity_points, s.n);
  GLOC_REQUIRE(!want_clusters || clusters_fit, GLOC_ERR_INVALID, "buffers hold %zu clusters, %zu are kept", capacity_clusters, K);
  return GLOC_OK;
}

int gloc_scan_store_add_filtered(gloc_scan_store* st, uint32_t base_id, const gloc_scan_filter_params* prm, uint32_t* new_id,
                                 gloc_scan_filter_info* info) {
  GLOC_TRY(check_filter_params(prm));
  GLOC_REQUIRE(st && new_id, GLOC_ERR_INVALID, "null argument");
  return add_filtered(st, base_id, *prm, new_id, info);
}

int gloc_scan_store_add_subset(gloc_scan_store* st, uint32_t base_id, const uint32_t* idx, size_t m, uint32_t* new_id) {
  GLOC_REQUIRE(idx && new_id, GLOC_ERR_INVALID, "null argument");
  GLOC_REQUIRE(m >= 1 && m < (1ull << 31), GLOC_ERR_INVALID, "a subset of %zu rows", m);
  GLOC_REQUIRE(st, GLOC_ERR_INVALID, "null store");
  GLOC_HIP(hipSetDevice(st->device));
  std::lock_guard<std::mutex> lk(st->mu);
  GLOC_REQUIRE(base_id < st->scans.size() && st->scans[base_id].live, GLOC_ERR_INVALID, "unknown scan id %u", base_id);
  const DevScan base = st->scans[base_id];
  for (size_t r = 0; r < m; ++r) GLOC_REQUIRE(idx[r] < base.n, GLOC_ERR_INVALID, "idx[%zu] = %u, the scan has %zu points", r, idx[r], base.n);
  GLOC_TRY(ensure_ws(&st->cluster_ws));
  Ws& w = *st->cluster_ws;
  hipStream_t q = st->stream;
  GLOC_TRY(w.sel.ensure(4 * m, q));
  GLOC_HIP(hipMemcpyAsync(w.sel.p, idx, 4 * m, hipMemcpyHostToDevice, q));
  DevScan s;
  const int rc = gather_scan(st, w, base, (uint32_t)m, &s);  // (synchronises: idx has been consumed)
  if (rc != GLOC_OK) {
    (void)hipStreamSynchronize(q);
    return rc;
  }
  return reg::store_insert_scan(st, s, new_id);
}

}  // extern "C"
