// scan_store.hpp -- host-side view of the resident scan store (gloc_scan_store of include/gloc3d.h),
// shared by scan_store.hip (which owns it and indexes the scans), scan_features.hip (which gives the scans their normals
// and features) and reg.hip (whose registration handles read it).
#pragma once
#include <algorithm>
#include <atomic>
#include <map>
#include <mutex>
#include <vector>

#include "common.hpp"
#include "ground_normals.hpp"
#include "p2l.hpp"  // gn6::Call, p2l::SourceView: what CallScans resolves
#include "scan_index.hpp"

// A scan resident in HBM: original-order xyz plus its search index (Hilbert-sorted copy with the
// original indices, boxes, sorted keys, inverse permutation, launch order).  ONE allocation per scan.
struct DevScan {
  void* block = nullptr;
  size_t block_bytes = 0;
  float* xyz = nullptr;  // original order, packed
  size_t n = 0;
  gloc::reg::ScanIndexDev idx{};
  // Launch order of the source groups (groups of 64 * cs sorted points, widest first), ONE ARRAY PER cs in
  // {1, 2, 4}, each built once (cs = 2 at upload, the others on first request) and never rewritten: a
  // DevScan copy handed out by store_get() keeps pointing at valid, unchanging data whatever other
  // handles or later calls ask for.  `order` of a copy returned by store_get(cs) is the array of that cs
  // (null for cs = 0: a target's order is never read).
  uint32_t* order_base = nullptr;
  uint32_t* order = nullptr;
  unsigned order_built = 0;  // bit (cs) set: order_of(cs) is valid
  uint32_t* kpos_mem = nullptr;  // room for the target index's curve position -> kd position table
  gloc::reg::KdRecord* kdt_mem = nullptr;  // ... and for its split planes (scan_index.hpp): kd_table_records(n) records
  size_t order_g1 = 0;       // groups at cs = 1
  uint32_t* order_of(int cs) const {
    return order_base + (cs == 1 ? 0 : cs == 2 ? order_g1 : order_g1 + (order_g1 + 1) / 2);
  }
  // Per-point normals (gloc_scan_store_build_normals), an OPTIONAL SECOND allocation of 12 B per point: packed xyz in the
  // order of idx.pts -- the order the 1-NN search reports its matches in -- so that a correspondence reads its normal at
  // the index it got.  Built once per (scan, support); re-ordered with the points by the kd re-sort; zero = no normal.
  float* nrm = nullptr;
  gloc::Support nrm_sup;  // what they were built from (none: no normals)
  size_t nrm_bytes() const { return nrm ? 12 * n : 0; }
  // FPFH features (gloc_scan_store_build_fpfh), an OPTIONAL THIRD allocation of 132 B per point: rows of 33 floats in the
  // order of idx.pts, as the normals are, and re-ordered with them.  Built once per (scan, normals' support, features'
  // support); valid for the normals they were built from only (fpfh_nsup = that nrm_sup); the zero row = no feature.
  float* fpfh = nullptr;
  gloc::Support fpfh_nsup, fpfh_fsup;  // the supports of the normals they were built on and of their own lists (none: no features)
  size_t fpfh_bytes() const { return fpfh ? 132 * n : 0; }
  bool has_normals(const gloc::Support& ns) const { return nrm_sup == ns; }
  bool has_fpfh(const gloc::Support& ns, const gloc::Support& fs) const { return fpfh_nsup == ns && fpfh_fsup == fs && nrm_sup == ns; }
  // ISS keypoints (gloc_scan_store_build_keypoints), an OPTIONAL allocation of 4 B per keypoint: their ORIGINAL indices in
  // ascending order -- nothing the kd re-sort moves -- K known to the host, tagged with the parameters they were built from.
  // kp_feat: the keypoints' feature rows [K][33] in list order, what the keypoint-restricted matcher reads; valid for the
  // features it was gathered from only, so dropped whenever the features or the keypoints are rebuilt and gathered again
  // on the next request.
  uint32_t* kp = nullptr;
  float* kp_feat = nullptr;
  size_t kp_n = 0;
  bool kp_built = false;  // (K = 0 is a keypoint set too)
  gloc_iss_params kp_prm{};
  size_t kp_bytes() const { return (kp ? 4 * kp_n : 0) + (kp_feat ? 132 * kp_n : 0); }
  bool has_keypoints(const gloc_iss_params& p) const {
    return kp_built && kp_prm.salient_radius == p.salient_radius && kp_prm.max_nn == p.max_nn && kp_prm.min_nn == p.min_nn &&
           kp_prm.non_max_radius == p.non_max_radius && kp_prm.gamma_21 == p.gamma_21 && kp_prm.gamma_32 == p.gamma_32;
  }
  bool live = false;
  bool kd = false;  // the index is in kd order (target index)
  int pins = 0;     // batches in flight (gloc_reg_batch_multi_begin .. _end) whose jobs hold a by-value view of THIS scan:
                    // it may not be re-sorted in place meanwhile (store_pin / store_unpin, under the store's mutex)
};

namespace gloc {
namespace submap {
struct Ws;  // the scratch of gloc_scan_store_add_submaps (submap.hip), made on first use
void free_ws(Ws* w);
}  // namespace submap
namespace cluster {
struct Ws;  // the scratch of gloc_scan_store_cluster / _add_filtered / _add_subset (cluster.hip), made on first use
void free_ws(Ws* w);
}  // namespace cluster
}  // namespace gloc

struct gloc_scan_store : gloc::Handle {  // (always on its own stream; the base's profiler stays idle)
  std::mutex mu;  // guards the tables, the store's stream and its scratch
  std::vector<DevScan> scans;
  std::vector<uint32_t> free_ids;
  std::multimap<size_t, void*> free_blocks;  // released allocations by capacity, reused by later adds
  size_t live_count = 0, live_bytes = 0, cached_bytes = 0;
  // scratch of the indexing pipeline (scan_store.hip): sort ping-pong arrays over all scans of a batch, descriptor
  // tables, bounding-box partials, radix histograms; the same for the source-group sort and the kd re-sort
  gloc::DevBuf sort_keys, sort_keys2, sort_vals, sort_perm, sort_hist, stage, part, builds, segs;
  gloc::DevBuf grp_k0, grp_k1, grp_v0, grp_v1, grp_segs;
  gloc::DevBuf kd_k0, kd_k1, kd_v0, kd_v1, kd_p0, kd_p1, kd_h0, kd_h1, kd_box, kd_desc;
  gloc::ground::NormalsScratch nrm_ws;  // the normals' k-NN lists and staging (gloc_scan_store_build_normals)
  gloc::DevBuf nrm_tmp;                 // normals in original order, between the normal kernel / a download and the sorted copy
  gloc::DevBuf fpfh_tmp, spfh_tmp;      // features in original order (as nrm_tmp) and the SPFH counts they are summed from
  gloc::DevBuf iss_sal, iss_sal_sorted, iss_eig, iss_flag, iss_list, iss_count;  // the keypoint detector's scratch (iss.hip)
  gloc::submap::Ws* submap_ws = nullptr;
  gloc::cluster::Ws* cluster_ws = nullptr;
  std::atomic<int> attached{0};  // registration handles using this store
  ~gloc_scan_store() {
    gloc::submap::free_ws(submap_ws);
    gloc::cluster::free_ws(cluster_ws);
    for (auto& s : scans) {
      if (s.block) (void)hipFree(s.block);
      if (s.nrm) (void)hipFree(s.nrm);
      if (s.fpfh) (void)hipFree(s.fpfh);
      if (s.kp) (void)hipFree(s.kp);
      if (s.kp_feat) (void)hipFree(s.kp_feat);
    }
    for (auto& kv : free_blocks) (void)hipFree(kv.second);
  }
};

namespace gloc {
namespace reg {

// Build a scan from host (`device_src` false) or device memory into a fresh or recycled allocation;
// returns after the indexing work has completed on the store's stream.  Caller holds store->mu.
int store_make_scan(gloc_scan_store* st, const float* pts, size_t n, size_t stride, bool device_src,
                    DevScan* out);
// The same for `count` scans in ONE launch sequence (kernels take the scan from blockIdx.y, sorts are segmented).
int store_make_scans(gloc_scan_store* st, size_t count, const float* const* pts, const size_t* n, size_t stride,
                     bool device_src, DevScan* out);
void store_free_scan(gloc_scan_store* st, DevScan& s, bool cache_block);
// Give a scan made by store_make_scan an id (a recycled one first).  Caller holds store->mu.
int store_insert_scan(gloc_scan_store* st, const DevScan& s, uint32_t* id);
// Take a live, unpinned scan out again (its block goes to the cache, its id is free).  Caller holds store->mu.
void store_remove_scan(gloc_scan_store* st, uint32_t id);
// Re-sort an indexed scan into kd order (target index) and rebuild everything that depends on the order.
// Caller holds store->mu; nothing may be reading the scan; returns after the work has completed.
int store_build_target_index(gloc_scan_store* st, DevScan& s);
int store_build_target_indices(gloc_scan_store* st, DevScan* const* scans, size_t count);  // batches of <= 8 M points
// Build (once) the launch order of a scan for `cs` source points per lane into its own array and point
// s.order at it.  Caller holds store->mu.
int store_build_order(gloc_scan_store* st, DevScan& s, int cs);
// Copy of scan `id` (by value: the table may grow under another thread) with `order` = the launch order
// for `cs` sources per lane (cs = 0: the scan is used as a target only, no order).  GLOC_ERR_INVALID if unknown.
int store_get(gloc_scan_store* st, uint32_t id, int cs, DevScan* out);
// A batch about to be enqueued takes the by-value views of the scans its jobs read AND pins them under ONE acquisition of
// the store's mutex (round 6; before, the views were taken first and pinned afterwards: a re-sort or a release by another
// thread in between left the batch with a stale view).  All or nothing: an unknown id or a failed launch-order build
// pins nothing.  ids may repeat (pins are counted).  gloc_scan_store_build_target_index refuses a pinned scan that still
// needs the re-sort, gloc_scan_store_release refuses any pinned scan.
int store_get_pinned(gloc_scan_store* st, const uint32_t* ids, const int* cs, size_t count, DevScan* out);
// Give a scan its normals from the support ns (no-op when it has them from it).  Caller holds store->mu; returns after the
// work has completed.  Adds an allocation and moves nothing: safe on a pinned scan, except that normals a batch may be
// reading are not rebuilt from another support (GLOC_ERR_STATE).  One set of normals and one of features per scan,
// whichever support they were built from.
int store_build_normals(gloc_scan_store* st, DevScan& s, const Support& ns);
// Give a scan its FPFH features from the support fs and normals of ns (built or rebuilt first when the scan's differ:
// store_build_normals and its rule); no-op when it has them from these two.  Caller holds store->mu; returns after the
// work has completed.  Features a batch may be reading are not rebuilt (GLOC_ERR_STATE).
int store_build_fpfh(gloc_scan_store* st, DevScan& s, const Support& ns, const Support& fs);
// ... for a list of ids (takes store->mu).  GLOC_ERR_INVALID for an unknown id.
int store_ensure_fpfh(gloc_scan_store* st, const uint32_t* ids, size_t n, const Support& ns, const Support& fs);
// Give a scan its ISS keypoints of prm (iss.hip; no-op when it has them from these parameters), and the table of their
// feature rows when the scan has features.  Caller holds store->mu; returns after the work has completed.  Keypoints a
// batch may be reading are not rebuilt (GLOC_ERR_STATE).
int store_build_keypoints(gloc_scan_store* st, DevScan& s, const gloc_iss_params& prm);
// ... for a list of ids whose features exist (takes store->mu).  GLOC_ERR_INVALID for an unknown id.
int store_ensure_keypoints(gloc_scan_store* st, const uint32_t* ids, size_t n, const gloc_iss_params& prm);
// Let go of the table of the keypoints' feature rows: what every rebuild of the features or the normals under them calls.
void store_drop_keypoint_rows(gloc_scan_store* st, DevScan& s);
int check_iss_params(const gloc_iss_params* prm);
// A scan's normals between original order and the order of its sorted points (`pts`, n of them): what the builders, the
// downloads and the target-index re-sort, which moves the points under them, all go through.  Enqueued on q.
int store_reorder_normals(hipStream_t q, const f32x4* pts, uint32_t n, const float* in, float* out, bool to_sorted);
// The pins' release (delta = -1) once the batch's event has been waited for.  Ids no longer live are skipped.
void store_pin(gloc_scan_store* st, const uint32_t* ids, size_t count, int delta);
// Scans without normals get them from k neighbours -- normals from any other support are used as they are (takes
// store->mu; an allocation beside the scan: nothing a batch in flight reads moves).  GLOC_ERR_INVALID for an unknown id.
int store_ensure_normals(gloc_scan_store* st, const uint32_t* ids, size_t n, uint32_t k);

// The scans of a synchronous call, pinned for as long as the holder lives: pin() is store_get_pinned (cs null: no launch
// orders, the scans are only read) and `scans` its views; the destructor waits for the stream and lets the pins go.  A
// pin() that failed has pinned nothing, and then nothing is let go.
struct ScopedPins {
  gloc_scan_store* st;
  hipStream_t q;
  std::vector<uint32_t> ids;
  std::vector<DevScan> scans;
  ScopedPins(gloc_scan_store* st_, hipStream_t q_) : st(st_), q(q_) {}
  ScopedPins(const ScopedPins&) = delete;
  ScopedPins& operator=(const ScopedPins&) = delete;
  int pin(const uint32_t* ids_, const int* cs, size_t n) {
    const std::vector<int> none(cs ? 0 : n, 0);
    scans.resize(n);
    GLOC_TRY(store_get_pinned(st, ids_, cs ? cs : none.data(), n, scans.data()));
    ids.assign(ids_, ids_ + n);
    return GLOC_OK;
  }
  ~ScopedPins() {
    if (ids.empty()) return;
    (void)hipStreamSynchronize(q);
    store_pin(st, ids.data(), ids.size(), -1);
  }
};

// The distinct ids of a list in order of first appearance, and for every entry its index among them.
inline void distinct_in_order(const uint32_t* ids, size_t n, std::vector<uint32_t>* uniq, std::vector<uint32_t>* index_of) {
  uniq->clear();
  index_of->resize(n);
  for (size_t c = 0; c < n; ++c) {
    auto it = std::find(uniq->begin(), uniq->end(), ids[c]);
    (*index_of)[c] = (uint32_t)(it - uniq->begin());
    if (it == uniq->end()) uniq->push_back(ids[c]);
  }
}

// What a list of (source, target) pairs is refused for before anything is enqueued: an id the store does not know (a
// target of 0xFFFFFFFF is "no target", not an id) and a source that is empty or too large.  Looks each distinct id up once.
inline int store_check_pairs(gloc_scan_store* st, const uint32_t* src_ids, const uint32_t* tgt_ids, size_t n) {
  std::vector<uint32_t> seen_src, seen_tgt, at;
  distinct_in_order(src_ids, n, &seen_src, &at);
  distinct_in_order(tgt_ids, n, &seen_tgt, &at);
  DevScan s;
  for (const uint32_t id : seen_src) {
    GLOC_TRY(store_get(st, id, 0, &s));
    GLOC_REQUIRE(s.n >= 1 && s.n < (1ull << 31), GLOC_ERR_INVALID, "the source scan %u is empty or too large", id);
  }
  for (const uint32_t id : seen_tgt)
    if (id != 0xFFFFFFFFu) GLOC_TRY(store_get(st, id, 0, &s));
  return GLOC_OK;
}

constexpr uint32_t NO_SCAN = 0xFFFFFFFFu;  // "no target" in a pair list

// The scans of a refinement call (gn6::Call), resolved once for reg.hip's run_refine and vgicp::run: the ids checked
// before anything is enqueued (a pair list: store_check_pairs), every distinct source and then every distinct target
// pinned for as long as this lives, targets -- and with src_normals sources -- without normals given them from normal_k
// neighbours, and every job's source as the accumulate kernels take it.  cs: the sources' launch order (0: nothing searches).
// normal_k 0: a call that reads no normals (the point-to-point evaluation, eval.hip) -- none is built, none is asked for.
struct CallScans {
  ScopedPins pins;                         // .scans: the distinct sources, then the distinct targets
  size_t n_srcs = 0;
  std::vector<uint32_t> job_src, job_tgt;  // [n]: which of each job c reads; job_tgt NO_SCAN: a row without a target
  std::vector<p2l::SourceView> srcs;       // [n]; n = 0 in such a row: no work-group, no pair
  CallScans(gloc_scan_store* st, hipStream_t q) : pins(st, q) {}
  const DevScan& src(size_t c) const { return pins.scans[job_src[c]]; }
  const DevScan* tgt(size_t c) const { return job_tgt[c] == NO_SCAN ? nullptr : &pins.scans[n_srcs + job_tgt[c]]; }
  int resolve(const gn6::Call& c, uint32_t normal_k, bool src_normals, int cs) {
    gloc_scan_store* st = pins.st;
    GLOC_REQUIRE(st, GLOC_ERR_INVALID, "unknown scan id %u", c.src_ids[0]);
    if (c.pairs) GLOC_TRY(store_check_pairs(st, c.src_ids, c.tgt_ids, c.n));
    std::vector<uint32_t> ids, have, uniq, have_tgt;
    distinct_in_order(c.src_ids, c.pairs ? c.n : 1, &ids, &job_src);
    job_src.resize(c.n, 0u);
    n_srcs = ids.size();
    for (size_t j = 0; j < c.n; ++j)
      if (!c.pairs || c.tgt_ids[j] != NO_SCAN) have.push_back(c.tgt_ids[j]);
    distinct_in_order(have.data(), have.size(), &uniq, &have_tgt);
    job_tgt.assign(c.n, NO_SCAN);
    for (size_t j = 0, k = 0; j < c.n; ++j)
      if (!c.pairs || c.tgt_ids[j] != NO_SCAN) job_tgt[j] = have_tgt[k++];
    ids.insert(ids.end(), uniq.begin(), uniq.end());
    // (an unknown source id without src_normals: refused by pin())
    const size_t first = src_normals ? 0 : n_srcs;
    if (normal_k) GLOC_TRY(store_ensure_normals(st, ids.data() + first, ids.size() - first, normal_k));
    std::vector<int> css(ids.size(), 0);
    std::fill(css.begin(), css.begin() + n_srcs, cs);
    GLOC_TRY(pins.pin(ids.data(), css.data(), ids.size()));
    const std::vector<DevScan>& scans = pins.scans;
    for (size_t u = 0; u < scans.size(); ++u) {
      const DevScan& s = scans[u];
      if (u < n_srcs) GLOC_REQUIRE(s.n >= 1 && s.n < (1ull << 31), GLOC_ERR_INVALID, "the source scan is empty or too large");
      const bool read = normal_k && (u < n_srcs ? src_normals : s.n > 0);  // are its normals read (an empty target has none)
      GLOC_REQUIRE(!read || s.nrm, GLOC_ERR_STATE, "scan %u lost its normals during the call", ids[u]);
    }
    srcs.resize(c.n);
    for (size_t j = 0; j < c.n; ++j)
      srcs[j] = p2l::SourceView{src(j).idx.pts, src_normals ? src(j).nrm : nullptr, job_tgt[j] == NO_SCAN ? 0u : (uint32_t)src(j).n};
    return GLOC_OK;
  }
};

}  // namespace reg
}  // namespace gloc
