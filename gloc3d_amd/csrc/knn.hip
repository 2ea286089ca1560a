// knn.hip -- C ABI of the descriptor kNN (include/gloc3d.h) over the kernels in knn_kernels.hpp.
// Replaces registration/loop_detector.cpp:34-45,66-79 (KD-tree build + query) and
// main.py:317-324 (faiss.IndexFlatL2 add/search) of the reference.
#include <algorithm>
#include <atomic>
#include <cfloat>
#include <vector>

#include "comm.hpp"
#include "common.hpp"
#include "knn_kernels.hpp"
#include "synth_kernels.hpp"

using namespace gloc;
using namespace gloc::knn;

// The database: what a handle owns and its views (gloc_knn_create_view) read.
struct KnnRows {
  size_t n = 0;
  DevBuf rows;      // n x dim fp32, row-major, dense
  DevBuf norms;     // n fp32 (coarse form only)
  DevBuf mirror;    // the rows again, split into two bf16 values and tiled by 64 rows (knn_kernels.hpp: mirror_rows_kernel) --
                    // what the split-bf16 coarse pass streams; dim % 8 == 0 only; kept current by every add
  DevBuf dn_max;    // 1 x uint32 (bits of the largest row norm)
};

struct gloc_knn : Handle {
  size_t dim = 0;
  KnnRows own;       // (stays empty in a view)
  KnnRows* db = &own;  // the rows searched: a view's are its parent's, as they are now -- read through this pointer, never
                       // grown or freed through it (GLOC_NOT_VIEW)
  DevBuf dist;      // exact: [nq][ld]; mfma: [splits][Qpad][ld]
  DevBuf keys;      // select output [nq][K]
  DevBuf n_incomplete;  // 1 x u64: queries the MFMA path sent to the exact fallback (device counter)
  DevBuf shard_ws;  // gloc_knn_search_sharded: local + gathered lists
  DevBuf klists, klists2;  // per-chunk K-lists during selection
  DevBuf exact;     // rerank: reference-order distances [nq][KC]
  DevBuf keys2;     // rerank output [nq][k]
  DevBuf qnorm;     // [nq]
  DevBuf qsplit;    // [nq][dim / 8][8 bf16 h, 8 bf16 m]: the queries of the split-bf16 coarse pass
  DevBuf flags;     // [nq] int
  DevBuf redo_tickets;  // [nq] u32: flagged_redo_kernel's tickets (0 between searches)
  DevBuf bmin;          // [nq][blocks of 32 rows]: the coarse kernel's block minima (large windows, one K-split)
  DevBuf stage_q;   // host-API staging: queries
  DevBuf stage_idx, stage_d2;
  int* h_flags = nullptr;  // pinned
  size_t h_flags_cap = 0;
  // The split-bf16 coarse pass proves less on data whose neighbours lie close together relative to the norms (its bound is
  // eight times the fp32 form's): a search whose queries mostly went to the exact pass costs far more than the fp32 coarse pass
  // would have.  The fallback counter is copied to the host behind every tracked search (no wait: it is looked at when the
  // next search finds the copy done); above a quarter of the queries the handle's next 64 searches take the fp32 form, then
  // the split form is tried again.  Results do not depend on it.
  unsigned long long* h_inc = nullptr;  // pinned: the counter as of the tracked search
  hipEvent_t inc_ev = nullptr;
  bool inc_pending = false;
  unsigned long long inc_seen = 0;      // the counter at the last look
  size_t inc_queries = 0;               // queries of the tracked search
  int coarse_fp32_left = 0;             // searches still to run on the fp32 coarse pass
  int algo = GLOC_KNN_ALGO_AUTO;
  int candidates = 32;
  gloc_knn_stats stats{};
  gloc_knn* parent = nullptr;  // gloc_knn_create_view: a view searches db = &parent->own with its own stream and workspace
  int views = 0;  // live views of this handle
  ~gloc_knn() {
    if (h_flags) (void)hipHostFree(h_flags);
    if (h_inc) (void)hipHostFree(h_inc);
    if (inc_ev) (void)hipEventDestroy(inc_ev);
  }
};

namespace {

#define GLOC_NOT_VIEW(h) \
  GLOC_REQUIRE(!(h)->parent, GLOC_ERR_STATE, "a view (gloc_knn_create_view) searches its parent's rows: add / reserve / clear / load on the parent")

int ensure_rows(gloc_knn* h, size_t n_rows) {
  GLOC_NOT_VIEW(h);
  GLOC_TRY(h->db->rows.ensure(n_rows * h->dim * sizeof(float), h->stream, true, h->db->n * h->dim * sizeof(float)));
  GLOC_TRY(h->db->norms.ensure(n_rows * sizeof(float), h->stream, true, h->db->n * sizeof(float)));
  if (h->dim % 8 == 0) {  // (whole tiles, and two more: the coarse kernel's last work-group may own a tile past the end)
    const size_t tile_bytes = mirror_tile_u32x4((int)h->dim) * 16;
    // (+ 8 KB: a step's four planes of the last tile when dim / 8 is no multiple of four -- dist_bf16x3_tiled_kernel)
    GLOC_TRY(h->db->mirror.ensure(((n_rows + MIR_ROWS - 1) / MIR_ROWS + 2) * tile_bytes + 8192, h->stream, true,
                                  (h->db->n + MIR_ROWS - 1) / MIR_ROWS * tile_bytes));
  }
  if (!h->db->dn_max.p) {
    GLOC_TRY(h->db->dn_max.ensure(sizeof(uint32_t), h->stream));
    GLOC_HIP(hipMemsetAsync(h->db->dn_max.p, 0, sizeof(uint32_t), h->stream));
  }
  return GLOC_OK;
}

int update_norms(gloc_knn* h, size_t first, size_t count) {
  if (!count) return GLOC_OK;
  ProfScope ps(h->prof, "norms", h->stream);
  const unsigned blocks = (unsigned)((count + 3) / 4);
  hipLaunchKernelGGL(row_norms_kernel, dim3(blocks), dim3(256), 0, h->stream,
                     h->db->rows.as<float>() + first * h->dim, count, (int)h->dim,
                     h->db->norms.as<float>() + first, h->db->dn_max.as<uint32_t>());
  GLOC_HIP(hipGetLastError());
  if (h->dim % 8 == 0) {  // the coarse pass's mirror of the same rows
    ProfScope pm(h->prof, "mirror", h->stream);
    hipLaunchKernelGGL(mirror_rows_kernel, dim3((unsigned)((count + 63) / 64), (unsigned)((h->dim / 8 + 3) / 4)), dim3(256), 0, h->stream,
                       h->db->rows.as<float>(), first, count, (int)h->dim, h->db->mirror.as<u32x4>());
    GLOC_HIP(hipGetLastError());
  }
  return GLOC_OK;
}

// ---- exact path ------------------------------------------------------------------------------
int launch_dist_exact(gloc_knn* h, const float* d_q, int nq, size_t first, int n_range,
                      size_t ld, const int* only_flagged = nullptr) {
  ProfScope ps(h->prof, "dist_exact", h->stream);
  const int QT = only_flagged ? 1 : (nq >= 8 ? 8 : (nq >= 4 ? 4 : (nq >= 2 ? 2 : 1)));
  const int qgroups = (nq + QT - 1) / QT;
  if (nq <= 2) {
    // one or two queries: the streaming form (one wave per work-group, all group sums before the chains);
    // measured against the general kernel at 4541 x 4096: Q = 1 18.6 vs 33 us, Q = 2 equal, Q = 4 / 8 slower
    const int G = (int)h->dim >> 2, Gs = std::min(G, EXS_G);
    float* dist = h->dist.as<float>();
    const float* db = h->db->rows.as<float>();
#define LAUNCH_SMALL(QT_, RW_)                                                                             \
  hipLaunchKernelGGL((dist_exact_small_kernel<QT_, RW_>), dim3((unsigned)((n_range + RW_ - 1) / RW_), (unsigned)qgroups), \
                     dim3(64), sizeof(float) * (QT_ * RW_) * (Gs + 4), h->stream, db, d_q, dist, (int)h->dim, \
                     first, n_range, nq, ld, only_flagged)
    if (QT == 2) LAUNCH_SMALL(2, 4);
    else LAUNCH_SMALL(1, 4);
#undef LAUNCH_SMALL
    GLOC_HIP(hipGetLastError());
    return GLOC_OK;
  }
  // rows per wave: fill the chip with >= ~2048 waves when the window is small, up to 64/QT
  int RW = 64 / QT;
  while (RW > 4 && (long long)((n_range + RW - 1) / RW) * qgroups < 2048) RW >>= 1;
  if (RW < 4) RW = 4;
  const unsigned gx = (unsigned)((n_range + 4 * RW - 1) / (4 * RW));
  // (the flagged pass over a large window: y = 1, every work-group walks the flags)
  dim3 grid(gx, (only_flagged && (long long)gx * qgroups > 4096) ? 1u : (unsigned)qgroups), block(256);
  float* dist = h->dist.as<float>();
  const float* db = h->db->rows.as<float>();
#define LAUNCH_EXACT(QT_)                                                                      \
  hipLaunchKernelGGL(dist_exact_kernel<QT_>, grid, block, 0, h->stream, db, d_q, dist,         \
                     (int)h->dim, first, n_range, nq, RW, ld, only_flagged)
  switch (QT) {
    case 8: LAUNCH_EXACT(8); break;
    case 4: LAUNCH_EXACT(4); break;
    case 2: LAUNCH_EXACT(2); break;
    default: LAUNCH_EXACT(1); break;
  }
#undef LAUNCH_EXACT
  GLOC_HIP(hipGetLastError());
  return GLOC_OK;
}

template <int MODE>
int launch_slices(gloc_knn* h, const float* d_q, int nq, int K, size_t first, int n_range, size_t ld, size_t strideP,
                  int n_splits, const SlicePlan& sl, const int* only_flagged) {
  GLOC_TRY(h->klists.ensure((size_t)nq * sl.S * K * sizeof(uint64_t), h->stream));
  // (the flagged pass: y = 1, every work-group walks the flags)
#define SLICES_ARGS                                                                                                 \
  dim3(SELQ_THREADS), 0, h->stream, h->dist.as<float>(), ld, strideP, n_splits, h->qnorm.as<float>(), d_q, (int)h->dim, \
      h->db->norms.as<float>(), first, n_range, sl.L, K, h->klists.as<uint64_t>(), only_flagged, nq
  if constexpr (MODE == 0) {  // (only the exact pass is ever launched for flagged queries)
    if (only_flagged)
      hipLaunchKernelGGL((select_slices_kernel<0, true>), dim3(sl.S, 1), SLICES_ARGS);
    else
      hipLaunchKernelGGL((select_slices_kernel<0, false>), dim3(sl.S, nq), SLICES_ARGS);
  } else {
    GLOC_REQUIRE(!only_flagged, GLOC_ERR_STATE, "internal: flagged selection of coarse distances");
    hipLaunchKernelGGL((select_slices_kernel<MODE, false>), dim3(sl.S, nq), SLICES_ARGS);
  }
#undef SLICES_ARGS
  GLOC_HIP(hipGetLastError());
  return GLOC_OK;
}

const FinalOut KEYS_ONLY{nullptr, nullptr, 0, 1};

// Per-query top-K of h->dist in the form `sp` names (knn_plan.hpp: plan_select).  MODE as select_chunk_kernel.  Window and
// Slices also write the result through `fo` when it is given; Chunks leaves the keys alone (through_fo below).
template <int MODE>
int run_select(gloc_knn* h, const SelectPlan& sp, const float* d_q, int nq, int K, size_t first, int n_range, size_t ld,
               size_t strideP, int n_splits, uint64_t* d_keys_out, const int* only_flagged = nullptr,
               const FinalOut& fo = KEYS_ONLY) {
  ProfScope ps(h->prof, "select", h->stream);
  if (sp.form == Selection::Window) {
    hipLaunchKernelGGL(select_query_kernel<MODE>, dim3(nq), dim3(SELQ_THREADS), 0, h->stream, h->dist.as<float>(), ld,
                       strideP, n_splits, h->qnorm.as<float>(), d_q, (int)h->dim, h->db->norms.as<float>(), first, n_range,
                       K, d_keys_out, only_flagged, fo);
    GLOC_HIP(hipGetLastError());
    return GLOC_OK;
  }
  if (sp.form == Selection::Slices) {
    const SlicePlan& sl = sp.sl;
    GLOC_TRY(launch_slices<MODE>(h, d_q, nq, K, first, n_range, ld, strideP, n_splits, sl, only_flagged));
    hipLaunchKernelGGL(select_query_kernel<2>, dim3(nq), dim3(SELQ_THREADS), 0, h->stream,
                       reinterpret_cast<const float*>(h->klists.as<uint64_t>()), (size_t)2 * sl.S * K, (size_t)0, 1,
                       (float*)nullptr, (const float*)nullptr, (int)h->dim, (const float*)nullptr, (size_t)0, sl.S * K, K,
                       d_keys_out, only_flagged, fo);
    GLOC_HIP(hipGetLastError());
    return GLOC_OK;
  }
  const int per_group = SEL_LIST / K;  // lists one merge can take
  int E = (n_range + 256 * per_group - 1) / (256 * per_group);
  E = std::max(E, 8);
  E = std::min(E, std::max(1, SEL_LIST / K));
  // the device-side fallback (only_flagged) selects with ONE work-group per query, so that no merge
  // launch is needed (measured for the main path: one work-group per query over 10 000 rows takes 47 us,
  // five chunks + one merge 18 + 10 us -- the main path keeps its chunks)
  const int e_one = (n_range + 255) / 256;
  if (only_flagged && n_range <= SELECT_ONE_BLOCK_MAX && e_one <= std::max(1, SEL_LIST / K)) E = std::max(e_one, 1);
  int nlists = (n_range + 256 * E - 1) / (256 * E);
  GLOC_TRY(h->klists.ensure((size_t)nq * nlists * K * sizeof(uint64_t), h->stream));
  uint64_t* cur = nlists == 1 ? d_keys_out : h->klists.as<uint64_t>();
  hipLaunchKernelGGL(select_chunk_kernel<MODE>, dim3(nlists, nq), dim3(256), 0, h->stream,
                     h->dist.as<float>(), ld, strideP, n_splits, h->qnorm.as<float>(), d_q, (int)h->dim,
                     h->db->norms.as<float>(), first, n_range, K, E, cur, only_flagged);
  GLOC_HIP(hipGetLastError());
  bool flip = false;
  while (nlists > 1) {
    const int ngroups = (nlists + per_group - 1) / per_group;
    uint64_t* nxt;
    if (ngroups == 1) {
      nxt = d_keys_out;
    } else {
      DevBuf& b = flip ? h->klists : h->klists2;
      GLOC_TRY(b.ensure((size_t)nq * ngroups * K * sizeof(uint64_t), h->stream));
      nxt = b.as<uint64_t>();
    }
    hipLaunchKernelGGL(select_merge_kernel, dim3(ngroups, nq), dim3(256), 0, h->stream, cur, nlists,
                       per_group, K, nxt);
    GLOC_HIP(hipGetLastError());
    cur = nxt;
    nlists = ngroups;
    flip = !flip;
  }
  return GLOC_OK;
}

// *through_fo (here and in run_mfma): the result (indices, distances) has been written through `fo` already -- no finalize
// launch; else it is the keys in d_keys_out
int run_exact(gloc_knn* h, const float* d_q, int nq, int k, size_t first, int n_range, uint64_t* d_keys_out,
              const FinalOut& fo, bool* through_fo) {
  const size_t ld = ((size_t)n_range + 63) & ~(size_t)63;
  const SelectPlan sp = plan_select(n_range, nq, k);
  GLOC_TRY(h->dist.ensure((size_t)nq * ld * sizeof(float), h->stream));
  GLOC_TRY(launch_dist_exact(h, d_q, nq, first, n_range, ld));
  GLOC_TRY(run_select<0>(h, sp, d_q, nq, k, first, n_range, ld, 0, 1, d_keys_out, nullptr, fo));
  *through_fo = fo.idx && sp.form != Selection::Chunks;
  return GLOC_OK;
}

// ---- MFMA path -------------------------------------------------------------------------------
// The split-bf16 coarse pass over the mirror.  Its LDS image may exceed the 48-KB default, and the attribute that allows
// more belongs to the device's copy of the kernel: set once per kernel and device.
template <auto KERNEL>
int allow_lds(int device, int bytes) {
  static std::atomic<uint64_t> done{0};  // bit d: set on device d
  const uint64_t bit = 1ull << (device & 63);
  if (bytes > 48 * 1024 && !(done.load(std::memory_order_relaxed) & bit)) {
    GLOC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    done.fetch_or(bit, std::memory_order_relaxed);
  }
  return GLOC_OK;
}
template <int NT, bool QRAW, bool BMIN>
int launch_bf16x3(gloc_knn* h, const SearchPlan& p, dim3 grid, const float* qsrc, size_t first, int n_range, int nq) {
  constexpr int lds_bytes = b3_lds_bytes<NT>();
  GLOC_TRY((allow_lds<dist_bf16x3_tiled_kernel<NT, QRAW, BMIN>>(h->device, lds_bytes)));
  hipLaunchKernelGGL((dist_bf16x3_tiled_kernel<NT, QRAW, BMIN>), grid, dim3(256), lds_bytes, h->stream, h->db->mirror.as<u32x4>(),
                     qsrc, h->dist.as<float>(), (int)h->dim, first, n_range, nq, p.kps, p.ld, p.strideP,
                     BMIN ? h->db->norms.as<float>() : (const float*)nullptr, BMIN ? h->bmin.as<float>() : (float*)nullptr,
                     BMIN ? p.n_blocks : 0);
  return GLOC_OK;
}

// The steps of a coarse search, in the order run_mfma takes them; every decision is the plan's (knn_plan.hpp).
// 1. the workspaces (the slices' and the redo's lists are sized where they are launched)
int ensure_search_ws(gloc_knn* h, const SearchPlan& p, int nq) {
  GLOC_TRY(h->dist.ensure((size_t)p.tile.KS * p.strideP * sizeof(float), h->stream));
  GLOC_TRY(h->qnorm.ensure((size_t)nq * sizeof(float), h->stream));
  GLOC_TRY(h->keys.ensure((size_t)nq * p.KC * sizeof(uint64_t), h->stream));
  GLOC_TRY(h->flags.ensure((size_t)nq * sizeof(int), h->stream));
  if (!h->n_incomplete.p) {
    GLOC_TRY(h->n_incomplete.ensure(sizeof(unsigned long long), h->stream));
    GLOC_HIP(hipMemsetAsync(h->n_incomplete.p, 0, sizeof(unsigned long long), h->stream));
  }
  if (p.tile.b3 && !p.qraw) GLOC_TRY(h->qsplit.ensure((size_t)nq * h->dim * sizeof(float), h->stream));
  if (p.use_bmin) {
    GLOC_TRY(h->bmin.ensure((size_t)nq * p.n_blocks * sizeof(float), h->stream));
    GLOC_TRY(h->klists.ensure((size_t)nq * SELB_LIST * sizeof(uint64_t), h->stream));
  }
  if (!p.fused) GLOC_TRY(h->exact.ensure((size_t)nq * p.KC * sizeof(float), h->stream));
  return GLOC_OK;
}

// 2. the coarse pass: the partial dots of every (K split, query, row) into h->dist
int coarse_pass(gloc_knn* h, const SearchPlan& p, const float* d_q, int nq, size_t first, int n_range) {
  const dim3 grid(p.gx, p.gy, p.gz);
  const float* qsrc = d_q;
  if (p.tile.b3 && !p.qraw) {
    ProfScope ps(h->prof, "split_queries", h->stream);
    const size_t n8 = (size_t)nq * h->dim / 8;
    hipLaunchKernelGGL(split_queries_kernel, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, h->stream, d_q, n8,
                       h->qsplit.as<float>());
    qsrc = h->qsplit.as<float>();
  }
  ProfScope ps(h->prof, "dist_mfma", h->stream);
  if (p.tile.b3) {
    // the rows from their tiled, pre-split mirror (round 6), which every add keeps when dim % 8 == 0
    GLOC_REQUIRE(h->db->mirror.p, GLOC_ERR_STATE, "internal: the split-bf16 coarse pass without the rows' mirror");
#define B3T(NT_, QR_) \
  (p.use_bmin ? launch_bf16x3<NT_, QR_, true>(h, p, grid, qsrc, first, n_range, nq) : launch_bf16x3<NT_, QR_, false>(h, p, grid, qsrc, first, n_range, nq))
    if (p.tile.NT == 1) GLOC_TRY(p.qraw ? B3T(1, true) : B3T(1, false));
    else GLOC_TRY(p.qraw ? B3T(2, true) : B3T(2, false));
#undef B3T
  } else {
    // the fp32 forms: plan_mfma's one 32 x 32 plan (NT = 2, steps of 32 k), else the 16 x 16 tiles <WQ, NT> in steps of 32 or 64 k
#define FP32(...)                                                                                                       \
  hipLaunchKernelGGL((__VA_ARGS__), grid, dim3(256), 0, h->stream, h->db->rows.as<float>(), d_q, h->dist.as<float>(), \
                     (int)h->dim, first, n_range, nq, p.kps, p.ld, p.strideP)
#define MF(WQ_, NT_)                                                   \
  if (p.tile.WQ == WQ_ && p.tile.NT == NT_) {                          \
    if (p.kps < 128) FP32(dist_mfma_kernel<WQ_, NT_, 8>);              \
    else FP32(dist_mfma_kernel<WQ_, NT_, 16>);                         \
  } else
    if (p.tile.t32) FP32(dist_mfma32_kernel<2, 8>);
    else MF(4, 2) MF(4, 3) MF(4, 4) MF(4, 5) MF(4, 6) MF(4, 8) MF(2, 2) MF(2, 4) MF(1, 1) MF(1, 2) {
      set_err("internal: no MFMA instance for WQ=%d NT=%d", p.tile.WQ, p.tile.NT);
      return GLOC_ERR_STATE;
    }
#undef FP32
#undef MF
  }
  GLOC_HIP(hipGetLastError());
  return GLOC_OK;
}

// 3. selection, re-rank and completeness check: the keys in d_keys_out, the unproven queries' flags in h->flags.
// Fused: ONE launch, one work-group per query, which also writes the result through `fo`.
int select_rerank_fused(gloc_knn* h, const SearchPlan& p, const float* d_q, int nq, int k, size_t first, int n_range,
                        uint64_t* d_keys_out, const FinalOut& fo) {
  if (p.sel.form == Selection::Slices) {
    ProfScope ps(h->prof, "select", h->stream);
    GLOC_TRY(launch_slices<1>(h, d_q, nq, p.KC, first, n_range, p.ld, p.strideP, p.tile.KS, p.sel.sl, nullptr));
  }
  ProfScope ps(h->prof, "select_rerank", h->stream);
#define SRR_ARGS                                                                                                          \
  dim3(nq), dim3(SELQ_THREADS), 0, h->stream, h->dist.as<float>(), p.ld, p.strideP, p.tile.KS, d_q, (int)h->dim,         \
      h->db->norms.as<float>(), first, n_range, p.KC, k, h->db->rows.as<float>(), h->db->dn_max.as<uint32_t>(), p.eps_rel_d, p.eps_rel_n, \
      h->qnorm.as<float>(), d_keys_out, h->flags.as<int>(), h->n_incomplete.as<unsigned long long>(), fo,                \
      h->dist.as<float>()
  switch (p.sel.form) {
    case Selection::BlockMinima:  // selected inside the launch itself (select_blocks_body), which leaves the blocks' keys in h->klists
      hipLaunchKernelGGL(select_rerank_kernel<true>, SRR_ARGS, h->klists.as<uint64_t>(), SELB_LIST, h->bmin.as<float>(), p.n_blocks,
                         h->klists.as<uint64_t>());
      break;
    case Selection::Slices:  // from their lists
      hipLaunchKernelGGL(select_rerank_kernel<true>, SRR_ARGS, h->klists.as<uint64_t>(), p.sel.sl.S * p.KC, (const float*)nullptr,
                         p.n_blocks, h->klists.as<uint64_t>());
      break;
    default:  // Window: from the partial dots
      hipLaunchKernelGGL(select_rerank_kernel<false>, SRR_ARGS, (const uint64_t*)nullptr, 0, (const float*)nullptr, 0, (uint64_t*)nullptr);
  }
#undef SRR_ARGS
  GLOC_HIP(hipGetLastError());
  return GLOC_OK;
}

// Not fused (more than SRR_KC candidates, dim > 4 * SRR_G, or a window whose slices' lists fit no work-group): launch by launch
int select_then_rerank(gloc_knn* h, const SearchPlan& p, const float* d_q, int nq, int k, size_t first, int n_range,
                       uint64_t* d_keys_out) {
  // (the query norms of the coarse form are made by the select kernel, which leaves them in h->qnorm)
  GLOC_TRY(run_select<1>(h, p.sel, d_q, nq, p.KC, first, n_range, p.ld, p.strideP, p.tile.KS, h->keys.as<uint64_t>()));
  ProfScope ps(h->prof, "rerank", h->stream);
  hipLaunchKernelGGL(rerank_dist_kernel, dim3((p.KC + RR - 1) / RR, nq), dim3(64), 0, h->stream,
                     h->db->rows.as<float>(), d_q, (int)h->dim, h->keys.as<uint64_t>(), p.KC, k,
                     h->qnorm.as<float>(), h->db->dn_max.as<uint32_t>(), p.eps_rel_d, p.eps_rel_n,
                     h->exact.as<float>());
  hipLaunchKernelGGL(rerank_final_kernel, dim3(nq), dim3(64), 0, h->stream,
                     h->keys.as<uint64_t>(), h->exact.as<float>(), p.KC, k, n_range,
                     h->qnorm.as<float>(), h->db->dn_max.as<uint32_t>(), p.eps_rel_d, p.eps_rel_n,
                     d_keys_out, h->flags.as<int>(), h->n_incomplete.as<unsigned long long>());
  GLOC_HIP(hipGetLastError());
  return GLOC_OK;
}

// 4. the redo of the unproven queries behind a search that has not done it in its own launch (Redo::InLaunch), in one of
// three forms.  (The coarse partial dots in h->dist are dead by now: the exact distances of the flagged queries reuse
// the buffer, row q at q * ld.)
int redo_one_launch(gloc_knn* h, const SearchPlan& p, const float* d_q, int nq, int k, size_t first, int n_range,
                    uint64_t* d_keys_out, const FinalOut& fo) {
  const SlicePlan& sl = p.redo.sl;
  const size_t before = h->redo_tickets.cap;
  GLOC_TRY(h->redo_tickets.ensure((size_t)nq * sizeof(unsigned int), h->stream));
  if (h->redo_tickets.cap != before) GLOC_HIP(hipMemsetAsync(h->redo_tickets.p, 0, h->redo_tickets.cap, h->stream));
  GLOC_TRY(h->klists.ensure((size_t)nq * sl.S * k * sizeof(uint64_t), h->stream));
  ProfScope ps(h->prof, "dist_exact", h->stream);
  hipLaunchKernelGGL(flagged_redo_kernel, dim3((unsigned)sl.S), dim3(SELQ_THREADS), 0, h->stream, h->db->rows.as<float>(), d_q,
                     (int)h->dim, first, n_range, sl.L, k, h->dist.as<float>(), p.ld, h->klists.as<uint64_t>(),
                     h->redo_tickets.as<unsigned int>(), h->flags.as<int>(), nq, d_keys_out, fo);
  GLOC_HIP(hipGetLastError());
  return GLOC_OK;
}

int redo_flagged_exact(gloc_knn* h, const SearchPlan& p, const float* d_q, int nq, int k, size_t first, int n_range,
                       uint64_t* d_keys_out, const FinalOut& fo) {
  GLOC_TRY(launch_dist_exact(h, d_q, nq, first, n_range, p.ld, h->flags.as<int>()));
  // (behind the fused launch, which has written the result through `fo`: the flagged queries' is replaced there too)
  return run_select<0>(h, p.redo, d_q, nq, k, first, n_range, p.ld, 0, 1, d_keys_out, h->flags.as<int>(), p.fused ? fo : KEYS_ONLY);
}

// Reached only when the lists of the redo's slices no longer fit one work-group, S * k > 16 384 -- by plan_slices a
// window above roughly 5 million rows at k = 52 (16 384 / 52 = 315 slices of 16 384 rows): the completeness flags go to the
// host behind a synchronisation, and each flagged query takes the exact path on its own, leaving keys.
int redo_on_host(gloc_knn* h, const float* d_q, int nq, int k, size_t first, int n_range, uint64_t* d_keys_out, bool* redone) {
  if (h->h_flags_cap < (size_t)nq) {
    if (h->h_flags) (void)hipHostFree(h->h_flags);
    h->h_flags = nullptr;
    GLOC_HIP(hipHostMalloc((void**)&h->h_flags, sizeof(int) * (size_t)nq * 2));
    h->h_flags_cap = (size_t)nq * 2;
  }
  GLOC_HIP(hipMemcpyAsync(h->h_flags, h->flags.p, sizeof(int) * (size_t)nq,
                          hipMemcpyDeviceToHost, h->stream));
  GLOC_HIP(hipStreamSynchronize(h->stream));
  for (int q = 0; q < nq; ++q) {
    if (h->h_flags[q]) {
      bool ignored;  // (keys only: nothing goes through a FinalOut here)
      GLOC_TRY(run_exact(h, d_q + (size_t)q * h->dim, 1, k, first, n_range, d_keys_out + (size_t)q * k, KEYS_ONLY, &ignored));
      *redone = true;
    }
  }
  return GLOC_OK;
}

int run_mfma(gloc_knn* h, const float* d_q, int nq, int k, size_t first, int n_range, uint64_t* d_keys_out,
             const FinalOut& fo, bool fp32_only, bool* through_fo) {
  const SearchPlan p = plan_search(nq, n_range, (int)(first % MIR_ROWS), (int)h->dim, k, h->candidates, fp32_only);
  GLOC_TRY(ensure_search_ws(h, p, nq));
  GLOC_TRY(coarse_pass(h, p, d_q, nq, first, n_range));
  GLOC_TRY(p.fused ? select_rerank_fused(h, p, d_q, nq, k, first, n_range, d_keys_out, fo)
                   : select_then_rerank(h, p, d_q, nq, k, first, n_range, d_keys_out));
  h->stats.last_n_tile = (uint32_t)p.tile.BN;
  h->stats.last_k_split = (uint32_t)p.tile.KS;
  h->stats.last_candidates = (uint32_t)p.KC;
  bool redone_on_host = false;
  switch (p.how_redo) {
    case Redo::InLaunch: break;
    case Redo::OneLaunch: GLOC_TRY(redo_one_launch(h, p, d_q, nq, k, first, n_range, d_keys_out, fo)); break;
    case Redo::FlaggedExact: GLOC_TRY(redo_flagged_exact(h, p, d_q, nq, k, first, n_range, d_keys_out, fo)); break;
    case Redo::HostReadBack: GLOC_TRY(redo_on_host(h, d_q, nq, k, first, n_range, d_keys_out, &redone_on_host)); break;
  }
  // the fused launch and the device redos behind it write through `fo`; the re-rank kernels and the host's redo leave keys
  *through_fo = p.fused && !redone_on_host;
  return GLOC_OK;
}

int search_device_impl(gloc_knn* h, const float* d_q, size_t nq, size_t k, size_t first_row,
                       size_t last_row, uint64_t index_offset, uint64_t* d_idx, float* d_d2,
                       uint64_t index_stride = 1) {
  GLOC_REQUIRE(h && d_q && d_idx && d_d2, GLOC_ERR_INVALID, "null argument");
  GLOC_REQUIRE(k >= 1 && k <= 256, GLOC_ERR_INVALID, "k = %zu outside [1,256]", k);
  GLOC_REQUIRE(nq >= 1 && nq <= (1u << 20), GLOC_ERR_INVALID, "nq = %zu outside [1,2^20]", nq);
  GLOC_HIP(hipSetDevice(h->device));
  if (last_row > h->db->n) last_row = h->db->n;
  if (first_row > last_row) first_row = last_row;
  const size_t range = last_row - first_row;
  GLOC_REQUIRE(range < (1ull << 31), GLOC_ERR_INVALID, "row window too large");
  GLOC_TRY(h->keys2.ensure(nq * k * sizeof(uint64_t), h->stream));
  uint64_t* keys_out = h->keys2.as<uint64_t>();
  bool all_final = true;  // every block of queries left its result in d_idx / d_d2 itself
  if (range == 0) {
    all_final = false;
    GLOC_HIP(hipMemsetAsync(keys_out, 0xFF, nq * k * sizeof(uint64_t), h->stream));
  } else {
    int algo = h->algo;
    const bool mfma_ok = (h->dim % 4 == 0) && k <= 52 && range >= 64;
    if (algo == GLOC_KNN_ALGO_AUTO) algo = (nq > 8 && mfma_ok) ? GLOC_KNN_ALGO_MFMA : GLOC_KNN_ALGO_EXACT;
    if ((algo == GLOC_KNN_ALGO_MFMA || algo == GLOC_KNN_ALGO_MFMA_FP32) && !mfma_ok) algo = GLOC_KNN_ALGO_EXACT;
    // process queries in blocks that bound the distance workspace (<= 2 GiB)
    const size_t ld = (range + 63) & ~(size_t)63;
    size_t qblk = (size_t)(2ull << 30) / (ld * sizeof(float) * 4);
    qblk = std::min<size_t>(1024, std::max<size_t>(64, qblk / 64 * 64));
    // the coarse form of this search (see h_inc): look at the last tracked search's count if its copy has landed
    bool tracked = false;
    if (algo == GLOC_KNN_ALGO_MFMA) {
      if (h->inc_pending && hipEventQuery(h->inc_ev) == hipSuccess) {
        const unsigned long long now = *h->h_inc, delta = now - h->inc_seen;
        h->inc_seen = now;
        h->inc_pending = false;
        if (delta * 4 > h->inc_queries) h->coarse_fp32_left = 64;
      }
      if (h->coarse_fp32_left > 0) {
        h->coarse_fp32_left--;
        algo = GLOC_KNN_ALGO_MFMA_FP32;
      } else {
        tracked = !h->inc_pending;
      }
    }
    const bool coarse = algo == GLOC_KNN_ALGO_MFMA || algo == GLOC_KNN_ALGO_MFMA_FP32;
    for (size_t q0 = 0; q0 < nq; q0 += qblk) {
      const int cnt = (int)std::min(qblk, nq - q0);
      const FinalOut fo{d_idx + q0 * k, d_d2 + q0 * k, index_offset, index_stride};
      bool fin = false;
      (coarse ? h->stats.searches_mfma : h->stats.searches_exact)++;
      GLOC_TRY(coarse ? run_mfma(h, d_q + q0 * h->dim, cnt, (int)k, first_row, (int)range, keys_out + q0 * k, fo,
                                 algo == GLOC_KNN_ALGO_MFMA_FP32, &fin)
                      : run_exact(h, d_q + q0 * h->dim, cnt, (int)k, first_row, (int)range, keys_out + q0 * k, fo, &fin));
      all_final = all_final && fin;
    }
    if (tracked && h->n_incomplete.p) {  // the fallback count as of this search, for the next one to look at
      if (!h->h_inc) {
        GLOC_HIP(hipHostMalloc((void**)&h->h_inc, sizeof(unsigned long long)));
        *h->h_inc = 0;
        GLOC_HIP(hipEventCreateWithFlags(&h->inc_ev, hipEventDisableTiming));
      }
      GLOC_HIP(hipMemcpyAsync(h->h_inc, h->n_incomplete.p, sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
      GLOC_HIP(hipEventRecord(h->inc_ev, h->stream));
      h->inc_pending = true;
      h->inc_queries = nq;
    }
  }
  h->stats.queries_total += nq;
  if (!all_final) {
    ProfScope ps(h->prof, "finalize", h->stream);
    const size_t total = nq * k;
    hipLaunchKernelGGL(finalize_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                       h->stream, keys_out, total, index_offset, index_stride, d_idx, d_d2);
    GLOC_HIP(hipGetLastError());
  }
  return GLOC_OK;
}

}  // namespace

extern "C" {

int gloc_knn_create(int device, size_t dim, gloc_knn** out) {
  GLOC_REQUIRE(out, GLOC_ERR_INVALID, "out is null");
  *out = nullptr;
  GLOC_REQUIRE(dim >= 1 && dim <= (1u << 20), GLOC_ERR_INVALID, "dim = %zu outside [1,2^20]", dim);
  GLOC_TRY(create_handle(device, out));
  (*out)->dim = dim;
  return GLOC_OK;
}

int gloc_knn_create_view(gloc_knn* parent, gloc_knn** out) {
  GLOC_REQUIRE(parent && out, GLOC_ERR_INVALID, "null argument");
  *out = nullptr;
  GLOC_REQUIRE(!parent->parent, GLOC_ERR_INVALID, "a view of a view: take it of the owning handle");
  gloc_knn* v = nullptr;
  GLOC_TRY(gloc_knn_create(parent->device, parent->dim, &v));
  v->parent = parent;
  v->algo = parent->algo;
  v->candidates = parent->candidates;
  parent->views++;
  v->db = &parent->own;
  *out = v;
  return GLOC_OK;
}

int gloc_knn_destroy(gloc_knn* h) {
  if (!h) return GLOC_OK;
  GLOC_REQUIRE(h->views == 0, GLOC_ERR_STATE, "%d view(s) of this handle are still alive (gloc_knn_create_view): destroy them first", h->views);
  if (h->parent) h->parent->views--;
  return destroy_handle(h);
}

int gloc_knn_set_stream(gloc_knn* h, void* hip_stream) { return handle_set_stream(h, hip_stream); }

int gloc_knn_synchronize(gloc_knn* h) { return handle_synchronize(h); }

int gloc_knn_set_option(gloc_knn* h, int option, int64_t value) {
  GLOC_REQUIRE(h, GLOC_ERR_INVALID, "null handle");
  switch (option) {
    case GLOC_KNN_OPT_ALGO:
      GLOC_REQUIRE(value >= 0 && value <= 3, GLOC_ERR_INVALID, "bad algorithm %lld", (long long)value);
      h->algo = (int)value;
      return GLOC_OK;
    case GLOC_KNN_OPT_CANDIDATES:
      GLOC_REQUIRE(value >= 1 && value <= 64, GLOC_ERR_INVALID, "candidates %lld outside [1,64]",
                   (long long)value);
      h->candidates = (int)value;
      return GLOC_OK;
    case GLOC_KNN_OPT_PROFILE:
      h->prof.enabled = value != 0;
      return GLOC_OK;
    default:
      set_err("unknown option %d", option);
      return GLOC_ERR_INVALID;
  }
}

int gloc_knn_reserve(gloc_knn* h, size_t n_rows) {
  GLOC_REQUIRE(h, GLOC_ERR_INVALID, "null handle");
  GLOC_HIP(hipSetDevice(h->device));
  return ensure_rows(h, n_rows);
}

int gloc_knn_add(gloc_knn* h, const float* rows, size_t n) {
  GLOC_REQUIRE(h && (rows || n == 0), GLOC_ERR_INVALID, "null argument");
  if (n == 0) return GLOC_OK;
  GLOC_REQUIRE(h->db->n + n < (1ull << 32) - 1, GLOC_ERR_INVALID, "database limited to 2^32-2 rows");
  GLOC_HIP(hipSetDevice(h->device));
  GLOC_TRY(ensure_rows(h, h->db->n + n));
  GLOC_HIP(hipMemcpyAsync(h->db->rows.as<float>() + h->db->n * h->dim, rows, n * h->dim * sizeof(float),
                          hipMemcpyHostToDevice, h->stream));
  GLOC_TRY(update_norms(h, h->db->n, n));
  GLOC_HIP(hipStreamSynchronize(h->stream));  // the caller may free `rows` on return
  h->db->n += n;
  return GLOC_OK;
}

int gloc_knn_add_device(gloc_knn* h, const float* d_rows, size_t n) {
  GLOC_REQUIRE(h && (d_rows || n == 0), GLOC_ERR_INVALID, "null argument");
  if (n == 0) return GLOC_OK;
  GLOC_REQUIRE(h->db->n + n < (1ull << 32) - 1, GLOC_ERR_INVALID, "database limited to 2^32-2 rows");
  GLOC_HIP(hipSetDevice(h->device));
  GLOC_TRY(ensure_rows(h, h->db->n + n));
  GLOC_HIP(hipMemcpyAsync(h->db->rows.as<float>() + h->db->n * h->dim, d_rows,
                          n * h->dim * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
  GLOC_TRY(update_norms(h, h->db->n, n));
  h->db->n += n;
  return GLOC_OK;
}

int gloc_knn_add_synthetic(gloc_knn* h, int kind, uint64_t seed, uint64_t first_row, size_t n,
                           uint64_t row_stride) {
  GLOC_REQUIRE(h, GLOC_ERR_INVALID, "null handle");
  GLOC_REQUIRE(kind == 0 || kind == 1, GLOC_ERR_INVALID, "kind must be 0 (iid) or 1 (trajectory)");
  if (n == 0) return GLOC_OK;
  GLOC_REQUIRE(h->db->n + n < (1ull << 32) - 1, GLOC_ERR_INVALID, "database limited to 2^32-2 rows");
  GLOC_HIP(hipSetDevice(h->device));
  GLOC_TRY(ensure_rows(h, h->db->n + n));
  gloc::synth::launch_fill(h->stream, kind, seed, first_row, n, h->dim, row_stride ? row_stride : 1,
                           h->db->rows.as<float>() + h->db->n * h->dim);
  GLOC_HIP(hipGetLastError());
  GLOC_TRY(update_norms(h, h->db->n, n));
  h->db->n += n;
  return GLOC_OK;
}

int gloc_synth_fill_device(int device, void* hip_stream, int kind, uint64_t seed,
                           uint64_t first_row, size_t n, size_t dim, uint64_t row_stride,
                           float* d_out) {
  GLOC_REQUIRE(d_out || n == 0, GLOC_ERR_INVALID, "null output");
  GLOC_REQUIRE(kind == 0 || kind == 1, GLOC_ERR_INVALID, "kind must be 0 (iid) or 1 (trajectory)");
  GLOC_TRY(select_device(device));
  if (n == 0) return GLOC_OK;
  gloc::synth::launch_fill((hipStream_t)hip_stream, kind, seed, first_row, n, dim,
                           row_stride ? row_stride : 1, d_out);
  GLOC_HIP(hipGetLastError());
  return GLOC_OK;
}

int gloc_knn_clear(gloc_knn* h) {
  GLOC_REQUIRE(h, GLOC_ERR_INVALID, "null handle");
  GLOC_NOT_VIEW(h);
  GLOC_HIP(hipSetDevice(h->device));
  GLOC_HIP(hipStreamSynchronize(h->stream));
  h->db->n = 0;
  if (h->db->dn_max.p) GLOC_HIP(hipMemsetAsync(h->db->dn_max.p, 0, sizeof(uint32_t), h->stream));
  return GLOC_OK;
}

int gloc_knn_size(const gloc_knn* h, size_t* n_rows) {
  GLOC_REQUIRE(h && n_rows, GLOC_ERR_INVALID, "null argument");
  *n_rows = h->db->n;
  return GLOC_OK;
}

int gloc_knn_dim(const gloc_knn* h, size_t* dim) {
  GLOC_REQUIRE(h && dim, GLOC_ERR_INVALID, "null argument");
  *dim = h->dim;
  return GLOC_OK;
}

int gloc_knn_device_rows(const gloc_knn* h, const float** d_rows) {
  GLOC_REQUIRE(h && d_rows, GLOC_ERR_INVALID, "null argument");
  *d_rows = h->db->rows.as<float>();
  return GLOC_OK;
}

int gloc_knn_save(gloc_knn* h, const char* path) {
  GLOC_REQUIRE(h && path, GLOC_ERR_INVALID, "null argument");
  GLOC_HIP(hipSetDevice(h->device));
  FILE* f = fopen(path, "wb");
  GLOC_REQUIRE(f, GLOC_ERR_INVALID, "cannot open %s for writing", path);
  const uint32_t hdr[2] = {(uint32_t)h->db->n, (uint32_t)h->dim};
  bool ok = fwrite("GLOCDESC", 1, 8, f) == 8 && fwrite(hdr, 4, 2, f) == 2;
  std::vector<float> buf;
  const size_t chunk = std::max<size_t>(1, (64u << 20) / (h->dim * sizeof(float)));  // 64 MiB pieces
  for (size_t r = 0; ok && r < h->db->n; r += chunk) {
    const size_t cnt = std::min(chunk, h->db->n - r);
    buf.resize(cnt * h->dim);
    if (hipMemcpyAsync(buf.data(), h->db->rows.as<float>() + r * h->dim, buf.size() * sizeof(float),
                       hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
        hipStreamSynchronize(h->stream) != hipSuccess)
      ok = false;
    else
      ok = fwrite(buf.data(), sizeof(float), buf.size(), f) == buf.size();
  }
  ok = (fclose(f) == 0) && ok;
  GLOC_REQUIRE(ok, GLOC_ERR_STATE, "writing %s failed", path);
  return GLOC_OK;
}

int gloc_knn_load(gloc_knn* h, const char* path) {
  GLOC_REQUIRE(h && path, GLOC_ERR_INVALID, "null argument");
  FILE* f = fopen(path, "rb");
  GLOC_REQUIRE(f, GLOC_ERR_INVALID, "cannot open %s", path);
  char magic[8];
  uint32_t hdr[2] = {0, 0};
  if (fread(magic, 1, 8, f) != 8 || memcmp(magic, "GLOCDESC", 8) != 0 || fread(hdr, 4, 2, f) != 2) {
    fclose(f);
    set_err("%s is not a GLOCDESC file", path);
    return GLOC_ERR_INVALID;
  }
  if (hdr[1] != h->dim) {
    fclose(f);
    set_err("%s holds %u-D rows, the index is %zu-D", path, hdr[1], h->dim);
    return GLOC_ERR_INVALID;
  }
  // the header must agree with the file's size before a single row is added
  const long pos = ftell(f);
  if (pos < 0 || fseek(f, 0, SEEK_END) != 0) {
    fclose(f);
    set_err("cannot size %s", path);
    return GLOC_ERR_INVALID;
  }
  const long end = ftell(f);
  if (end < 0 || (unsigned long long)(end - pos) < (unsigned long long)hdr[0] * h->dim * sizeof(float)) {
    fclose(f);
    set_err("%s is truncated: the header announces %u rows", path, hdr[0]);
    return GLOC_ERR_INVALID;
  }
  (void)fseek(f, pos, SEEK_SET);
  std::vector<float> buf;
  const size_t chunk = std::max<size_t>(1, (64u << 20) / (h->dim * sizeof(float)));
  const size_t n0 = h->db->n;  // on any failure below the index is rolled back to this many rows
  int rc = GLOC_OK;
  for (size_t r = 0; rc == GLOC_OK && r < hdr[0]; r += chunk) {
    const size_t cnt = std::min<size_t>(chunk, hdr[0] - r);
    buf.resize(cnt * h->dim);
    if (fread(buf.data(), sizeof(float), buf.size(), f) != buf.size()) {
      set_err("%s is truncated", path);
      rc = GLOC_ERR_INVALID;
    } else {
      rc = gloc_knn_add(h, buf.data(), cnt);
    }
  }
  fclose(f);
  if (rc != GLOC_OK) h->db->n = n0;  // (the running maximum norm may stay larger: it only widens the re-rank window)
  return rc;
}

int gloc_knn_search_device(gloc_knn* h, const float* d_queries, size_t nq, size_t k,
                           size_t first_row, size_t last_row, uint64_t index_offset,
                           uint64_t* d_out_idx, float* d_out_d2) {
  GLOC_REQUIRE(h, GLOC_ERR_INVALID, "null handle");
  return search_device_impl(h, d_queries, nq, k, first_row, last_row, index_offset, d_out_idx,
                            d_out_d2);
}

int gloc_knn_search_sharded(gloc_knn* h, gloc_comm* comm, const float* d_queries, size_t nq, size_t k,
                            uint64_t index_stride, uint64_t index_offset, uint64_t* d_out_idx,
                            float* d_out_d2) {
  GLOC_REQUIRE(h && comm && d_queries && d_out_idx && d_out_d2, GLOC_ERR_INVALID, "null argument");
  GLOC_REQUIRE(comm->device == h->device, GLOC_ERR_INVALID, "communicator on device %d, index on %d", comm->device,
               h->device);
  GLOC_REQUIRE(index_stride >= 1, GLOC_ERR_INVALID, "index_stride must be >= 1");
  GLOC_REQUIRE((size_t)comm->world * k <= 1024, GLOC_ERR_INVALID, "shards x k = %zu exceeds 1024",
               (size_t)comm->world * k);
  const size_t G = (size_t)comm->world, cnt = nq * k;
  // [local idx | local d2 | gathered idx | gathered d2]
  GLOC_TRY(h->shard_ws.ensure(cnt * 12 + G * cnt * 12 + 64, h->stream));
  uint64_t* li = h->shard_ws.as<uint64_t>();
  uint64_t* gi = li + cnt;
  float* ld = reinterpret_cast<float*>(gi + G * cnt);
  float* gd = ld + cnt;
  // this shard's top-k with GLOBAL row indices ...  (profile families: shard_local / shard_gather / shard_merge)
  {
    ProfScope ps(h->prof, "shard_local", h->stream);
    GLOC_TRY(search_device_impl(h, d_queries, nq, k, 0, (size_t)-1, index_offset, li, ld, index_stride));
  }
  if (G == 1) {
    GLOC_HIP(hipMemcpyAsync(d_out_idx, li, cnt * sizeof(uint64_t), hipMemcpyDeviceToDevice, h->stream));
    GLOC_HIP(hipMemcpyAsync(d_out_d2, ld, cnt * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    return GLOC_OK;
  }
  // ... all-gathered over xGMI: one fused launch for the two small arrays ([shard][nq][k], what K3 reads) ...
  {
    ProfScope ps(h->prof, "shard_gather", h->stream);
    GLOC_TRY(gloc::comm::group_begin());
    int rc = gloc::comm::all_gather(comm, li, gi, cnt * sizeof(uint64_t), h->stream);
    if (rc == GLOC_OK) rc = gloc::comm::all_gather(comm, ld, gd, cnt * sizeof(float), h->stream);
    const int rc2 = gloc::comm::group_end();
    GLOC_TRY(rc);
    GLOC_TRY(rc2);
  }
  // ... and merged on every rank in the same (d2, idx) order: a replicated result, equal to the one-GPU search
  ProfScope ps(h->prof, "shard_merge", h->stream);
  hipLaunchKernelGGL(merge_kernel, dim3((unsigned)nq), dim3(64), 0, h->stream, gi, gd, (int)G, (int)nq, (int)k,
                     d_out_idx, d_out_d2);
  GLOC_HIP(hipGetLastError());
  return GLOC_OK;
}

int gloc_knn_search_sharded_host(gloc_knn* h, gloc_comm* comm, const float* queries, size_t nq, size_t k,
                                 uint64_t index_stride, uint64_t index_offset, uint64_t* out_idx, float* out_d2) {
  GLOC_REQUIRE(h && queries && out_idx && out_d2, GLOC_ERR_INVALID, "null argument");
  GLOC_REQUIRE(k >= 1 && k <= 256 && nq >= 1 && nq <= (1u << 20), GLOC_ERR_INVALID, "bad nq / k");
  GLOC_NOT_VIEW(h);
  GLOC_HIP(hipSetDevice(h->device));
  GLOC_TRY(h->stage_q.ensure(nq * h->dim * sizeof(float), h->stream));
  GLOC_TRY(h->stage_idx.ensure(nq * k * sizeof(uint64_t), h->stream));
  GLOC_TRY(h->stage_d2.ensure(nq * k * sizeof(float), h->stream));
  GLOC_HIP(hipMemcpyAsync(h->stage_q.p, queries, nq * h->dim * sizeof(float), hipMemcpyHostToDevice, h->stream));
  GLOC_TRY(gloc_knn_search_sharded(h, comm, h->stage_q.as<float>(), nq, k, index_stride, index_offset,
                                   h->stage_idx.as<uint64_t>(), h->stage_d2.as<float>()));
  GLOC_HIP(hipMemcpyAsync(out_idx, h->stage_idx.p, nq * k * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
  GLOC_HIP(hipMemcpyAsync(out_d2, h->stage_d2.p, nq * k * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  GLOC_HIP(hipStreamSynchronize(h->stream));
  return GLOC_OK;
}

int gloc_knn_search(gloc_knn* h, const float* queries, size_t nq, size_t k, size_t first_row,
                    size_t last_row, uint64_t* out_idx, float* out_d2) {
  GLOC_REQUIRE(h && queries && out_idx && out_d2, GLOC_ERR_INVALID, "null argument");
  GLOC_REQUIRE(k >= 1 && k <= 256, GLOC_ERR_INVALID, "k = %zu outside [1,256]", k);
  GLOC_REQUIRE(nq >= 1 && nq <= (1u << 20), GLOC_ERR_INVALID, "nq = %zu outside [1,2^20]", nq);
  GLOC_HIP(hipSetDevice(h->device));
  GLOC_TRY(h->stage_q.ensure(nq * h->dim * sizeof(float), h->stream));
  GLOC_TRY(h->stage_idx.ensure(nq * k * sizeof(uint64_t), h->stream));
  GLOC_TRY(h->stage_d2.ensure(nq * k * sizeof(float), h->stream));
  GLOC_HIP(hipMemcpyAsync(h->stage_q.p, queries, nq * h->dim * sizeof(float),
                          hipMemcpyHostToDevice, h->stream));
  GLOC_TRY(search_device_impl(h, h->stage_q.as<float>(), nq, k, first_row, last_row, 0,
                              h->stage_idx.as<uint64_t>(), h->stage_d2.as<float>()));
  GLOC_HIP(hipMemcpyAsync(out_idx, h->stage_idx.p, nq * k * sizeof(uint64_t),
                          hipMemcpyDeviceToHost, h->stream));
  GLOC_HIP(hipMemcpyAsync(out_d2, h->stage_d2.p, nq * k * sizeof(float), hipMemcpyDeviceToHost,
                          h->stream));
  GLOC_HIP(hipStreamSynchronize(h->stream));
  return GLOC_OK;
}

int gloc_topk_merge_device(int device, void* hip_stream, const uint64_t* d_idx, const float* d_d2,
                           size_t n_lists, size_t nq, size_t k, uint64_t* d_out_idx,
                           float* d_out_d2) {
  GLOC_REQUIRE(d_idx && d_d2 && d_out_idx && d_out_d2, GLOC_ERR_INVALID, "null argument");
  GLOC_REQUIRE(n_lists >= 1 && k >= 1 && n_lists * k <= 1024, GLOC_ERR_INVALID,
               "n_lists * k = %zu outside [1,1024]", n_lists * k);
  GLOC_REQUIRE(nq >= 1 && nq <= (1u << 20), GLOC_ERR_INVALID, "nq outside [1,2^20]");
  GLOC_TRY(select_device(device));
  hipLaunchKernelGGL(merge_kernel, dim3((unsigned)nq), dim3(64), 0, (hipStream_t)hip_stream, d_idx,
                     d_d2, (int)n_lists, (int)nq, (int)k, d_out_idx, d_out_d2);
  GLOC_HIP(hipGetLastError());
  return GLOC_OK;
}

int gloc_knn_get_stats(const gloc_knn* h, gloc_knn_stats* out) {
  GLOC_REQUIRE(h && out, GLOC_ERR_INVALID, "null argument");
  *out = h->stats;
  if (h->n_incomplete.p) {  // the fallback count lives on the device (no read-back on the search path)
    unsigned long long c = 0;
    GLOC_HIP(hipSetDevice(h->device));
    GLOC_HIP(hipStreamSynchronize(h->stream));
    GLOC_HIP(hipMemcpy(&c, h->n_incomplete.p, sizeof(c), hipMemcpyDeviceToHost));
    out->queries_fallback = c;
  }
  return GLOC_OK;
}

int gloc_knn_profile(gloc_knn* h, const char* kernel, double* total_ms, uint64_t* launches) {
  return handle_profile(h, kernel, total_ms, launches);
}

int gloc_knn_profile_reset(gloc_knn* h) { return handle_profile_reset(h); }

}  // extern "C"
