/*
 * gloc3d.h -- C ABI of the MI355X-native place-retrieval + global-registration hot path.
 *
 * This is the drop-in boundary: plain C, opaque handles, `int` status codes, no exceptions and no
 * torch/HIP types in any signature (streams travel as `void*`).  One handle = one device + one HIP
 * stream + one caller thread (thread-compatible, not thread-safe -- the same contract as the
 * reference's RpyPCLoopDetector, registration/loop_detector.h:41-119).  The caller owns every host
 * buffer; handles own their device memory.  There is NO CPU fallback: every entry point fails with
 * GLOC_ERR_NODEVICE / GLOC_ERR_HIP when no gfx950 device is usable.
 *
 * Each entry point cites the reference interface it replaces (paths relative to the reference
 * repository root).  INTEGRATION.md shows the reference-side bindings.
 */
#ifndef GLOC3D_H
#define GLOC3D_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GLOC3D_ABI_VERSION 6

enum {
  GLOC_OK = 0,
  GLOC_ERR_INVALID = 1,  /* bad argument (null pointer, k = 0, k too large, dim mismatch ...) */
  GLOC_ERR_HIP = 2,      /* a HIP runtime call failed; see gloc_last_error() */
  GLOC_ERR_NOMEM = 3,    /* device or host allocation failed */
  GLOC_ERR_NODEVICE = 4, /* no usable gfx950 device */
  GLOC_ERR_STATE = 5     /* call not valid in the handle's current state */
};

/* Thread-local description of the last failure on the calling thread ("" if none). */
const char* gloc_last_error(void);
int gloc_abi_version(void);
/* Number of visible HIP devices (0 if none; never fails). */
int gloc_device_count(void);

/* ============================ descriptor kNN ============================================= *
 * Replaces the KD-tree the reference builds over its descriptor database,
 *   InvKeyTree(k_dim_, db_features_, 10)            registration/loop_detector.cpp:36,70
 *   kdtree_->query(&feat[0], top_k_, idx, d2)        registration/loop_detector.cpp:45,79
 *   (KDTreeVectorOfVectorsAdaptor<KeyMat,float>::query,
 *    registration/KDTreeVectorOfVectorsAdaptor.h:95-102)
 * and its Python twin faiss.IndexFlatL2(pool).add / .search(qFeat, 20), main.py:317-324.
 * Results are the exact squared-L2 top-k, ascending, with the d2 bit patterns of
 * nanoflann's L2_Adaptor::evalMetric (registration/nanoflann.hpp:453-487); rows at exactly equal
 * distance come out in ascending row index.
 */
typedef struct gloc_knn gloc_knn;

/* Algorithm selection for gloc_knn_set_option(GLOC_KNN_OPT_ALGO, ...). */
enum {
  GLOC_KNN_ALGO_AUTO = 0,  /* exact streaming kernel for few queries, MFMA path otherwise */
  GLOC_KNN_ALGO_EXACT = 1, /* reference-order fp32 differences on the vector ALUs, one pass */
  GLOC_KNN_ALGO_MFMA = 2,  /* matrix-core coarse pass -2Q.D^T + norms (operands split in two bf16 values, three bf16
                              MFMAs per product -- a proven bound on what that drops; fp32 MFMA when dim % 8 != 0),
                              top-k' selection, exact re-rank in the reference's order, completeness proven per query
                              (an unproven query is redone on the exact path): the same bits as GLOC_KNN_ALGO_EXACT.  A handle
                              whose searches keep failing that proof (rows clustered tightly relative to their norms) runs
                              its next searches with the fp32 coarse pass, whose bound is eight times tighter */
  GLOC_KNN_ALGO_MFMA_FP32 = 3 /* the same with the coarse pass on the fp32 MFMA (the rounds 1 - 3 form) */
};
enum {
  GLOC_KNN_OPT_ALGO = 1,
  GLOC_KNN_OPT_CANDIDATES = 2, /* k' kept by the MFMA path before the exact re-rank (<= 64) */
  GLOC_KNN_OPT_PROFILE = 3     /* 1: bracket every kernel with HIP events (gloc_knn_profile) */
};

/* device: HIP ordinal.  dim: descriptor length (reference: k_dim_ = 512, loop_detector.h:97). */
int gloc_knn_create(int device, size_t dim, gloc_knn** out);
/* A second SEARCH handle over the same resident database (round 6): its own HIP stream and workspace, the parent's rows
 * (no copy; rows the parent has added -- and finished adding: synchronize it -- are seen by the view's next search).
 * Searches on the parent and on a view run side by side on the device: one's selection + re-rank (a work-group per query:
 * 64 of 256 CUs at 64 queries) under the other's distance kernel -- back-to-back searches of DIFFERENT query batches then
 * cost max(stage) instead of the sum (bench.py: knn_cfgB_pipelined_us).  nanoflann's query is const for the same reason
 * (KDTreeVectorOfVectorsAdaptor.h:95-102).  A view cannot add / reserve / clear / load (GLOC_ERR_STATE); the parent cannot be
 * destroyed while views live. */
int gloc_knn_create_view(gloc_knn* parent, gloc_knn** out);
int gloc_knn_destroy(gloc_knn* h);

/* Use `hip_stream` (a hipStream_t created by the caller on the same device) for all work of this
 * handle instead of the handle's own stream.  NULL restores the own stream. */
int gloc_knn_set_stream(gloc_knn* h, void* hip_stream);
int gloc_knn_synchronize(gloc_knn* h);
int gloc_knn_set_option(gloc_knn* h, int option, int64_t value);

/* Append n rows (row-major n x dim, host memory).  Replaces db_features_.push_back(feat)
 * (registration/loop_detector.cpp:14) and faiss_index.add(dbFeat) (main.py:320).  Unlike the
 * reference's tree, which silently goes stale after the first detect (loop_detector.cpp:34-37
 * builds once over a const-ref), rows are searchable immediately. */
int gloc_knn_add(gloc_knn* h, const float* rows, size_t n);
/* Same with rows already in device memory on the handle's device. */
int gloc_knn_add_device(gloc_knn* h, const float* d_rows, size_t n);
int gloc_knn_reserve(gloc_knn* h, size_t n_rows);
int gloc_knn_clear(gloc_knn* h);
int gloc_knn_size(const gloc_knn* h, size_t* n_rows);
int gloc_knn_dim(const gloc_knn* h, size_t* dim);
/* Device pointer of the resident row-major database (valid until the next add/reserve/clear). */
int gloc_knn_device_rows(const gloc_knn* h, const float** d_rows);

/* Persist / restore the database ("next" row N4; the reference keeps its descriptor database in
 * memory only and rebuilds it from the scans on every start, global_localization.cpp:419-449).
 * File: "GLOCDESC", u32 rows, u32 dim, then rows x dim little-endian fp32 -- the same format the
 * drop-in global_localization command line reads in place of the TorchScript model.
 * load APPENDS the file's rows (dim must match). */
int gloc_knn_save(gloc_knn* h, const char* path);
int gloc_knn_load(gloc_knn* h, const char* path);

/* Top-k over rows [first_row, last_row) for nq queries (host buffers).  last_row is clamped to the
 * database size; pass SIZE_MAX for "all".  The row window expresses the SLAM-mode exclusion of the
 * newest frames (db_features_.begin() .. end()-num_exclude_recent_, loop_detector.cpp:66-72).
 * out_idx: nq x k row indices, out_d2: nq x k squared distances, ascending.  If the window holds
 * fewer than k rows the tail is idx = UINT64_MAX, d2 = FLT_MAX. */
int gloc_knn_search(gloc_knn* h, const float* queries, size_t nq, size_t k, size_t first_row,
                    size_t last_row, uint64_t* out_idx, float* out_d2);

/* Same with device buffers, enqueued on the handle's stream; `index_offset` is added to every
 * returned index (a shard's first global row, for row-sharded databases).  Returns after the work
 * is enqueued: for windows of up to 16384 rows there is no host synchronisation at all (queries whose
 * candidate set the MFMA path cannot prove complete are redone on the exact path by kernels that are
 * always enqueued and leave at once otherwise); larger windows read the completeness flags back. */
int gloc_knn_search_device(gloc_knn* h, const float* d_queries, size_t nq, size_t k,
                           size_t first_row, size_t last_row, uint64_t index_offset,
                           uint64_t* d_out_idx, float* d_out_d2);

/* Merge `n_lists` sorted top-k lists per query (gathered from the shards of a row-sharded
 * database: layout [n_lists][nq][k]) into one top-k, ordered by (d2, idx).  Device buffers;
 * enqueued on `hip_stream` (may be NULL = default stream). */
int gloc_topk_merge_device(int device, void* hip_stream, const uint64_t* d_idx, const float* d_d2,
                           size_t n_lists, size_t nq, size_t k, uint64_t* d_out_idx,
                           float* d_out_d2);

/* ---- multi-GPU through the C ABI (one process per GPU, RCCL over xGMI) ------------ *
 * The descriptor database is row-sharded over the ranks of a communicator; queries are replicated.
 * librccl is bound at run time (the copy already in the process -- PyTorch's -- else GLOC3D_RCCL, else
 * /opt/rocm/lib).  Rank 0 makes the 128-byte id and hands it to the others by any channel (a file,
 * MPI, torch.distributed); every rank then calls gloc_comm_create (ncclCommInitRank: collective). */
typedef struct gloc_comm gloc_comm;
int gloc_comm_unique_id(uint8_t* id128);
int gloc_comm_create(int device, int rank, int world, const uint8_t* id128, gloc_comm** out);
int gloc_comm_destroy(gloc_comm* c);
int gloc_comm_rank(const gloc_comm* c, int* rank, int* world);
/* d_recv[r * bytes_per_rank ..] = rank r's d_send; enqueued on hip_stream (result tables of a step). */
int gloc_comm_all_gather_device(gloc_comm* c, const void* d_send, void* d_recv, size_t bytes_per_rank,
                                void* hip_stream);
/* Top-k over the WHOLE row-sharded database, replicated on every rank and bit-equal to the one-GPU
 * search: this rank's shard is searched (local row l is global row l * index_stride + index_offset:
 * stride = world, offset = rank for the interleaved layout; stride 1, offset = first row for contiguous
 * shards), the per-shard (d2, idx) lists are all-gathered in ONE fused RCCL launch on the handle's
 * stream, and merged by (d2, idx) on the device (K3).  No host hop, no host synchronisation beyond the
 * search's own.  Collective: every rank calls it with the same nq and k. */
int gloc_knn_search_sharded(gloc_knn* h, gloc_comm* comm, const float* d_queries, size_t nq, size_t k,
                            uint64_t index_stride, uint64_t index_offset, uint64_t* d_out_idx,
                            float* d_out_d2);

/* Host-buffer forms (the C++ command line's sharded mode): staged through the device, synchronous. */
int gloc_knn_search_sharded_host(gloc_knn* h, gloc_comm* comm, const float* queries, size_t nq, size_t k,
                                 uint64_t index_stride, uint64_t index_offset, uint64_t* out_idx,
                                 float* out_d2);
int gloc_comm_all_gather_host(gloc_comm* c, const void* send, void* recv, size_t bytes_per_rank);

/* Counters since creation: searches on each path, queries that needed the exact fallback. */
typedef struct gloc_knn_stats {
  uint64_t searches_exact, searches_mfma, queries_total, queries_fallback;
  uint32_t last_n_tile, last_k_split, last_candidates;
} gloc_knn_stats;
int gloc_knn_get_stats(const gloc_knn* h, gloc_knn_stats* out);

/* With GLOC_KNN_OPT_PROFILE = 1: accumulated HIP-event time of one kernel family since the last
 * gloc_knn_profile_reset.  Names: "dist_exact", "dist_mfma", "select", "rerank", "norms",
 * "finalize".  Synchronizes the stream. */
int gloc_knn_profile(gloc_knn* h, const char* kernel, double* total_ms, uint64_t* launches);
int gloc_knn_profile_reset(gloc_knn* h);

/* ============================ 3-D registration =========================================== *
 * Replaces the reference's per-candidate registration seam,
 *   icp_match_3d(src, tgt, guess, pose)   registration/global_registration.cpp:237-248
 *   (pcl::IterativeClosestPoint, 30 iterations), and the RANSAC transform estimate the reference
 *   runs per candidate (cv::estimateAffinePartial2D(..., RANSAC, 3*res, 3000),
 *   registration/loop_detector.cpp:256-257), as the batched loop over the top-20 candidates of
 *   GlocEvaluator::global_registraion (registration/global_localization.cpp:511-574).
 * Semantics: SURVEY.md Appendix B (S1 exact 1-NN, S2 RANSAC 3-point Kabsch/SVD + inlier count +
 * refit, S3 point-to-point ICP).
 */
typedef struct gloc_reg gloc_reg;

typedef struct gloc_reg_params {
  uint32_t ransac_iters;  /* 3000 (loop_detector.cpp:257); 0 disables RANSAC */
  float inlier_thresh;    /* 0.6 m = 3 x 0.2 m (loop_detector.cpp:257, loop_detector.h:116) */
  float min_inlier_ratio; /* ok iff best inliers >= ratio x n_src (and >= 3) */
  uint32_t icp_iters;     /* 30 (global_registration.cpp:242) */
  float max_corr_dist;    /* <= 0: no correspondence rejection (PCL default) */
  uint64_t seed;          /* RANSAC sampling seed */
  float ransac_confidence; /* 0.99: adaptive stop as in OpenCV's RANSAC, which the reference calls with
                             its default confidence (loop_detector.cpp:256-257): ransac_iters is the
                             cap, hypotheses beyond the iteration count that reaches this confidence
                             for the best inlier ratio so far are not considered.  <= 0 or >= 1: off */
  float max_rmse;          /* > 0: a candidate is ok only if, in addition, the RMS nearest-neighbour distance of
                             its final pose is <= this (metres).  Plausibility check on the estimated
                             transform, the analogue of the reference's |1 - scale| < 0.1
                             (loop_detector.cpp:268-272): the RANSAC inlier ratio at 0.6 m alone cannot
                             tell two scenes apart that share a ground plane.  <= 0: off (default) */
  float max_final_step;    /* > 0 (needs icp_iters > 0): a candidate is ok only if, in addition, the ICP has CONVERGED:
                             the RMS displacement its last update gives the matched points --
                             sqrt(|R c + t - c|^2 + |R - I|_F^2 / 2 * tr cov), c and cov the centroid and covariance
                             of those points -- is <= this; an ICP that stopped for want of correspondences
                             (max_corr_dist) counts as not converged.  A plausibility check of the 3-D stage in the
                             role the reference gives |1 - scale| < 0.1 on its 2-D fit (loop_detector.cpp:268-272);
                             pcl::IterativeClosestPoint::hasConverged() is the nearest thing upstream, and the
                             reference does not consult it.  <= 0: OFF -- THE DEFAULT (round 5; 0.03 in round 4): the
                             reference's 3-D stage accepts whatever its ICP returns, and so does this library unless
                             the caller asks (the loop_detector mirrors and the two command lines do not: their
                             plausibility check is the reference's, on the 2-D match).  bench.py passes
                             GLOC_REG_FINAL_STEP_SUGGESTED below and says so in its line. */
} gloc_reg_params;

/* A value for gloc_reg_params.max_final_step.  NOT reference-derived (the reference has no such quantity): it was
 * chosen by sweeping 0.025 / 0.03 / 0.04 / 0.05 m over bench.py's own synthetic legs (LAB_NOTES.md, round 4) and
 * checked in round 5 on worlds, views and poses that sweep never saw (bench.py legs.gate_holdout,
 * tests/test_gate_holdout_gpu.py; DESIGN.md section 4 has the numbers, including the right poses it rejects). */
#define GLOC_REG_FINAL_STEP_SUGGESTED 0.03f

/* Fills the defaults above: the reference's constants where it has them (3000 hypotheses, 0.6 m, 30 ICP passes,
 * confidence 0.99), this library's own otherwise (min_inlier_ratio 0.3, seed 1234); both plausibility checks off. */
void gloc_reg_default_params(gloc_reg_params* p);

int gloc_reg_create(int device, gloc_reg** out);
int gloc_reg_destroy(gloc_reg* h);
/* Use `hip_stream` for all work of this handle (NULL: back to its own).  Handles may SHARE a stream: a batch call
 * returns when its own results have arrived (an event behind its last copy), not when the stream is idle, so two
 * handles driven by two host threads queue their batches back to back on one stream -- the device never waits for the
 * host between batches (bench.py's registration pipeline). */
int gloc_reg_set_stream(gloc_reg* h, void* hip_stream);
int gloc_reg_synchronize(gloc_reg* h);
int gloc_reg_set_option(gloc_reg* h, int option, int64_t value);
enum {
  GLOC_REG_OPT_PROFILE = 1, /* 1: bracket every kernel with HIP events (gloc_reg_profile) */
  GLOC_REG_OPT_NN_MODE = 2, /* how S1 (exact 1-NN) is searched; the result is identical */
  GLOC_REG_OPT_NN_SRC_PER_LANE = 3, /* culled search tuning: source points per lane (1, 2 or 4) */
  GLOC_REG_OPT_NN_JOB_GROUP = 4,    /* culled search tuning: jobs whose work-groups are interleaved in the
                                       launch order (their scans share the caches); default 24 -- 8 in a batch under
                                       48 jobs, with 2 / 4 / 8 shares of a job per slot (NN_SUB_JOBS below), unless either
                                       option is set.  A multiple of 8 keeps each slot's work-groups on one XCD, i.e. its
                                       scans in one L2 */
  GLOC_REG_OPT_TEMP_TARGET_INDEX = 5, /* 1: the host-buffer calls (gloc_reg_batch, gloc_reg_nn) build the kd-ordered
                                       target index for their temporary candidate scans too (default 0: a
                                       millisecond per candidate is more than one registration saves) */
  GLOC_REG_OPT_NN_SPLIT_HELPERS = 6, /* culled search: wave slots per job at the head of the launch order for the
                                       heaviest source groups (a group whose work estimate of the previous pass
                                       exceeds the threshold is searched by 2, 4 or 8 waves that start first;
                                       identical results).  -1 (default): by batch size (256 up to
                                       64 jobs, 64 up to 256, else off); 0: off */
  GLOC_REG_OPT_NN_SPLIT_THRESH = 7,  /* the estimate (cycles of one wave) above which a group is split; default
                                       60000 (85000 for the batches whose passes are chained: GLOC_REG_OPT_NN_CHAIN); 0: off */
  GLOC_REG_OPT_NN_SUB_JOBS = 8,      /* culled search tuning: interleaved shares of a job's work-groups that take a
                                       slot of the launch order each (a slot stays on one XCD); 0 (default): in a
                                       batch under 48 jobs, which 8 XCDs cannot balance job by job, the fewest of 2 / 4 /
                                       8 that make the slots a multiple of 8 (20 jobs: 2), else 1 */
  GLOC_REG_OPT_NN_HEAVY_THRESH = 9,  /* culled search, first (cold) pass of a batch: a wave that has processed this many
                                       target chunks hands its source group to a second launch, which searches it with
                                       8 waves (identical results); default 32; 0: off */
  GLOC_REG_OPT_SUB_BATCHES = 10,     /* no effect: accepted in [-1, 8] for existing callers.  It cut a small batch into
                                       runs of jobs on internal streams of their own, which measured SLOWER for one query
                                       alone (20 jobs: 3.2 ms on one stream, 3.9 with 4); a batch is always enqueued on
                                       the handle's stream */
  GLOC_REG_OPT_NN_CHAIN = 11,        /* 1 (default): the warm ICP passes of a SMALL batch (fewer than 48 jobs: one query's
                                       20 candidates) run as ONE launch -- every pass's searches, reductions, solves and
                                       plans laid end to end, a wave of pass p + 1 waiting on the device for its own
                                       job's solve of pass p -- instead of 2 launches per pass with the chip draining
                                       in between; 0: launch by launch.  Identical results.  Every device-side wait is
                                       bounded (3 s): a batch whose chain runs out is run again launch by launch before
                                       the call returns (said once on stderr) and the handle stops chaining until this
                                       option is set again */
  GLOC_REG_OPT_PAIRGRAPH_BUDGET = 12 /* internal (tests): bytes of graph workspace in flight at a time in
                                       gloc_reg_fpfh_graph_batch_ids, which walks its batch in groups of jobs that fit;
                                       0 (default): 1 GiB.  Identical results */
};
enum {
  GLOC_REG_NN_CULLED = 0,    /* default: Hilbert-sorted scans, box hierarchy, skip what cannot win */
  GLOC_REG_NN_EXHAUSTIVE = 1 /* every (source, target) pair: the brute-force kernel */
};

/* ---- scan store ---------------------------------------------------------------------------- *
 * The database scans stay resident in HBM with their search index (38 B/point: all 4541 scans of
 * KITTI-00 = 20 GB of the 288 GB) -- the reference re-reads every candidate scan from disk for every
 * query (registration/global_localization.cpp:521-525).  A store is shared by any number of
 * registration handles (gloc_reg_attach_store); query scans are added, used and released.
 * add/release/count are thread-safe; a scan must not be released while a registration that uses it
 * is in flight.  Indexing (bounding box, Hilbert keys, radix sort, boxes) runs on the device; add
 * returns when the scan is ready.  `stride_floats` is 3 for packed xyz or 4 for KITTI x,y,z,i
 * (registration/global_localization.cpp:160-182). */
typedef struct gloc_scan_store gloc_scan_store;
int gloc_scan_store_create(int device, gloc_scan_store** out);
/* GLOC_ERR_STATE while registration handles are still attached. */
int gloc_scan_store_destroy(gloc_scan_store* st);
int gloc_scan_store_add(gloc_scan_store* st, const float* pts, size_t n, size_t stride_floats,
                        uint32_t* scan_id);
/* Same with the points already in device memory on the store's device. */
int gloc_scan_store_add_device(gloc_scan_store* st, const float* d_pts, size_t n,
                               size_t stride_floats, uint32_t* scan_id);
/* `count` scans (host buffers pts[i] of n[i] points) uploaded and indexed in ONE launch sequence: the launch count
 * does not depend on `count` (every indexing kernel covers all the scans, the sorts are segmented).  The query scans
 * of a batch of localizations in flight go in together.  Each scan ends up exactly as gloc_scan_store_add leaves it. */
int gloc_scan_store_add_batch(gloc_scan_store* st, const float* const* pts, const size_t* n, size_t count,
                              size_t stride_floats, uint32_t* scan_ids);
/* Re-sort a resident scan's search index into kd order (the TARGET index): chunks and sub-blocks become
 * disjoint kd cells fitted to the point density instead of runs of a space-filling curve, and the culled 1-NN
 * search of every registration AGAINST this scan tests ~35 % fewer boxes and evaluates ~30 % fewer pairs.
 * Costs about a millisecond of device time per 120k-point scan, once: meant for the database places
 * (db_files_ of the reference's GlocEvaluator, read at registration/global_localization.cpp:521-525), not for
 * query scans, which are added, used as the source once and released.  Results never depend on it (the search is
 * exact either way).  The scan must not be in use by a registration in flight. */
int gloc_scan_store_build_target_index(gloc_scan_store* st, uint32_t scan_id);
/* The same for many scans, in batches of up to 8 M points per launch sequence (a database build). */
int gloc_scan_store_build_target_index_batch(gloc_scan_store* st, const uint32_t* scan_ids, size_t count);
/* Frees the scan's id and memory for reuse by later adds (ids of other scans do not change). */
int gloc_scan_store_release(gloc_scan_store* st, uint32_t scan_id);
int gloc_scan_store_clear(gloc_scan_store* st);
int gloc_scan_store_count(gloc_scan_store* st, size_t* n_scans);
/* HBM held by live scans, and by released allocations kept for reuse (either may be NULL). */
int gloc_scan_store_bytes(gloc_scan_store* st, size_t* live_bytes, size_t* cached_bytes);
int gloc_scan_store_points(gloc_scan_store* st, uint32_t scan_id, size_t* n_points);
/* The scan's points, original order, packed xyz (tests). */
int gloc_scan_store_download(gloc_scan_store* st, uint32_t scan_id, float* out_xyz,
                             size_t capacity_points);
/* Per-point unit normals of a resident scan, for the point-to-plane refinement (gloc_reg_p2l_batch_ids).  Exactly
 * gloc_ground_normals applied to the whole scan, with no range filter: the k nearest neighbours within the scan, self
 * included, in ascending (d2, index) order; fp64 mean and covariance accumulated in that order; the eigenvector of the
 * smallest eigenvalue (cyclic Jacobi, ties keep the lower column); flipped towards the origin; stored as fp32.  A point
 * with fewer than 3 usable neighbours or non-finite coordinates gets the ZERO normal, which means "no normal".
 * k in [3, 16]; 10 is the reference's (registration/ground_estimator.cpp:79).  An optional second allocation of the
 * scan, 12 B per point, kept in the order the 1-NN search reports its matches in; built at most once per (scan, k)
 * (the same k again is a no-op), freed by release / clear, counted by gloc_scan_store_bytes, carried along by
 * gloc_scan_store_build_target_index.  Safe on a scan that batches in flight have pinned -- it adds data and moves
 * nothing -- except that EXISTING normals of a pinned scan are not rebuilt with another k (GLOC_ERR_STATE). */
int gloc_scan_store_build_normals(gloc_scan_store* st, uint32_t scan_id, uint32_t k /* 3..16 */);
/* The scan's normals, original order, packed xyz, as gloc_scan_store_download (GLOC_ERR_STATE: none built). */
int gloc_scan_store_normals(gloc_scan_store* st, uint32_t scan_id, float* out_nxyz, size_t capacity_points);

/* Use `store` for every scan id of this handle (NULL: back to the handle's private store, which
 * gloc_reg_scan_upload creates on first use). */
int gloc_reg_attach_store(gloc_reg* h, gloc_scan_store* store);

/* Shims over the handle's current store (private unless one is attached). */
int gloc_reg_scan_upload(gloc_reg* h, const float* pts, size_t n, size_t stride_floats,
                         uint32_t* scan_id);
int gloc_reg_scan_build_target_index(gloc_reg* h, uint32_t scan_id); /* gloc_scan_store_build_target_index */
int gloc_reg_scan_release(gloc_reg* h, uint32_t scan_id);
int gloc_reg_scan_count(const gloc_reg* h, size_t* n_scans);
int gloc_reg_scan_clear(gloc_reg* h);

/* Register one query scan against n_cand candidate scans (host buffers, packed xyz).
 * init_T: n_cand x 16 row-major 4x4 (query -> candidate frame) or NULL for identity.
 * cand_stream_ids: RANSAC sampling stream of each candidate, or NULL for 0..n_cand-1 (its rank in
 * the retrieval list).  A rank that registers only a subset of a query's candidates passes their
 * ranks here so that the result is independent of how candidates are sharded over GPUs.
 * Outputs per candidate: out_T (n_cand x 16, query -> db), out_rmse, out_inliers, out_ok
 * (any may be NULL except out_T). */
int gloc_reg_batch(gloc_reg* h, const float* q_xyz, size_t nq_pts, const float* const* cand_xyz,
                   const size_t* cand_npts, size_t n_cand, const uint32_t* cand_stream_ids,
                   const float* init_T, const gloc_reg_params* params, float* out_T,
                   float* out_rmse, uint32_t* out_inliers, int* out_ok);

/* Same with the query scan and the candidates taken from the scan store. */
int gloc_reg_batch_ids(gloc_reg* h, uint32_t q_scan_id, const uint32_t* cand_scan_ids,
                       size_t n_cand, const uint32_t* cand_stream_ids, const float* init_T,
                       const gloc_reg_params* params, float* out_T, float* out_rmse,
                       uint32_t* out_inliers, int* out_ok);

/* Several queries in flight: query q is registered against candidates cand_scan_ids[q*n_cand ..]
 * (UINT32_MAX = no candidate: that row keeps its initial guess, ok = 0).  Every kernel launch covers
 * the candidates of ALL the queries, on the handle's one stream.  cand_stream_ids: n_queries x n_cand,
 * or NULL for 0..n_cand-1 per query.  init_T and the outputs are n_queries x n_cand rows.  Each row
 * equals what gloc_reg_batch_ids returns for that query alone, bit for bit. */
int gloc_reg_batch_multi(gloc_reg* h, size_t n_queries, const uint32_t* q_scan_ids,
                         const uint32_t* cand_scan_ids, size_t n_cand,
                         const uint32_t* cand_stream_ids, const float* init_T,
                         const gloc_reg_params* params, float* out_T, float* out_rmse,
                         uint32_t* out_inliers, int* out_ok);

/* The same in two halves.  begin: looks the scans up and ENQUEUES the whole launch sequence of the batch plus the copy of
 * its results on the handle's stream, then returns without waiting (nothing it needs from the caller is read later).
 * end: waits for THAT batch's results (its own event, not the stream) and writes the outputs, rows as in
 * gloc_reg_batch_multi.  One batch per handle may be in flight.  Two handles that share a stream (gloc_reg_set_stream)
 * pipeline a stream of batches from one host thread: begin(A, batch i + 1) goes in before end(B, batch i), so the
 * device runs batch after batch while the host post-processes -- bench.py's registration pipeline.  The scans of a batch
 * must stay in the store until its end. */
int gloc_reg_batch_multi_begin(gloc_reg* h, size_t n_queries, const uint32_t* q_scan_ids,
                               const uint32_t* cand_scan_ids, size_t n_cand, const uint32_t* cand_stream_ids,
                               const float* init_T, const gloc_reg_params* params);
int gloc_reg_batch_multi_end(gloc_reg* h, float* out_T, float* out_rmse, uint32_t* out_inliers, int* out_ok);

/* The reference's candidate loop as it is written -- stop at the first match()==true
 * (registration/global_localization.cpp:519-572) -- for several queries at once: rank by rank, the
 * rank-r candidates of all queries still without a success are registered in one batch.  Every job is the
 * one gloc_reg_batch_multi runs for that (query, rank), so out_rank / out_T equal
 * gloc_reg_select_first_ok over its result, bit for bit; only the candidates behind a success are never
 * touched.  out_rank: -1 where no candidate succeeded (out_T = identity); out_jobs_run (may be NULL):
 * registrations actually run. */
int gloc_reg_first_success_multi(gloc_reg* h, size_t n_queries, const uint32_t* q_scan_ids,
                                 const uint32_t* cand_scan_ids, size_t n_cand, const float* init_T,
                                 const gloc_reg_params* params, int* out_rank, float* out_T,
                                 float* out_rmse, uint32_t* out_inliers, uint64_t* out_jobs_run);

/* The reference's selection rule: lowest-rank candidate whose registration succeeded
 * (registration/global_localization.cpp:519-572 stops at the first match()==true).
 * Returns the rank or -1. */
int gloc_reg_select_first_ok(const int* ok, size_t n_cand);
/* The convergence measure of the last batch the handle returned: per job, in job order, the RMS displacement of the
 * last ICP update (what gloc_reg_params.max_final_step is compared with; 0 for a job without an ICP pass). */
int gloc_reg_final_steps(gloc_reg* h, float* out, size_t n_jobs);

/* Building blocks, exposed for tests and for callers that drive ICP themselves (host buffers). */
int gloc_reg_nn(gloc_reg* h, const float* src_xyz, size_t n_src, const float* tgt_xyz,
                size_t n_tgt, const float* T16 /* may be NULL */, uint32_t* out_idx, float* out_d2);
int gloc_reg_ransac_hypotheses(gloc_reg* h, const float* src_xyz, const float* tgt_xyz,
                               const uint32_t* corr, size_t n, uint64_t seed, uint32_t cand,
                               uint32_t n_hyp, float* out_Rt /* n_hyp x 12 */,
                               uint32_t* out_valid, uint32_t* out_inliers, float inlier_thresh);

/* HIP-event time per kernel family ("nn", "ransac_hyp", "ransac_score", "accum", "solve",
 * "transform"), as gloc_knn_profile.  "nn_cold" is the part of "nn" that a batch's first, cold, pass took: the same
 * span counted a second time, so "nn" - "nn_cold" is the warm passes alone.  Where one family's launches follow
 * another's with nothing enqueued in between (a pass and its solve, the RANSAC phases, the refit), the two spans
 * share ONE event: the idle gap between the two kernels belongs to the later family, launch counts are unaffected. */
int gloc_reg_profile(gloc_reg* h, const char* kernel, double* total_ms, uint64_t* launches);
int gloc_reg_profile_reset(gloc_reg* h);
/* With profiling on: (source, target) pairs evaluated by the culled 1-NN kernel and the number of
 * 1-NN launches since the last gloc_reg_profile_reset. */
int gloc_reg_nn_stats(gloc_reg* h, uint64_t* pairs_evaluated, uint64_t* launches);

/* ---- NDT scan registration ---------------------------------------------------------------------------- *
 * Replaces ndt_match_3d (registration/global_registration.cpp:250-330): the source thinned by an approximate voxel grid
 * (pcl::ApproximateVoxelGrid, 0.2 m), the unfiltered target modelled by normal distributions in 0.5 m cells
 * (pcl::VoxelGridCovariance), Newton iterations with a More-Thuente line search from the caller's guess
 * (pcl::NormalDistributionsTransform: step 0.1, epsilon 0.01, 35 iterations).  The executable contract is the float64
 * restatement tests/ndt_ref.py; parity with PCL itself is unpinned.  A refinement behind a 3-D
 * RANSAC guess, in the slot the reference's use_icp branch gives ICP or NDT (:1388-1398). */
typedef struct gloc_ndt_params {
  float source_leaf;             /* 0.2 m (:256); <= 0: no filter (the finite points of the source) */
  float resolution;              /* 0.5 m cells (:271) */
  float step_size;               /* 0.1: the line search's largest step (:268) */
  float trans_eps;               /* 0.01: stop once a step is shorter (:266); the line search's shortest step is half of it */
  uint32_t max_iters;            /* 35 (:274) */
  float outlier_ratio;           /* 0.55 [upstream default] */
  uint32_t min_points_per_cell;  /* 6 [upstream default] */
  float min_covar_eigvalue_mult; /* 0.01 [upstream default]: eigenvalues below this x the largest are raised to it */
} gloc_ndt_params;

void gloc_ndt_default_params(gloc_ndt_params* p);

/* Refine n candidates: the source scan against each target scan (ids of the handle's store), from init_T (n x 16
 * row-major floats, source -> target, NULL = identity).  The source is filtered once per call.  Outputs per candidate
 * (any may be NULL except out_T): the pose (n x 16), trans_probability = score / filtered source size, the iteration
 * count, and converged = the loop stopped because a step was shorter than trans_eps (or was zero) -- stricter than
 * PCL's hasConverged(), which is also true when the iteration cap stops it.  A target with no cell in reach of the
 * source returns its guess after 0 iterations with probability 0.  Every candidate's result is independent of the
 * batch it is in, bit for bit.  GLOC_ERR_INVALID: null arguments, an unknown id, resolution <= 0, max_iters = 0, an empty
 * filtered source; GLOC_ERR_STATE: a batch in flight on the handle. */
int gloc_reg_ndt_batch_ids(gloc_reg* h, uint32_t src_scan_id, const uint32_t* tgt_scan_ids, size_t n, const float* init_T,
                           const gloc_ndt_params* prm, float* out_T, double* out_prob, uint32_t* out_iters,
                           int* out_converged);
/* One evaluation at p6 = [tx, ty, tz, rx, ry, rz] (T = Trans Rx Ry Rz) of the score, gradient and Hessian (6 x 6 row-major)
 * of the filtered source against the target's cells (tests and callers that drive the optimiser themselves). */
int gloc_reg_ndt_derivatives(gloc_reg* h, uint32_t src_scan_id, uint32_t tgt_scan_id, const double p6[6],
                             const gloc_ndt_params* prm, double* out_score, double* out_grad6, double* out_hess36);
/* The valid cells of a scan at prm->resolution, sorted by (kx, ky, kz): integer cell index, point count, mean, inverse
 * covariance (3 x 3 row-major).  n_cells: how many there are (the arrays may be NULL to ask). */
int gloc_reg_ndt_cells(gloc_reg* h, uint32_t scan_id, const gloc_ndt_params* prm, size_t capacity, int32_t* out_key3,
                       uint32_t* out_count, double* out_mean3, double* out_icov9, size_t* n_cells);
/* A new resident scan: the approximate voxel filter (pcl::ApproximateVoxelGrid: 512 hash slots, a slot taken by another
 * cell is flushed first) of scan base_id at `leaf` -- the NDT source filter on its own, e.g. to thin a source before ICP.
 * Rows come out in (slot, first point) order. */
int gloc_scan_store_add_approx_voxel(gloc_scan_store* st, uint32_t base_id, float leaf, uint32_t* new_id);

/* ---- local submaps --------------------------------------------------------------------------------------- *
 * A registration target made of several resident scans: the members brought into one frame by their poses and thinned by
 * an EXACT voxel grid (one centroid per occupied cell).  Such a target has no ring pattern of its own, covers what one
 * view occludes and overlaps a query that stands between two places.  The reference has no counterpart; the executable
 * contract is the numpy restatement tests/submap_ref.py, bit for bit:
 *   - member m = a resident scan id and a 4x4 row-major fp32 pose T_m, member frame -> submap frame (rows 0..2 are used);
 *   - point p = (x, y, z) of the member's original-order xyz (the result never depends on a member's target index) is
 *     left out if a coordinate is not finite, or if max_range > 0 and (x x + y y) + z z > max_range^2;
 *   - q_a = ((T[a][0] x + T[a][1] y) + T[a][2] z) + T[a][3], every product and sum rounded to fp32 on its own;
 *   - k_a = floorf(q_a * (1.0f / leaf)); the point is left out if q is not finite or |k_a| >= 2^20 on an axis;
 *   - cells ascend in (kx, ky, kz); inside a cell the points are in (position in the member list, point index) order;
 *   - centroid = fp32(sum / count), the sum accumulated in fp64 in that order, the division in fp64;
 *   - a cell stays iff count >= max(min_points, 1) and the number of distinct member positions in it >= max(min_scans, 1)
 *     (an id listed twice counts twice);
 *   - the centroids that stay, in cell order, become a new resident scan, exactly the scan gloc_scan_store_add_device
 *     makes of those points.
 * One member with the identity pose is the exact voxel-grid filter of one scan (its rows in cell order, independent of
 * the point order -- unlike gloc_scan_store_add_approx_voxel). */
typedef struct gloc_submap_params {
  float leaf;            /* 0.2 m */
  uint32_t min_points;   /* 1 */
  uint32_t min_scans;    /* 1; 2 drops what only one member saw (moving objects) -- at the price of most cells of a sparse map */
  float max_range;       /* <= 0: off; else member points farther than this from their own sensor are left out */
  uint32_t group_points; /* 0: 8 M.  Input points per launch sequence of the batch call; results never depend on it */
} gloc_submap_params;

typedef struct gloc_submap_info {
  uint64_t points_in;   /* points of the members */
  uint64_t points_used; /* ... that fell into a cell */
  uint32_t cells;       /* occupied cells */
  uint32_t kept;        /* cells that stayed = points of the new scan */
} gloc_submap_info;

void gloc_submap_default_params(gloc_submap_params* p);

/* One submap of n members (member_T: n x 16); *new_id: the new scan.  info may be NULL.  The members are only read
 * (scans pinned by batches in flight are fine); the call holds the store's mutex and returns when the scan is complete.
 * GLOC_ERR_INVALID, before any device work: a null argument, n = 0, an unknown or released id, leaf not positive and
 * finite, a non-finite pose entry, members that hold 2^31 points or more (or none), more than 65535 members; and, after
 * the device work, a submap in which no cell stays.  A call that fails adds nothing. */
int gloc_scan_store_add_submap(gloc_scan_store* st, const uint32_t* member_ids, const float* member_T, size_t n,
                               const gloc_submap_params* prm, uint32_t* new_id, gloc_submap_info* info);
/* `count` submaps at once: submap s has members first[s] .. first[s + 1] - 1 of the two arrays (first: count + 1 entries,
 * strictly ascending).  One launch sequence per group of submaps of at most prm->group_points input points, however many
 * submaps the group holds; every submap equals the single call, bit for bit.  new_ids: count; info: count, or NULL.  A
 * batch that fails for any reason -- one empty submap included -- leaves the store as it found it. */
int gloc_scan_store_add_submaps(gloc_scan_store* st, const uint32_t* member_ids, const float* member_T, const uint32_t* first,
                                size_t count, const gloc_submap_params* prm, uint32_t* new_ids, gloc_submap_info* info);
/* The same over the handle's current store, as gloc_reg_scan_upload is. */
int gloc_reg_scan_add_submaps(gloc_reg* h, const uint32_t* member_ids, const float* member_T, const uint32_t* first,
                              size_t count, const gloc_submap_params* prm, uint32_t* new_ids, gloc_submap_info* info);

/* ---- point-to-plane ICP refinement -------------------------------------------------------------------- *
 * The linearised point-to-plane step (Chen & Medioni; pcl::IterativeClosestPointWithNormals, Open3D's
 * TransformationEstimationPointToPlane) behind the exact 1-NN search of the ICP above, on the TARGET's normals
 * (gloc_scan_store_build_normals).  Lidar scans are mostly ground and walls: point-to-point pairs resist sliding along
 * those surfaces, point-to-plane pairs do not, so it needs fewer passes.  An alternative a caller chooses; the default
 * pipeline is unchanged.  The executable contract is the float64 restatement tests/p2l_ref.py.
 *
 * One pass at pose T = (R, t), source -> target:
 *   1. every source point s: p = R s + t in fp32 (the pose rounded to fp32, the ICP's operation order);
 *   2. j = the exact 1-NN of p in the target (the ICP's search: same bits, same tie rule);
 *   3. the pair is used iff d2 is finite, max_corr_dist <= 0 or d2 <= max_corr_dist^2, and the normal n_j is not zero;
 *   4. in fp64, r = n_j . (p - q_j), J = [p x n_j ; n_j]:  H += J J^T, g += J r, sum r^2, the count;
 *   5. fewer than 6 pairs, or a pivot of the fp64 Cholesky factorisation of H <= 1e-12 x the largest diagonal entry of H:
 *      status 2, the pose stays, the job stops;
 *   6. H xi = -g, xi = (w, v);  7. T <- (Rodrigues(w), v) . T, held in fp64;
 *   8. both eps > 0 and |v| < trans_eps and |w| < rot_eps: status 1, the job stops (the updating pass is counted);
 *   9. a job that has stopped is frozen: later passes of the batch leave its pose alone. */
typedef struct gloc_p2l_params {
  uint32_t max_iters;  /* 30, as the reference's ICP (registration/global_registration.cpp:242) */
  float max_corr_dist; /* <= 0: no rejection, as gloc_reg_params */
  float trans_eps;     /* stop when |v| < trans_eps AND |w| < rot_eps; both <= 0 (default): run max_iters passes */
  float rot_eps;
  uint32_t normal_k;   /* 10: targets without normals get them built with this k (existing normals are used as they are) */
  uint32_t reserved_;
} gloc_p2l_params;

void gloc_p2l_default_params(gloc_p2l_params* p);

/* Refine n candidates: the source scan against each target scan (ids of the handle's store) from init_T (n x 16
 * row-major floats, source -> target; NULL = identity).  Outputs per candidate (any may be NULL except out_T): the pose,
 * the RMS point-to-plane residual of ONE more evaluation at the final pose, the number of updates applied, and the
 * status: 0 the iteration cap stopped it, 1 converged, 2 degenerate (the pose is the last one before the degenerate
 * pass: the guess, if it was the first).  Every candidate's result is independent of the batch it is in, bit for bit.
 * GLOC_ERR_INVALID: null arguments, an unknown id, an empty source, max_iters = 0, normal_k outside [3, 16];
 * GLOC_ERR_STATE: a batch in flight on the handle. */
int gloc_reg_p2l_batch_ids(gloc_reg* h, uint32_t src_scan_id, const uint32_t* tgt_scan_ids, size_t n, const float* init_T,
                           const gloc_p2l_params* prm, float* out_T, float* out_rmse, uint32_t* out_iters, int* out_status);
/* Steps 1 - 4 once at T16 (NULL = identity): H (6 x 6 row-major), g, sum r^2 and the number of pairs used (tests, and
 * callers that drive the loop themselves). */
int gloc_reg_p2l_system(gloc_reg* h, uint32_t src_scan_id, uint32_t tgt_scan_id, const float* T16, const gloc_p2l_params* prm,
                        double* out_H36, double* out_g6, double* out_sum_r2, uint64_t* out_count);

/* ---- generalized (plane-to-plane) ICP refinement ------------------------------------------------------ *
 * Generalized ICP (Segal, Haehnel & Thrun; pcl::GeneralizedIterativeClosestPoint, fast_gicp) behind the same exact 1-NN
 * search, on BOTH scans' normals.  Every pair is weighted by a full 3 x 3 information matrix built from the two local
 * surface models: it slides along ground and walls as point-to-plane does, down-weights pairs whose two surfaces
 * disagree, and is point-to-point where a side has no normal.  The covariances are PCL's plane-to-plane regularisation --
 * the eigenvalues of a neighbourhood's covariance replaced by (1, 1, plane_eps) -- which makes a point's covariance a
 * function of its normal alone, C = I - (1 - plane_eps) n n^T, so the scans' normals (gloc_scan_store_build_normals) are
 * all it stores.  An alternative a caller chooses; the default pipeline is unchanged.  The executable contract is the
 * float64 restatement tests/gicp_ref.py.
 *
 * M is frozen at each pass's linearisation point: this is the Gauss-Newton step as fast_gicp takes it, NOT PCL's BFGS
 * inner loop, and parity with PCL is unpinned.  PCL's neighbourhood size is 20; the store's k-NN stops at 16.
 *
 * One pass at pose T = (R, t), source -> target, with a = 1 - plane_eps:
 *   1. every source point s: p = R s + t in fp32 (the pose rounded to fp32, the ICP's operation order);
 *   2. j = the exact 1-NN of p in the target (the ICP's search: same bits, same tie rule);
 *   3. the pair is used iff d2 is finite, p is finite, and max_corr_dist <= 0 or d2 <= max_corr_dist^2;
 *   4. C_A = I - a n_s n_s^T from the source point's normal, C_B = I - a n_j n_j^T from the match's; a zero normal means
 *      "no normal" and gives C = I: the pair stays and is isotropic on that side.  From here on in fp64;
 *   5. m = R n_s (R the fp32 pose widened), S = C_B + R C_A R^T = 2I - a (n_j n_j^T + m m^T), M = S^-1 (S is symmetric
 *      with eigenvalues >= 2 plane_eps);
 *   6. e = p - q_j, and for T <- exp(xi) T, xi = (w, v), J = [-[p]x , I]:  H += J^T M J, g += J^T M e, sum e^T M e, the
 *      count;
 *   7. fewer than 6 pairs, or a pivot of the fp64 Cholesky factorisation of H <= 1e-12 x the largest diagonal entry of H:
 *      status 2, the pose stays, the job stops;
 *   8. H xi = -g;  T <- (Rodrigues(w), v) . T, held in fp64;
 *   9. both eps > 0 and |v| < trans_eps and |w| < rot_eps: status 1, the job stops (the updating pass is counted);
 *  10. a job that has stopped is frozen: later passes of the batch leave its pose alone. */
typedef struct gloc_gicp_params {
  uint32_t max_iters;  /* 30, as the reference's ICP (registration/global_registration.cpp:242) */
  float max_corr_dist; /* <= 0: no rejection, as gloc_reg_params */
  float trans_eps;     /* stop when |v| < trans_eps AND |w| < rot_eps; both <= 0 (default): run max_iters passes */
  float rot_eps;
  uint32_t normal_k;   /* 10: scans without normals, the source included, get them built with this k (existing normals
                          are used as they are) */
  float plane_eps;     /* 1e-3: pcl::GeneralizedIterativeClosestPoint's gicp_epsilon_ [upstream default]; must be in
                          (0, 1]; 1 makes every pair point-to-point.  The normals are unit to fp32 rounding only: below
                          about 1e-6 S is no longer safely positive definite */
} gloc_gicp_params;    /* 24 bytes */

void gloc_gicp_default_params(gloc_gicp_params* p);

/* Refine n candidates as gloc_reg_p2l_batch_ids does: the same arguments and outputs, the rmse being
 * sqrt(sum e^T M e / count) of ONE more evaluation at the final pose.  Every candidate's result is independent of the
 * batch it is in, bit for bit.  Normals missing on the source or on a target are built first, under the rule of
 * gloc_scan_store_build_normals.  GLOC_ERR_INVALID: null arguments, an unknown id, an empty source, max_iters = 0,
 * normal_k outside [3, 16], plane_eps outside (0, 1]; GLOC_ERR_STATE: a batch in flight on the handle. */
int gloc_reg_gicp_batch_ids(gloc_reg* h, uint32_t src_scan_id, const uint32_t* tgt_scan_ids, size_t n, const float* init_T,
                            const gloc_gicp_params* prm, float* out_T, float* out_rmse, uint32_t* out_iters, int* out_status);
/* Steps 1 - 6 once at T16 (NULL = identity): H (6 x 6 row-major), g, sum e^T M e and the number of pairs used. */
int gloc_reg_gicp_system(gloc_reg* h, uint32_t src_scan_id, uint32_t tgt_scan_id, const float* T16, const gloc_gicp_params* prm,
                         double* out_H36, double* out_g6, double* out_sum, uint64_t* out_count);

/* ---- voxelized generalized ICP refinement -------------------------------------------------------------- *
 * Voxelized GICP (Koide, Yokozuka, Oishi & Banno; fast_gicp's FastVGICP): generalized ICP's distribution-to-distribution
 * cost without its nearest-neighbour search.  The target is cut into voxels of `resolution`, each with the mean of its
 * points and the mean of their plane-to-plane covariances; a moved source point is paired with the voxel it falls into
 * (and, by `neighbors`, the voxels around it) by one hash-table lookup each.  No 1-NN search runs, so a target needs no
 * target index: this is the one refinement usable on a scan that was only uploaded.  The voxel maps are built per call
 * on the device, as NDT's cells are.  With a = 1 - plane_eps and a zero normal meaning "no normal":
 *   1. normals: the source's and every target's, as generalized ICP takes them;
 *   2. voxels of a target: per point, in the order the scan was uploaded, k = floor(x * inv) per axis in fp32 with
 *      inv = 1.0f / resolution (a non-finite point, or one with |k| >= 2^20 on an axis, is in no voxel); per voxel with
 *      N >= min_points members: N, the mean mu (fp64 sums relative to the voxel's corner k * resolution, in upload order)
 *      and Nbar = (1 / N) sum n n^T over its members (fp64; a member without a normal adds zero).  The voxel's covariance is
 *      C_B = I - a Nbar, the mean of its members' generalized-ICP covariances (fast_gicp's rule); nothing is inverted here;
 *   3. each pass moves every source point by the pose rounded to fp32, p = R s + t in fp32, and finds its voxel by the
 *      rule of step 2;
 *   4. for each offset of the neighbourhood the voxel at (voxel of p) + offset, if the target has one, makes a pair.
 *      neighbors = 1: (0,0,0); 7: (0,0,0) (-1,0,0) (1,0,0) (0,-1,0) (0,1,0) (0,0,-1) (0,0,1); 27: the 3 x 3 x 3 block,
 *      dz, dy, dx from -1 to 1 with dx fastest -- the order the pairs of a point are summed in;
 *   5. a pair is used iff p is finite and max_corr_dist <= 0 or |p - mu|^2 <= max_corr_dist^2 (fp64);
 *   6. in fp64: m = R n_s, S = 2I - a (Nbar + m m^T), M = S^-1 (the symmetric adjugate; S has eigenvalues >= 2 plane_eps),
 *      e = p - mu, J = [-[p]x , I], and the pair's weight is w = N:  H += w J^T M J, g += w J^T M e, sum w e^T M e, the
 *      count of pairs (unweighted);
 *   7. - 10. steps 7 - 10 of generalized ICP: status 2 below 6 pairs or at a bad pivot, H xi = -g, T <- exp(xi) T in fp64,
 *      the stop test with both eps, stopped jobs frozen. */
typedef struct gloc_vgicp_params {
  uint32_t max_iters;  /* 30 */
  float max_corr_dist; /* <= 0: no rejection; else a pair's |p - mu| may not exceed it */
  float trans_eps;     /* stop when |v| < trans_eps AND |w| < rot_eps; both <= 0 (default): run max_iters passes */
  float rot_eps;
  uint32_t normal_k;   /* 10: scans without normals, the source included, get them built with this k */
  float plane_eps;     /* 1e-3, in (0, 1], as gloc_gicp_params */
  float resolution;    /* 1.0 m: the voxels' edge (fast_gicp's default); must be > 0 */
  uint32_t neighbors;  /* 7: voxels probed per source point; one of 1, 7, 27 */
  uint32_t min_points; /* 1: voxels with fewer points are left out; must be >= 1 */
  uint32_t reserved_;
} gloc_vgicp_params;   /* 40 bytes */

void gloc_vgicp_default_params(gloc_vgicp_params* p);

/* Refine n candidates as gloc_reg_gicp_batch_ids does: the same arguments and outputs.  The rmse is
 * sqrt(sum w e^T M e / count) of ONE more evaluation at the final pose: the residuals are weighted by the voxels' point
 * counts, the count is of pairs, so it is the WEIGHTED residual per pair, not a distance.  Every candidate's result is
 * independent of the batch it is in, bit for bit, and of whether a target carries a target index.  Normals missing on
 * the source or on a target are built first, under the rule of gloc_scan_store_build_normals.  GLOC_ERR_INVALID: null
 * arguments, an unknown id, an empty source, max_iters = 0, normal_k outside [3, 16], plane_eps outside (0, 1],
 * resolution <= 0, neighbors not 1, 7 or 27, min_points = 0; GLOC_ERR_STATE: a batch in flight on the handle. */
int gloc_reg_vgicp_batch_ids(gloc_reg* h, uint32_t src_scan_id, const uint32_t* tgt_scan_ids, size_t n, const float* init_T,
                             const gloc_vgicp_params* prm, float* out_T, float* out_rmse, uint32_t* out_iters, int* out_status);
/* Steps 1 - 6 once at T16 (NULL = identity): H (6 x 6 row-major), g, sum w e^T M e and the number of pairs used. */
int gloc_reg_vgicp_system(gloc_reg* h, uint32_t src_scan_id, uint32_t tgt_scan_id, const float* T16, const gloc_vgicp_params* prm,
                          double* out_H36, double* out_g6, double* out_sum, uint64_t* out_count);
/* The voxels of a scan (step 2), sorted by (kx, ky, kz): integer voxel index, point count, mean, Nbar as xx xy xz yy yz zz.
 * n_voxels: how many there are (the arrays may be NULL to ask). */
int gloc_reg_vgicp_voxels(gloc_reg* h, uint32_t scan_id, const gloc_vgicp_params* prm, size_t capacity, int32_t* out_key3,
                          uint32_t* out_count, double* out_mean3, double* out_nn6, size_t* n_voxels);

/* ---- robust weighting of the three Gauss-Newton refinements ---------------------------------------------- *
 * Iteratively re-weighted least squares (an M-estimator per pair, as Open3D's RobustKernel and small_gicp's Huber and
 * Cauchy factors) on point-to-plane, generalized and voxelized generalized ICP.  The gate max_corr_dist takes a pair
 * in with full weight or leaves it out; a moved object, other traffic and the half of a scan that does not overlap the
 * stored one all find a partner inside any gate wide enough to converge from a retrieval-grade guess.  Here every pair
 * is weighted by its own residual, on a scale that may be annealed from a wide start (graduated non-convexity).
 * Opt-in, through the _robust entries only: the plain entries do not change.  The executable contract is the float64
 * restatement tests/robust_ref.py.
 *
 * The residual of a pair, squared, in fp64:
 *   point-to-plane     s2 = r^2, r = n_j . (p - q_j): metres^2, so `scale` is in metres;
 *   generalized ICP    s2 = e^T M e: dimensionless.  For two coplanar surfaces M is 1 / (2 plane_eps) along their normal,
 *                      so s2 = e_n^2 / (2 plane_eps): a normal distance of d metres counts sqrt(s2) = 22.4 d at the default
 *                      plane_eps = 1e-3, and `scale` is in those units;
 *   voxelized          s2 = e^T M e of the (point, voxel) term, M = S^-1 BEFORE the voxel's point count N multiplies it.
 * The weight, with c the scale of the pass and t = s2 / (c c):
 *   HUBER          t <= 1 ? 1 : 1 / sqrt(t)          CAUCHY         1 / (1 + t)
 *   TUKEY          t <= 1 ? (1 - t)^2 : 0            GEMAN_MCCLURE  1 / ((1 + t) (1 + t))
 * What it multiplies: the pair's 27 contributions to H and g.  The squared-residual sum and the pair count stay what the
 * plain entries make them -- rmse, the "fewer than 6 pairs" rule and the count keep their meaning -- and the sum of the
 * weights is one more output.  A pair of weight 0 is still a pair: if every weight is 0, H is 0, the pivot rule makes
 * the job degenerate (status 2) and the pose stays.  max_corr_dist is applied first and unchanged.
 * The schedule:  c(0) = scale_start if one is set, else scale;  c(k + 1) = max(scale, c(k) anneal), in fp64 with the
 * floats widened.  The update a job applies as its k-th (k = its `iters` before it) uses c(k).  The stop test (status 1)
 * is honoured only on an update whose c(k) == scale: before that a small step means "this scale is exhausted", not
 * "done".  The evaluation after the loop (rmse, the weights' sum) uses `scale`. */
enum { GLOC_ROBUST_NONE = 0, GLOC_ROBUST_HUBER = 1, GLOC_ROBUST_CAUCHY = 2, GLOC_ROBUST_TUKEY = 3, GLOC_ROBUST_GEMAN_MCCLURE = 4 };
typedef struct gloc_robust_params {
  uint32_t kind;       /* NONE: the other three fields are ignored */
  float scale;         /* c > 0, finite: where a residual stops counting fully (units above) */
  float scale_start;   /* 0: no schedule; otherwise finite and >= scale */
  float anneal;        /* with a schedule: in (0, 1), the factor per applied update */
} gloc_robust_params;  /* 16 bytes */

/* kind NONE and zeros. */
void gloc_robust_default_params(gloc_robust_params* p);
/* What the device uses, on the host: c(pass) (0 for kind NONE, which has no scale), and the weight of a squared residual
 * s2 at c(pass) (1 for kind NONE).
 * GLOC_ERR_INVALID: a null argument or a block the entries below refuse. */
int gloc_robust_scale(const gloc_robust_params* prm, uint32_t pass, double* c);
int gloc_robust_weight(const gloc_robust_params* prm, uint32_t pass, double s2, double* w);

/* The plain entries' arguments with the robust block behind the method's own, and one more output: out_weight (may be
 * NULL), per candidate the weights' sum over the pair count of the final evaluation, 0 where the count is 0.  With kind
 * NONE every output equals the plain entry's bit for bit and out_weight is 1 where there are pairs.  GLOC_ERR_INVALID
 * beyond the plain entries', looked at before the handle: a null robust block; kind > 4; with a kind other than NONE,
 * scale <= 0 or not finite, scale_start negative, not finite or in (0, scale), anneal outside (0, 1) with a schedule. */
int gloc_reg_p2l_batch_ids_robust(gloc_reg* h, uint32_t src_scan_id, const uint32_t* tgt_scan_ids, size_t n, const float* init_T,
                                  const gloc_p2l_params* prm, const gloc_robust_params* robust, float* out_T, float* out_rmse,
                                  uint32_t* out_iters, int* out_status, float* out_weight);
int gloc_reg_gicp_batch_ids_robust(gloc_reg* h, uint32_t src_scan_id, const uint32_t* tgt_scan_ids, size_t n, const float* init_T,
                                   const gloc_gicp_params* prm, const gloc_robust_params* robust, float* out_T, float* out_rmse,
                                   uint32_t* out_iters, int* out_status, float* out_weight);
int gloc_reg_vgicp_batch_ids_robust(gloc_reg* h, uint32_t src_scan_id, const uint32_t* tgt_scan_ids, size_t n, const float* init_T,
                                    const gloc_vgicp_params* prm, const gloc_robust_params* robust, float* out_T, float* out_rmse,
                                    uint32_t* out_iters, int* out_status, float* out_weight);
/* One evaluation at T16 with the weights of c(pass): the plain entries' outputs (the squared sum and the count
 * unweighted) and out_wsum, the sum of the weights. */
int gloc_reg_p2l_system_robust(gloc_reg* h, uint32_t src_scan_id, uint32_t tgt_scan_id, const float* T16, const gloc_p2l_params* prm,
                               const gloc_robust_params* robust, uint32_t pass, double* out_H36, double* out_g6, double* out_sum_r2,
                               uint64_t* out_count, double* out_wsum);
int gloc_reg_gicp_system_robust(gloc_reg* h, uint32_t src_scan_id, uint32_t tgt_scan_id, const float* T16, const gloc_gicp_params* prm,
                                const gloc_robust_params* robust, uint32_t pass, double* out_H36, double* out_g6, double* out_sum,
                                uint64_t* out_count, double* out_wsum);
int gloc_reg_vgicp_system_robust(gloc_reg* h, uint32_t src_scan_id, uint32_t tgt_scan_id, const float* T16,
                                 const gloc_vgicp_params* prm, const gloc_robust_params* robust, uint32_t pass, double* out_H36,
                                 double* out_g6, double* out_sum, uint64_t* out_count, double* out_wsum);

/* ---- pair lists: many (source, target) pairs through one of the three refinements in ONE call ------------- *
 * The entries above take one source against n targets; a stream of queries, the loop-closure edges of a pose graph or a
 * multi-way registration hand over a LIST of pairs.  Row c is (src_scan_ids[c], tgt_scan_ids[c]) from init_T + 16 c
 * (init_T NULL: the identity), and every launch of the call -- the 1-NN pass, the accumulate kernel, the solve -- covers
 * all rows: one batch set-up, one launch sequence, one read-back.
 *
 * Row equality.  Row c is the result of the single-source entry for (src_scan_ids[c], &tgt_scan_ids[c], 1, init_T + 16 c):
 * gloc_reg_<m>_batch_ids with robust NULL, gloc_reg_<m>_batch_ids_robust otherwise.  Every output is equal BIT FOR BIT,
 * out_iters and out_status included.  robust NULL is the plain step, and out_weight is then left alone; a block of kind
 * NONE gives the same rows and out_weight 1 where there are pairs, as the _robust entries do.
 * Independence.  A row does not depend on the list it is in, on its position there or on how often its scans appear
 * elsewhere in the list, as sources, as targets or as both: a job is cut into work-groups of 256 consecutive source
 * slots, its sums are added in that order, and both depend on its own source alone.  A scan against itself is a legal
 * pair.  A target may or may not carry a target index: the same bits.  (A SOURCE that carries one is kept in kd order,
 * and its rows are those of the single-source entries on that scan as it is kept: the same pairs summed in another order.)
 * Absent target.  tgt_scan_ids[c] == UINT32_MAX is "no target", as in gloc_reg_batch_multi: the row is exactly that of an
 * empty target scan -- the guess, 0 iterations, status 2, rmse 0, weight 0.
 * Normals that scans lack are built first with normal_k, as the single-source entries do: the targets', and for
 * generalized and voxelized ICP every distinct source's.  A voxelized call builds one voxel map per distinct target.
 * Memory: the correspondences are kept as [n][the longest source of the list], so the call's workspace grows as n times
 * the LONGEST source, not as the sum of the sources; the partial sums are one row per work-group the list really has.
 *
 * The parameter blocks are checked before the handle: the method's own, then -- where it is not NULL -- the robust one.
 * GLOC_ERR_INVALID, before any device work and with the outputs untouched: a null src_scan_ids, tgt_scan_ids or out_T;
 * n outside [1, 4096]; an id the store does not know; a source, anywhere in the list, that is empty or too large.
 * GLOC_ERR_STATE: a batch in flight on the handle.  The call is synchronous and the scans are pinned for it.
 * out_rmse, out_iters, out_status and out_weight may be NULL. */
int gloc_reg_p2l_pairs(gloc_reg* h, const uint32_t* src_scan_ids, const uint32_t* tgt_scan_ids, size_t n, const float* init_T,
                       const gloc_p2l_params* prm, const gloc_robust_params* robust /* NULL: the plain step */, float* out_T,
                       float* out_rmse, uint32_t* out_iters, int* out_status, float* out_weight);
int gloc_reg_gicp_pairs(gloc_reg* h, const uint32_t* src_scan_ids, const uint32_t* tgt_scan_ids, size_t n, const float* init_T,
                        const gloc_gicp_params* prm, const gloc_robust_params* robust /* NULL: the plain step */, float* out_T,
                        float* out_rmse, uint32_t* out_iters, int* out_status, float* out_weight);
int gloc_reg_vgicp_pairs(gloc_reg* h, const uint32_t* src_scan_ids, const uint32_t* tgt_scan_ids, size_t n, const float* init_T,
                         const gloc_vgicp_params* prm, const gloc_robust_params* robust /* NULL: the plain step */, float* out_T,
                         float* out_rmse, uint32_t* out_iters, int* out_status, float* out_weight);

/* The system form of a pair list: steps 1 - 6 (1 - 4 for point-to-plane) ONCE per row at T + 16 c (T NULL: the identity),
 * every row in the one launch sequence -- one cold 1-NN pass (none for the voxelized form), one accumulate launch, one
 * read-back of all n rows.  Outputs per row: H (6 x 6 row-major, symmetric), g, the squared-residual sum, the number of
 * pairs and, where out_wsum is not NULL, the sum of the weights (the count with robust NULL).
 * Row c equals BIT FOR BIT the single-pair call on (src_scan_ids[c], tgt_scan_ids[c], T + 16 c): gloc_reg_<m>_system with
 * robust NULL, gloc_reg_<m>_system_robust with the same `pass` otherwise (pass is ignored with robust NULL).  A row whose
 * target is UINT32_MAX is the row of an empty target scan: all zeros.  Normals built on demand, one voxel map per distinct
 * target, the limit on n and the refusals are those of gloc_reg_<m>_pairs, with out_H36, out_g6, out_sum and out_count in
 * the place of out_T: none of them may be NULL. */
int gloc_reg_p2l_pairs_system(gloc_reg* h, const uint32_t* src_scan_ids, const uint32_t* tgt_scan_ids, size_t n, const float* T,
                              const gloc_p2l_params* prm, const gloc_robust_params* robust /* NULL: plain */, uint32_t pass,
                              double* out_H36 /* [n][36] */, double* out_g6 /* [n][6] */, double* out_sum /* [n] */,
                              uint64_t* out_count /* [n] */, double* out_wsum /* [n], may be NULL */);
int gloc_reg_gicp_pairs_system(gloc_reg* h, const uint32_t* src_scan_ids, const uint32_t* tgt_scan_ids, size_t n, const float* T,
                               const gloc_gicp_params* prm, const gloc_robust_params* robust /* NULL: plain */, uint32_t pass,
                               double* out_H36, double* out_g6, double* out_sum, uint64_t* out_count, double* out_wsum);
int gloc_reg_vgicp_pairs_system(gloc_reg* h, const uint32_t* src_scan_ids, const uint32_t* tgt_scan_ids, size_t n, const float* T,
                                const gloc_vgicp_params* prm, const gloc_robust_params* robust /* NULL: plain */, uint32_t pass,
                                double* out_H36, double* out_g6, double* out_sum, uint64_t* out_count, double* out_wsum);

/* ---- resident voxel maps: insert scans, prune, voxelized generalized ICP against them ---------------------- *
 * The voxelized refinement above builds the voxels of its targets in every call.  A resident map is those voxel
 * statistics -- count, mean, mean normal outer product -- as a target that lives across calls: it is owned by a
 * registration handle, scans of the handle's store are merged into it under poses, voxels leave it by distance and age,
 * and gloc_reg_vgicp_vmap refines against it without building anything (small_gicp's IncrementalVoxelMap, fast_gicp's
 * voxel maps and KISS-ICP's local map are maps of this kind).  Scan-to-map tracking after a global fix and LiDAR odometry
 * are its use; a submap (gloc_scan_store_add_submap) is a different object, a scan of one point per voxel.
 *   M1. A map has a resolution (fp32, > 0), a capacity in voxels (1 .. 2^24) and normal_k.  Its frame is whatever frame
 *       the caller's poses map into.  There is no min_points: every voxel with at least one point is a voxel.  Everything
 *       is allocated at creation and never moves: the voxel array [capacity], beside it per voxel the running sums (3 + 6
 *       doubles) and a stamp, and ONE open-addressing table of the smallest power of two >= 2 x capacity slots (at least
 *       16).  The table is never more than half full, so every probe ends at an empty slot; there are no tombstones:
 *       removal rebuilds the table (M5).
 *   M2. Insert of scan s under pose T (scan -> map, 16 fp32 row-major).  The scan's normals are built first with normal_k,
 *       by the rule of gloc_scan_store_build_normals, if it has none.  With T given every point, in upload order, is moved
 *       as p = R s + t in fp32 in the refinements' operation order (step 3 of the voxelized refinement), and m = R n is
 *       formed in fp64 from the fp32 values as ((R0 n0 + R1 n1) + R2 n2), the accumulate kernel's expression.  With T NULL
 *       point and normal are taken as they are, without arithmetic.  The voxel of p is found by step 2 (floorf(p * inv),
 *       |k| < 2^20); a non-finite or out-of-range p is in no voxel.
 *   M3. Per voxel the insert contributes n, s1 = sum (p - corner) and s2 = sum m m^T (six entries): fp64 sums in upload
 *       order, corner = k x resolution -- the sums of step 2.  A voxel new to the map takes the contribution as it is; a
 *       voxel already there gets N += n, S1 += s1, S2 += s2, one fp64 add per component per insert, in insert order.  Then
 *       mean = corner + S1 / N, Nbar = S2 / N, count = N, and the voxel's stamp becomes the map's insert counter after this
 *       insert (1-based).  So after exactly one insert with T NULL into an empty map the voxels equal
 *       gloc_reg_vgicp_voxels of that scan (same resolution, min_points 1) bit for bit.
 *   M4. An insert that would take the map above its capacity is refused with GLOC_ERR_NOMEM and the map is left exactly as
 *       it was: the new keys are counted against the table before anything is written.  gloc_reg_vmap_insert takes a list
 *       and is its single inserts in order: the first scan that does not fit is refused, the ones before it stay.
 *   M5. Prune removes a voxel if a rule is set and holds -- distance, center3 not NULL: |mean - c|^2 > max_dist^2 in fp64
 *       from the widened fp32 values; age, max_age > 0: n_inserts - stamp > max_age.  The survivors' values and stamps are
 *       untouched; the voxel array is compacted and the table rebuilt from them.  Pruning to empty is legal.
 *   M6. Export: the voxels sorted by (kx, ky, kz), as gloc_reg_vgicp_voxels lists them, and their stamps.  The count is
 *       returned even where the buffers are too small (GLOC_ERR_INVALID then), as by that entry.
 *   M7. gloc_reg_vgicp_vmap and _system are steps 3 - 10 of the voxelized refinement with the map's voxels in place of
 *       step 2's, through the same accumulate and solve kernels, robust as in gloc_reg_vgicp_pairs[_system].
 *       prm->resolution must equal the map's bit for bit and prm->min_points must be 1 (GLOC_ERR_INVALID); plane_eps,
 *       neighbors, the gate, max_iters and both eps are the call's.  Rows are equal to their single calls and independent
 *       of each other, as the pair lists' are.  Against a map that holds exactly one scan inserted with T NULL every
 *       output equals gloc_reg_vgicp_pairs / _pairs_system on (source, that scan) bit for bit.  A map id of 0xFFFFFFFF,
 *       or an empty map, gives the row of an empty target.
 *   M8. All calls are synchronous.  GLOC_ERR_STATE with a batch in flight on the handle; GLOC_ERR_INVALID, before any
 *       device work and with the outputs untouched, for an unknown or destroyed map id, null arguments or bad parameters.
 *       A map owes nothing to a scan once its insert has returned: the scan may be released.  Destroying the handle frees
 *       its maps.  Ids are not reused on a handle. */
typedef struct gloc_vmap_params {
  float resolution;    /* 1.0 m: the voxels' edge; must be > 0 */
  uint32_t capacity;   /* 1 << 18 voxels; 1 .. 2^24 */
  uint32_t normal_k;   /* 10: inserted scans without normals get them built with this k; 3 .. 16 */
  uint32_t reserved_;
} gloc_vmap_params;    /* 16 bytes */

typedef struct gloc_vmap_info {
  uint32_t n_voxels, capacity;
  uint32_t n_inserts;  /* scans inserted so far: what the stamps count in */
  float resolution;
  uint64_t n_points;   /* the sum of the voxels' counts */
} gloc_vmap_info;      /* 24 bytes */

void gloc_vmap_default_params(gloc_vmap_params* p);
int gloc_reg_vmap_create(gloc_reg* h, const gloc_vmap_params* prm, uint32_t* out_map_id);
int gloc_reg_vmap_destroy(gloc_reg* h, uint32_t map_id);
/* T [n][16] or NULL: M2's "as they are".  GLOC_ERR_NOMEM: M4. */
int gloc_reg_vmap_insert(gloc_reg* h, uint32_t map_id, const uint32_t* scan_ids, size_t n, const float* T);
/* center3 NULL: the distance rule is off; max_age 0: the age rule is off.  out_removed may be NULL. */
int gloc_reg_vmap_prune(gloc_reg* h, uint32_t map_id, const float* center3, float max_dist, uint32_t max_age, uint32_t* out_removed);
int gloc_reg_vmap_info(gloc_reg* h, uint32_t map_id, gloc_vmap_info* out);
/* M6.  n_voxels: how many there are (the arrays may be NULL to ask). */
int gloc_reg_vmap_voxels(gloc_reg* h, uint32_t map_id, size_t capacity, int32_t* out_key3, uint32_t* out_count, double* out_mean3,
                         double* out_nn6, uint32_t* out_stamp, size_t* n_voxels);
/* M7: row c is (src_scan_ids[c], map_ids[c]); arguments and outputs as gloc_reg_vgicp_pairs / _pairs_system. */
int gloc_reg_vgicp_vmap(gloc_reg* h, const uint32_t* src_scan_ids, const uint32_t* map_ids, size_t n, const float* init_T,
                        const gloc_vgicp_params* prm, const gloc_robust_params* robust /* NULL: the plain step */, float* out_T,
                        float* out_rmse, uint32_t* out_iters, int* out_status, float* out_weight);
int gloc_reg_vgicp_vmap_system(gloc_reg* h, const uint32_t* src_scan_ids, const uint32_t* map_ids, size_t n, const float* T,
                               const gloc_vgicp_params* prm, const gloc_robust_params* robust /* NULL: plain */, uint32_t pass,
                               double* out_H36, double* out_g6, double* out_sum, uint64_t* out_count, double* out_wsum);

/* ---- evaluation of registered pairs: overlap, RMSE and the 6 x 6 information matrix ---------------------- *
 * Every way of bringing a scan into a place's frame reports a quality figure of its own -- an RMS nearest-neighbour
 * distance, a plane residual, a Mahalanobis residual, an inlier count over descriptor matches -- and none compares two
 * poses of the same pair that came from two methods.  This entry evaluates a LIST of (source, target, pose) rows with the
 * method-independent point-to-point figures (Open3D's evaluate_registration and GetInformationMatrixFromPointClouds, PCL's
 * getFitnessScore, small_gicp's H): what a pose-graph back end needs per edge -- an overlap figure to keep or drop it, an
 * information matrix to weight it.  It reports numbers and decides nothing: no `ok`, no gate.  The executable contract is
 * the float64 restatement tests/eval_ref.py; parity with Open3D is unpinned (V4).
 *
 * Row c is (src_scan_ids[c], tgt_scan_ids[c]) at T + 16 c (row-major, source -> target; T NULL: the identity).  One row:
 *   V1. every source point s: p = R s + t in fp32 (the pose as given, the ICP's operation order: step 1 of the refinements);
 *   V2. j = the exact 1-NN of p in the target, d2 the search's fp32 squared distance (the ICP's search: same bits, same tie
 *       rule as every other entry);
 *   V3. the pair counts iff d2 is finite and d2 <= max_corr_dist x max_corr_dist, the product formed in fp32;
 *   V4. in fp64 from the fp32 values: e = p - q_j and, for T <- exp(xi) T with xi = (w, v), rotation first, J = [-[p]x , I]
 *       (generalized ICP's step 6):  info += J^T J, g += J^T e, sum += (ex ex + ey ey) + ez ez, count += 1.  Open3D builds J
 *       from the TARGET point q_j instead; at a registered pose the two differ by the residual;
 *   V5. fitness = (float)((double)count / (double)n_src), n_src the source scan's point count, rows with non-finite
 *       coordinates included (they are in no pair); rmse = (float)sqrt(sum / count), 0 when count = 0; info is symmetric,
 *       filled from its upper triangle as gloc_reg_<m>_system fills H;
 *   V6. independence and row equality as for gloc_reg_<m>_pairs: a job is cut into work-groups of 256 consecutive source
 *       slots and its partial sums are added in index order, so a row's bits do not depend on the list, on its position
 *       there or on whether the target carries a target index.  tgt_scan_ids[c] == UINT32_MAX or an empty target: count 0,
 *       fitness 0, rmse 0, info and g all zero.  A scan against itself is legal.
 * The reverse direction (target -> source, for a symmetric overlap) is another row: (tgt, src, T^-1).
 * Cost: ONE cold pass of the registration's exact 1-NN search over all rows, one accumulate launch, one read-back.
 *
 * The parameter block is checked before the handle.  GLOC_ERR_INVALID, before any device work and with the outputs
 * untouched: a null prm; max_corr_dist <= 0, NaN or infinite; null id arrays; all five outputs NULL (any four may be);
 * n outside [1, 4096]; an id the store does not know; a source that is empty or too large.  GLOC_ERR_STATE: a batch in
 * flight on the handle.  The call is synchronous and the scans are pinned for it. */
typedef struct gloc_eval_params {
  float max_corr_dist; /* 0.6 m = 3 x 0.2 m (registration/loop_detector.cpp:257, the library's inlier_thresh); must be > 0
                          and finite */
  uint32_t reserved_;
} gloc_eval_params;    /* 8 bytes */

void gloc_eval_default_params(gloc_eval_params* p);

int gloc_reg_evaluate_pairs(gloc_reg* h, const uint32_t* src_scan_ids, const uint32_t* tgt_scan_ids, size_t n,
                            const float* T /* [n][16] source -> target, NULL: identity */, const gloc_eval_params* prm,
                            float* out_fitness, float* out_rmse, uint32_t* out_count,
                            double* out_info36 /* [n][36] row-major, symmetric */, double* out_g6 /* [n][6] */);

/* ---- FPFH feature-based global registration ------------------------------------------------------------- *
 * The 3-D answer to "where is this scan, from nothing": local shape descriptors (Fast Point Feature Histograms: Rusu,
 * Blodow & Beetz; pcl::FPFHEstimation in its k-nearest form), descriptor matching, and the RANSAC stage of
 * gloc_reg_batch_* run on the descriptor matches instead of nearest-neighbour pairs under a guess (the idea of
 * pcl::SampleConsensusPrerejective).  It needs no initial pose and no level sensor; its pose is a START for one of the
 * refinements above (out_T as their init_T), not a result.  A stage a caller chooses; the default pipeline is unchanged.
 * The executable contract is the float64 restatement tests/fpfh_ref.py; parity with PCL is unpinned.
 *
 * F1  SPFH.  A point's list is its feature_k nearest neighbours within the scan, self included, ascending (d2, index) --
 *     the lists the normals are built from, d2 = ((dx dx + dy dy) + dz dz) in fp32.  Entry j != i is usable iff d2 > 0, both
 *     points are finite and both normals non-zero.  In fp64 from the fp32 inputs: dp = p_j - p_i, f4 = |dp|,
 *     a1 = n_i.dp / f4, a2 = n_j.dp / f4; if acos(min(|a1|, 1)) > acos(min(|a2|, 1)) the roles swap (n1 = n_j, n2 = n_i,
 *     dp = -dp, f3 = -a2), else n1 = n_i, n2 = n_j, f3 = a1; v = dp x n1, the pair is skipped if |v| = 0, v normalised;
 *     w = n1 x v; f2 = v.n2; f1 = atan2(w.n2, n1.n2).  Bins, each clamped to [0, 10]: floor(11 (f1 + pi) / (2 pi)),
 *     floor(11 (f2 + 1) / 2), floor(11 (f3 + 1) / 2).  The SPFH is the three count vectors and `used`, the pairs counted;
 *     its real form is counts x 100 / used.  A point with a zero normal or used = 0 has none.
 * F2  FPFH.  Over the usable entries j that have an SPFH, in list order: acc += SPFH_j x (1 / d2) in fp64; each of the
 *     three sub-histograms rescaled to sum to 100; 33 fp32 values.  The all-zero row means "no feature".
 * F3  Matching.  For every source row with a feature the target row with a feature at the smallest squared distance,
 *     defined in fp32, un-fused: acc = 0; for c in 0..32: t = a[c] - b[c]; acc = acc + t * t.  Ties: the smaller target
 *     index.  mutual: the same search target -> source; (i, j) is kept iff j's match is i.
 * F4  RANSAC.  The kept pairs in ascending source index are the correspondence list, M long; the RANSAC stage of
 *     gloc_reg_batch_* runs on it unchanged from the identity (3-point samples over [0, M) keyed by (seed, stream id, h),
 *     fp64 Kabsch, near-collinear samples skipped, inliers over the M pairs at inlier_thresh, most inliers then smallest
 *     h, the adaptive stop at ransac_confidence, the refit on the winner's inliers).  ok iff a valid hypothesis has at
 *     least max(3, ceil(min_inlier_ratio M)) inliers.  M < 3: the identity, ok = 0, 0 inliers. */
typedef struct gloc_fpfh_params {
  uint32_t normal_k;        /* 3..16, default 10 (registration/ground_estimator.cpp:79) */
  uint32_t feature_k;       /* 4..16, default 16: the list length, self included */
  uint32_t mutual;          /* default 1 */
  uint32_t ransac_iters;    /* default 3000 (registration/loop_detector.cpp:257); a cap, as in gloc_reg_params; >= 1 */
  float inlier_thresh;      /* 0.6 m */
  float min_inlier_ratio;   /* default 0: any valid hypothesis with >= 3 inliers is ok; plausibility belongs to the
                               refinement behind it */
  float ransac_confidence;  /* 0.99; outside (0, 1): every hypothesis is scored */
  uint32_t reserved_;
  uint64_t seed;            /* 1234 */
} gloc_fpfh_params;         /* 40 bytes */

void gloc_fpfh_default_params(gloc_fpfh_params* p);

/* Give a resident scan its FPFH features (F1, F2): 132 bytes per point in an allocation beside the scan, counted by
 * gloc_scan_store_bytes, freed with the scan, built at most once per (scan, normal_k, feature_k) -- a repeated call is a
 * no-op.  Normals the scan lacks are built first with normal_k; normals it has are used as they are when their k is
 * normal_k and rebuilt otherwise, under the rule of gloc_scan_store_build_normals (GLOC_ERR_STATE while a batch in flight
 * may read them; the same holds for rebuilding features with other k).  GLOC_ERR_INVALID: normal_k outside [3, 16],
 * feature_k outside [4, 16], a null store, an unknown id. */
int gloc_scan_store_build_fpfh(gloc_scan_store* st, uint32_t scan_id, uint32_t normal_k, uint32_t feature_k);
/* The features [n][33] in the order the scan was uploaded in.  GLOC_ERR_STATE: the scan has none. */
int gloc_scan_store_fpfh(gloc_scan_store* st, uint32_t scan_id, float* out_feat, size_t capacity_points);
/* Diagnostic, computed on demand from the scan's normals (GLOC_ERR_STATE without) and not kept: the SPFH counts
 * [n][33] and the pairs counted [n] (0: no SPFH), in upload order. */
int gloc_scan_store_spfh(gloc_scan_store* st, uint32_t scan_id, uint32_t feature_k, uint16_t* out_counts, uint32_t* out_used,
                         size_t capacity_points);

/* F3 on host buffers (a building block): src_feat [n_src][33], tgt_feat [n_tgt][33]; out_idx [n_src] the kept match of
 * every source row, UINT32_MAX for a row without a feature, without a target, or (mutual != 0) not its match's match;
 * out_d2 [n_src] the match's distance, +infinity where out_idx is UINT32_MAX (may be NULL). */
int gloc_reg_fpfh_match(gloc_reg* h, const float* src_feat, size_t n_src, const float* tgt_feat, size_t n_tgt, uint32_t mutual,
                        uint32_t* out_idx, float* out_d2);

/* Locate scan src_scan_id in each of the n targets (F3, F4): out_T [n][16] source -> target, out_inliers, out_n_pairs (M),
 * out_ok (each may be NULL but out_T).  stream_ids: the RANSAC stream of each job (NULL: 0 .. n - 1).  Features missing on
 * a scan are built first as gloc_scan_store_build_fpfh builds them.  One launch sequence covers all n jobs; job c equals
 * the single call with stream_ids[c], bit for bit, and the result does not depend on whether a scan carries a target
 * index.  The parameter block is checked before the handle.  GLOC_ERR_INVALID: null arguments, an unknown id, n outside
 * [1, 4096], normal_k outside [3, 16], feature_k outside [4, 16], ransac_iters = 0, inlier_thresh <= 0; GLOC_ERR_STATE: a
 * batch in flight on the handle. */
int gloc_reg_fpfh_batch_ids(gloc_reg* h, uint32_t src_scan_id, const uint32_t* tgt_scan_ids, size_t n, const uint32_t* stream_ids,
                            const gloc_fpfh_params* prm, float* out_T, uint32_t* out_inliers, uint32_t* out_n_pairs, int* out_ok);

/* ---- Correspondence-graph global registration on the FPFH matches ------------------------------------------ *
 * A second way from F3's match list to a pose, beside F4 and not instead of it.  Two correct matches (p_i -> q_i),
 * (p_j -> q_j) keep the distance between their points, two wrong ones almost never do: a compatibility graph over the
 * matches, in its second-order form (the idea of SC2-PCR, Chen et al. 2022; TEASER uses the same invariant), picks the
 * consistent set out without sampling.  n_seeds hypotheses instead of thousands, no random numbers, and integer
 * arithmetic up to the Kabsch fits.  The executable contract is tests/pairgraph_ref.py.
 *
 * The list is F4's: the kept pairs in ascending source index, M long; P_i the source point, Q_i the target point, fp32.
 * G1  Compatibility.  For i != j, in fp64 from the fp32 inputs: a = sqrt((dx dx + dy dy) + dz dz) over P_i - P_j, b
 *     likewise over Q; C_ij = 1 iff |a - b| < compat_thresh (the fp32 parameter widened to fp64).  C_ii = 0.  A pair with
 *     a non-finite coordinate is compatible with nothing.  C is symmetric by construction.  degree_i = sum_j C_ij.
 * G2  Second-order scores.  S_ij = C_ij |{k : C_ik and C_jk}|, an integer; score_i = sum_j S_ij, unsigned 64-bit.
 * G3  Seeds and consensus sets.  The seeds are the n_seeds pairs of largest score, ties to the smaller list position (rank
 *     r >= M: none).  A seed s with max_j S_sj = 0 gives no hypothesis (its set size is reported 0).  Else its set is
 *     {s} u {j : theta_den S_sj >= theta_num max_j S_sj and S_sj > 0} in ascending position; fewer than 3 members: no
 *     hypothesis.  The hypothesis is the fp64 Kabsch fit of the set -- raw moments, centroids, covariance and 3 x 3 SVD as
 *     the RANSAC refit forms them -- rounded to fp32.
 * G4  Choice and refit.  The inliers of a hypothesis are counted over all M pairs as F4 counts them (fp32, un-fused,
 *     < inlier_thresh^2).  The winner has the most inliers (at least one), then the smaller seed rank.  The refit on the
 *     winner's inliers and ok (at least max(3, ceil(min_inlier_ratio M)) inliers, the product in fp64) are F4's.  M < 3 or
 *     no hypothesis: the identity, ok = 0, 0 inliers. */
typedef struct gloc_fpfh_graph_params {
  uint32_t normal_k, feature_k, mutual; /* as gloc_fpfh_params: 10, 16, 1 */
  uint32_t n_seeds;                     /* default 64, 1..1024 */
  float compat_thresh;                  /* default 0.6 m, > 0 */
  float inlier_thresh;                  /* default 0.6 m, > 0 */
  float min_inlier_ratio;               /* default 0 */
  uint32_t theta_num, theta_den;        /* default 1, 2; 0 < num <= den */
  uint32_t reserved_;
} gloc_fpfh_graph_params;               /* 40 bytes */

void gloc_fpfh_graph_default_params(gloc_fpfh_graph_params* p);

/* Locate scan src_scan_id in each of the n targets (F3, then G1 - G4), shaped like gloc_reg_fpfh_batch_ids without
 * stream ids (nothing is random): out_T [n][16] source -> target, out_inliers, out_n_pairs (M), out_ok (each may be NULL
 * but out_T).  Job c equals its single call bit for bit; the result does not depend on whether a scan carries a target
 * index, nor on how the batch is cut to fit the graph workspace (1 GiB of bit matrices and seed rows in flight at a
 * time: n M_max ceil(M_max / 64) 8 bytes and 8 n_seeds M_max per job).  The parameter block is checked before the handle.
 * GLOC_ERR_INVALID: null arguments, an unknown id, n outside [1, 4096], a parameter outside its range; GLOC_ERR_NOMEM: one
 * list alone beyond the workspace (M ~ 90 000); GLOC_ERR_STATE: a batch in flight on the handle. */
int gloc_reg_fpfh_graph_batch_ids(gloc_reg* h, uint32_t src_scan_id, const uint32_t* tgt_scan_ids, size_t n,
                                  const gloc_fpfh_graph_params* prm, float* out_T, uint32_t* out_inliers, uint32_t* out_n_pairs,
                                  int* out_ok);

/* G1 - G4 on a host pair list (a building block and diagnostic): P, Q [m][3].  Any output may be NULL: out_degree [m],
 * out_score [m], out_seeds [n_seeds] (list positions, UINT32_MAX past rank m), out_set_sizes [n_seeds] (0: no set),
 * out_seed_inliers [n_seeds] (0: no hypothesis), out_T [16], out_inliers, out_winner_rank (UINT32_MAX: none), out_ok.
 * normal_k, feature_k and mutual are checked and not used. */
int gloc_reg_pair_graph(gloc_reg* h, const float* P, const float* Q, size_t m, const gloc_fpfh_graph_params* prm,
                        uint32_t* out_degree, uint64_t* out_score, uint32_t* out_seeds, uint32_t* out_set_sizes,
                        uint32_t* out_seed_inliers, float* out_T, uint32_t* out_inliers, uint32_t* out_winner_rank, int* out_ok);

/* ---- Radius-support FPFH ------------------------------------------------------------------------------------- *
 * The features above take every normal and every histogram from a k-NN list of at most 16 entries.  FPFH is customarily
 * used with a METRIC support instead -- all neighbours within a radius, capped at max_nn (pcl::Feature::setRadiusSearch,
 * Open3D's KDTreeSearchParamHybrid), about 2 x the voxel leaf for the normals and 5 x for the features, 30 and 100
 * neighbours.  These entries build the same features over such lists; F3, F4 and G1 - G4 are untouched.  A scan carries
 * ONE set of normals and ONE set of features, each tagged with the support it was built from -- k, or (radius, max_nn,
 * min_nn): a request for another support rebuilds, under the rule of gloc_scan_store_build_normals (GLOC_ERR_STATE while
 * a batch in flight may read them), a repeated request is a no-op, and radius features are valid only for the radius
 * normals they were built from.  The refinements that need normals (p2l, gicp) use whatever normals a scan has.  The
 * executable contract is tests/fpfh_radius_ref.py.
 *
 * R1  Lists.  d2(i, j) = ((dx dx + dy dy) + dz dz) in fp32, un-fused, as the k-NN lists compute it.  j belongs to i's
 *     neighbourhood iff d2 <= r2, r2 = r * r rounded to fp32.  A NaN distance is never inside: a point with a non-finite
 *     coordinate has an empty neighbourhood, itself included, and is in nobody's.  A finite point is always in its own;
 *     exact duplicates count with d2 = 0.  The list is the max_nn smallest entries of the neighbourhood in ascending
 *     (d2, index) order, the rest of the row 0xFFFFFFFF / FLT_MAX (the k-NN lists' padding).  count(i) is the size of the
 *     whole neighbourhood, before the cap.  Indices are upload-order indices; nothing depends on a target index.
 * R2  Normals.  The list of (normal_radius, normal_max_nn).  A point whose list holds fewer than normal_min_nn entries,
 *     self included, has no normal (zero row); every other point gets what gloc_scan_store_build_normals computes from
 *     that list: fp64 mean and covariance in list order, cyclic Jacobi, smallest eigenvalue with ties to the lower
 *     column, the flip towards the origin.  normal_min_nn >= 4 is part of the contract: three points span an exact
 *     plane, the normal is then perpendicular to every in-plane difference up to rounding, and F1's role test
 *     (acos|a1| > acos|a2|) hangs on the last bit.
 * R3  Features.  F1 and F2 word for word over the list of (feature_radius, feature_max_nn) and the normals of R2.  A row
 *     of all zeros still means "no feature". */
typedef struct gloc_fpfh_radius_params {
  float normal_radius;      /* default 1.0 m (2 x the 0.5 m leaf); > 0, finite */
  uint32_t normal_max_nn;   /* default 30;  normal_min_nn .. 128 */
  uint32_t normal_min_nn;   /* default 5;   4 .. normal_max_nn */
  float feature_radius;     /* default 2.5 m (5 x the leaf); > 0, finite */
  uint32_t feature_max_nn;  /* default 100; 4 .. 128 */
  uint32_t reserved_;       /* 0 */
} gloc_fpfh_radius_params;  /* 24 bytes */

void gloc_fpfh_radius_default_params(gloc_fpfh_radius_params* p);

/* R1 on a resident scan (a building block and diagnostic, nothing is kept): out_idx / out_d2 [n][max_nn], out_count [n],
 * in upload order; each may be NULL.  The arguments are checked before the handle.  GLOC_ERR_INVALID: radius not positive
 * and finite, max_nn outside [1, 128], a null store, an unknown id, capacity_points below the scan's size. */
int gloc_scan_store_radius_neighbors(gloc_scan_store* st, uint32_t scan_id, float radius, uint32_t max_nn, uint32_t* out_idx, float* out_d2,
                                     uint32_t* out_count, size_t capacity_points);
/* R2: the scan's normals from the lists of (radius, max_nn), none below min_nn entries; as gloc_scan_store_build_normals
 * otherwise (one set per scan: normals of another support are rebuilt, the features built from them dropped).
 * GLOC_ERR_INVALID: radius not positive and finite, min_nn outside [4, max_nn], max_nn above 128, a null store, an unknown id. */
int gloc_scan_store_build_normals_radius(gloc_scan_store* st, uint32_t scan_id, float radius, uint32_t max_nn, uint32_t min_nn);
/* R2 + R3: as gloc_scan_store_build_fpfh with this support; gloc_scan_store_fpfh downloads the features. */
int gloc_scan_store_build_fpfh_radius(gloc_scan_store* st, uint32_t scan_id, const gloc_fpfh_radius_params* prm);
/* as gloc_scan_store_spfh, over the radius list of (radius, max_nn in [4, 128]); needs normals (GLOC_ERR_STATE without) */
int gloc_scan_store_spfh_radius(gloc_scan_store* st, uint32_t scan_id, float radius, uint32_t max_nn, uint16_t* out_counts,
                                uint32_t* out_used, size_t capacity_points);
/* gloc_reg_fpfh_batch_ids / gloc_reg_fpfh_graph_batch_ids with features of this support: prm's normal_k and feature_k
 * are checked and not used; everything else is theirs, argument for argument.  Both parameter blocks are checked before
 * the handle. */
int gloc_reg_fpfh_batch_ids_radius(gloc_reg* h, uint32_t src_scan_id, const uint32_t* tgt_scan_ids, size_t n, const uint32_t* stream_ids,
                                   const gloc_fpfh_params* prm, const gloc_fpfh_radius_params* support, float* out_T, uint32_t* out_inliers,
                                   uint32_t* out_n_pairs, int* out_ok);
int gloc_reg_fpfh_graph_batch_ids_radius(gloc_reg* h, uint32_t src_scan_id, const uint32_t* tgt_scan_ids, size_t n,
                                         const gloc_fpfh_graph_params* prm, const gloc_fpfh_radius_params* support, float* out_T,
                                         uint32_t* out_inliers, uint32_t* out_n_pairs, int* out_ok);

/* ---- ISS keypoints and keypoint-restricted FPFH matching ----------------------------------------------------- *
 * F3 compares every source row with every target row.  FPFH registration is customarily run on KEYPOINTS instead:
 * Intrinsic Shape Signatures (Zhong 2009; pcl::ISSKeypoint3D, Open3D's compute_iss_keypoints) keeps the points whose
 * neighbourhood spreads in all three directions and distinctly so, and the matcher's work falls with K_src x K_tgt.
 * Opt-in: a scan gets keypoints only when asked, and only the two _keypoints batch entries read them.  The executable
 * contract is tests/iss_ref.py.
 *
 * I1  Saliency.  The list of point i is R1's list for (salient_radius, max_nn).  A point whose list holds fewer than
 *     min_nn entries, and any non-finite point (its list is empty), has saliency 0.  Otherwise, in fp64 from the fp32
 *     inputs and in list order: mean = sum / count; the covariance is the unnormalised sum of the outer products of
 *     (q - mean), its six upper-triangle sums formed as gloc_scan_store_build_normals forms them and mirrored; the
 *     eigenvalues are the diagonal the same cyclic Jacobi leaves, sorted l1 >= l2 >= l3.  The point is salient iff
 *     l3 > 0 && l2 < g21 l1 && l3 < g32 l2 (the fp32 gammas widened to fp64); its saliency is (float)l3, else 0.
 * I2  Non-maximum suppression, over the WHOLE neighbourhood (no capped list).  i is a keypoint iff its saliency is
 *     positive and no j != i with d2(i, j) <= r2 (R1's d2 and r2, from non_max_radius) has a larger saliency, or an equal
 *     one and j < i: among equal saliencies within the radius the lower upload index wins.
 * I3  The keypoint set is the keypoints in ascending upload-order index, K long.  A keypoint whose FPFH row is all zeros
 *     stays in the set and has "no feature", as before.
 * I4  Matching.  F3 word for word on feature tables in which every non-keypoint row counts as "no feature", on both
 *     sides and in the backward search of `mutual`; ties still go to the smaller target upload index.  F4's list is the
 *     kept pairs in ascending source index; F4 and G1 - G4 are unchanged.  K_src < 3: the identity, ok = 0, 0 inliers. */
typedef struct gloc_iss_params {
  float salient_radius;  /* default 3.0 m (6 x the 0.5 m leaf); > 0, finite */
  uint32_t max_nn;       /* default 128; min_nn .. 128 */
  uint32_t min_nn;       /* default 5;   3 .. max_nn */
  float non_max_radius;  /* default 2.0 m (4 x the leaf); > 0, finite */
  float gamma_21;        /* default 0.975; (0, 1] */
  float gamma_32;        /* default 0.975; (0, 1] */
} gloc_iss_params;       /* 24 bytes */

void gloc_iss_default_params(gloc_iss_params* p);

/* I1 as a diagnostic in upload order, nothing is kept: out_saliency [n], out_eig [n][3] the sorted fp64 eigenvalues (all
 * zeros where the list is too short); either may be NULL.  The parameters are checked before the handle.
 * GLOC_ERR_INVALID: a parameter outside its range, a null store, an unknown id, capacity_points below the scan's size. */
int gloc_scan_store_iss_saliency(gloc_scan_store* st, uint32_t scan_id, const gloc_iss_params* prm, float* out_saliency, double* out_eig,
                                 size_t capacity_points);
/* I1 - I3: the scan keeps its keypoint list (4 bytes per keypoint, and 132 more for the keypoints' feature rows gathered
 * into a table of their own whenever the scan has features; both counted by gloc_scan_store_bytes, freed with the scan),
 * tagged with the six parameters: a repeated request is a no-op, another parameter set rebuilds, GLOC_ERR_STATE while a
 * batch in flight may read the keypoints.  The list holds upload-order indices: building a target index does not change it. */
int gloc_scan_store_build_keypoints(gloc_scan_store* st, uint32_t scan_id, const gloc_iss_params* prm);
/* K, and the list in ascending order.  GLOC_ERR_STATE: the scan has no keypoints. */
int gloc_scan_store_keypoint_count(gloc_scan_store* st, uint32_t scan_id, size_t* out_k);
int gloc_scan_store_keypoints(gloc_scan_store* st, uint32_t scan_id, uint32_t* out_idx, size_t capacity);
/* Diagnostic: the keypoints' feature rows [K][33] in list order, as the matcher reads them (gathered again first when a
 * rebuild of the features dropped the table).  GLOC_ERR_STATE: the scan has no keypoints or no features. */
int gloc_scan_store_keypoint_fpfh(gloc_scan_store* st, uint32_t scan_id, float* out_feat, size_t capacity);
/* gloc_reg_fpfh_batch_ids_radius / gloc_reg_fpfh_graph_batch_ids_radius on the keypoints of `iss` alone (I4), argument
 * for argument; support == NULL: the k-mode features of prm.  Features and keypoints a scan lacks are built first.  All
 * parameter blocks are checked before the handle; job c equals its single call bit for bit, and the result does not
 * depend on target indices. */
int gloc_reg_fpfh_batch_ids_keypoints(gloc_reg* h, uint32_t src_scan_id, const uint32_t* tgt_scan_ids, size_t n, const uint32_t* stream_ids,
                                      const gloc_fpfh_params* prm, const gloc_fpfh_radius_params* support, const gloc_iss_params* iss,
                                      float* out_T, uint32_t* out_inliers, uint32_t* out_n_pairs, int* out_ok);
int gloc_reg_fpfh_graph_batch_ids_keypoints(gloc_reg* h, uint32_t src_scan_id, const uint32_t* tgt_scan_ids, size_t n,
                                            const gloc_fpfh_graph_params* prm, const gloc_fpfh_radius_params* support,
                                            const gloc_iss_params* iss, float* out_T, uint32_t* out_inliers, uint32_t* out_n_pairs,
                                            int* out_ok);

/* ---- Euclidean clusters and outlier filters of resident scans -------------------------------------------------- *
 * What a scan is customarily prepared with before it is described or registered (pcl::EuclideanClusterExtraction,
 * pcl::RadiusOutlierRemoval, pcl::StatisticalOutlierRemoval; Open3D's cluster_dbscan at min_points 1 and its two
 * remove_*_outlier): the connected components of the "within `tolerance`" graph, which drop the small blobs and keep the
 * structure, and the two neighbourhood filters.  Opt-in: nothing calls these unless asked, and a filter never changes a
 * scan -- its survivors become a NEW resident scan.  Every integer output is exact and every float output has a stated
 * summation order; the executable contract is tests/cluster_ref.py.  NONE below is 0xFFFFFFFF.
 *
 * E1  Graph.  The vertices are the points of the scan in upload order; i ~ j iff d2(i, j) <= r2, with R1's d2
 *     ((dx dx + dy dy) + dz dz in fp32, un-fused) and r2 = tolerance * tolerance rounded to fp32.  A point with a
 *     non-finite coordinate is a vertex of nothing, whatever r2 (an infinite r2 included): its root and cluster are NONE.
 *     Exact duplicates are neighbours (d2 = 0).  Nothing depends on whether the scan carries a target index.
 * E2  Components.  root(i) = the smallest upload index in i's connected component.
 * E3  Clusters.  size(c) = the component's point count.  A component is KEPT iff size >= max(min_size, 1) and
 *     (max_size == 0 or size <= max_size).  Kept components are ranked by descending size, ties by ascending root;
 *     cluster(i) = that rank, or NONE where i's component is not kept.
 * E4  Per kept cluster, in rank order: size; root; centroid = the fp64 sums of the widened fp32 coordinates divided by
 *     (double)size; min / max corner in fp32 (of equal zeros -0 is the smaller).  An ORDERED SUM here and in E6: the
 *     terms, in ascending upload index, are cut into runs of 64; a run's terms are added one by one from +0.0, then the
 *     runs' sums are added one by one, in run order, from +0.0.  E4's terms are the cluster's points.
 * E5  Radius outlier removal.  i stays iff it is finite and count(i) - 1 >= min_neighbors, count = R1's count for
 *     `ror_radius`: the whole neighbourhood, self included, before any cap.
 * E6  Statistical outlier removal.  The list of i is its k-NN list of mean_k + 1 entries, self included, ascending
 *     (d2, index), mean_k in [1, 15]; only finite distances enter a list, an entry a list cannot fill counts as FLT_MAX.
 *     m_i = (the fp64 sum of sqrt((double)d2) over the first mean_k entries of the list without i itself, in list
 *     order) / (double)mean_k.  Over the N finite points, as ordered sums (E4) whose terms are ALL the scan's points in
 *     upload order with +0.0 for a non-finite one: mu = sum(m_i) / N, sigma = sqrt(sum((m_i - mu) (m_i - mu)) / N) --
 *     population, two passes, fp64, nothing fused.  i stays iff it is finite and m_i <= mu + (double)std_mul * sigma.  A
 *     scan with fewer than mean_k + 1 finite points is refused.
 * E7  Derived scans.  The survivors of a filter, in upload order, become a new resident scan: exactly the scan
 *     gloc_scan_store_add_device makes of those points.  The range crop keeps i iff it is finite, not
 *     (x x + y y) + z z > max_range^2 (max_range > 0) and not (x x + y y) + z z < min_range^2 (min_range > 0), fp32
 *     un-fused as the submaps' max_range; the cluster stage keeps the points whose cluster is not NONE.
 *     gloc_scan_store_add_filtered runs its stages ONE AFTER THE OTHER, each on the survivors of the one before, in the
 *     order range crop, radius outlier removal, statistical outlier removal, clusters; a stage whose switch is zero is
 *     skipped.  Its result equals the chain of single-stage calls bit for bit.  A call in which nothing survives a stage
 *     is refused after that stage's device work and adds nothing. */
typedef struct gloc_cluster_params {
  float tolerance;     /* default 0.5 m; >= 0 and finite; 0: no cluster stage (refused by gloc_scan_store_cluster) */
  uint32_t min_size;   /* default 1 */
  uint32_t max_size;   /* default 0: no upper limit; else >= min_size */
  uint32_t reserved_;  /* 0 */
} gloc_cluster_params; /* 16 bytes */

void gloc_cluster_default_params(gloc_cluster_params* p);

/* E1 - E4 of a resident scan of n points, nothing is kept.  out_root / out_cluster [n] in upload order (capacity_points
 * entries each); out_size / out_cluster_root [n_kept], out_centroid3 [n_kept][3], out_lo3 / out_hi3 [n_kept][3] in rank
 * order (capacity_clusters rows each); n_components counts all components, n_kept the kept ones.  Every output may be
 * NULL.  The parameter block is checked before the handle.  GLOC_ERR_INVALID before any device work and with the outputs
 * untouched: a null block, tolerance not positive and finite, min_size > max_size != 0, reserved_ != 0, a null store, an
 * unknown id, a scan of 2^31 points or more.  A point buffer given with capacity_points < n, or a cluster buffer with
 * capacity_clusters < n_kept: GLOC_ERR_INVALID after the device work -- the two counts are returned, the buffers that are
 * too small are not written. */
int gloc_scan_store_cluster(gloc_scan_store* st, uint32_t scan_id, const gloc_cluster_params* prm, uint32_t* out_root,
                            uint32_t* out_cluster, size_t capacity_points, uint32_t* out_size, uint32_t* out_cluster_root,
                            double* out_centroid3, float* out_lo3, float* out_hi3, size_t capacity_clusters, uint32_t* n_components,
                            uint32_t* n_kept);

typedef struct gloc_scan_filter_params {
  float min_range, max_range;  /* <= 0: off; both set: min_range <= max_range */
  float ror_radius;            /* 0: off; else positive and finite */
  uint32_t ror_min_neighbors;
  uint32_t sor_mean_k;         /* 0: off; else 1 .. 15 */
  float sor_std_mul;           /* finite */
  gloc_cluster_params cluster; /* tolerance 0: off */
} gloc_scan_filter_params;     /* 40 bytes */

void gloc_scan_filter_default_params(gloc_scan_filter_params* p); /* everything off (cluster: min_size 1, max_size 0) */

typedef struct gloc_scan_filter_info {
  uint32_t points_in, after_range, after_ror, after_sor, after_cluster; /* a skipped stage repeats the count before it */
} gloc_scan_filter_info;

/* E7: *new_id is a new resident scan of what the stages of prm leave of scan base_id (all stages off: a copy).  info
 * may be NULL; on a refusal after device work it holds the counts up to the stage that left nothing.  The base scan is
 * only read; the call holds the store's mutex, returns when the scan is complete and has released every intermediate
 * scan.  The parameter block is checked before the handle.  GLOC_ERR_INVALID before any device work: a null block, a
 * radius or tolerance that is negative or not finite, min_size > max_size != 0, reserved_ != 0, sor_mean_k > 15,
 * sor_std_mul not finite, a non-finite range, min_range > max_range with both set, a null store or new_id, an unknown
 * id; after a stage's device work: fewer than sor_mean_k + 1 finite points at the statistical stage, no survivor.  A
 * call that fails adds nothing. */
int gloc_scan_store_add_filtered(gloc_scan_store* st, uint32_t base_id, const gloc_scan_filter_params* prm, uint32_t* new_id,
                                 gloc_scan_filter_info* info);

/* The primitive under E7: a new resident scan of rows idx[0 .. m) of scan base_id in the order given (indices may
 * repeat) -- a gather on the device, then the scan gloc_scan_store_add_device makes of those rows.  GLOC_ERR_INVALID
 * before any device work: a null argument, m = 0 or m >= 2^31, an unknown id, an index >= the scan's size. */
int gloc_scan_store_add_subset(gloc_scan_store* st, uint32_t base_id, const uint32_t* idx, size_t m, uint32_t* new_id);

/* ---- Fast Global Registration on the FPFH matches -------------------------------------------------------------- *
 * A third way from F3's match list to a pose, beside F4 and G1 - G4: Fast Global Registration (Zhou, Park, Koltun, ECCV
 * 2016; pcl and Open3D carry it beside their RANSAC routes).  A tuple test thins the matches, then ONE graduated-non-convexity
 * optimisation runs over the fixed correspondences with the Geman-McClure line process, its scale mu annealed from the
 * clouds' extent down to the match distance.  No hypotheses are drawn or scored and no neighbour is searched for behind
 * the matcher.  The executable contract is tests/fgr_ref.py.
 *
 * The list is F4's: the kept pairs in ascending source index, M long; P_i the source point, Q_i the target point, fp32.
 * R1  Tuple test (tuple_tries > 0).  For h = 0 .. tuple_tries - 1, (a, b, c) is F4's sample of (seed, stream id, h) over
 *     [0, M); a sample with two equal members is skipped.  For the edges (a, b), (b, c), (c, a), in fp64 from the fp32
 *     inputs: lp = sqrt((dx dx + dy dy) + dz dz) over P, lq likewise over Q.  The tuple passes iff every edge has
 *     s lp < lq and s lq < lp, s = tuple_scale widened to fp64: a non-finite coordinate or a zero-length edge fails
 *     without a special case.  The kept tuples are the first max_tuples passing ones in ascending h; mult_i is the number
 *     of times pair i occurs in them, n_tuples their count.  tuple_tries = 0: mult_i = 1 for every pair with six finite
 *     coordinates, else 0, and n_tuples = 0.
 * R2  Scale.  A = {i : mult_i > 0}, in ascending position.  c_P = sum mult_i P_i / sum mult_i over A in fp64, c_Q
 *     likewise; D^2 = max over A of max(|P_i - c_P|^2, |Q_i - c_Q|^2) (0 for an empty A); delta = max_corr_dist widened to
 *     fp64; mu_0 = max(D^2, delta^2).  Going into update k > 0 with k mod anneal_every = 0: mu <- max(mu / anneal_div,
 *     delta^2), one fp64 division per step, applied in sequence.
 * R3  Updates k = 0 .. max_iters - 1 from the identity, all fp64.  For i in A: x = R p_i + t, r = x - q_i,
 *     s2 = (r_x^2 + r_y^2) + r_z^2, l_i = the Geman-McClure weight of the robust block at (s2, mu_k), that is
 *     1 / (1 + s2 / mu_k)^2; J_i = [-[x]x | I], rotation first; H = sum mult_i l_i J^T J, g = sum mult_i l_i J^T r.  The
 *     solve is the Gauss-Newton refinements': degenerate with fewer than 3 members in A or a Cholesky pivot at or below
 *     1e-12 of the largest diagonal entry, else xi = -H^-1 g and T <- exp(xi) T by the same Rodrigues form.  A degenerate
 *     update leaves the pose of the update before it, sets status 2 and ends the loop; otherwise all max_iters updates run
 *     and status is 0.  There is no stop test.
 * R4  Verdict.  The pose is rounded to fp32; its inliers are counted over all M pairs as F4 counts them (fp32, un-fused,
 *     < inlier_thresh^2); there is no refit.  ok iff status = 0 and inliers >= max(3, ceil(min_inlier_ratio M)), the
 *     product in fp64.  M < 3, a test with no kept tuple, and any other degenerate first update: the identity, status 2,
 *     ok = 0, 0 inliers.  For M < 3 nothing is looked at: every mult_i is 0 whatever tuple_tries is, D^2 and the system are 0. */
typedef struct gloc_fgr_params {
  uint32_t normal_k, feature_k, mutual;  /* as gloc_fpfh_params: 10, 16, 1 */
  uint32_t tuple_tries;    /* default 10000; 0: no tuple test; <= 2^20 */
  uint32_t max_tuples;     /* default 1000; 1 .. 2^20 */
  float tuple_scale;       /* default 0.9; (0, 1] */
  uint32_t max_iters;      /* default 64; 1 .. 1024 */
  uint32_t anneal_every;   /* default 4; >= 1 */
  float anneal_div;        /* default 1.4; > 1, finite */
  float max_corr_dist;     /* default 0.6 m; > 0, finite */
  float inlier_thresh;     /* default 0.6 m; > 0 */
  float min_inlier_ratio;  /* default 0 */
  uint64_t seed;           /* default 1234; offset 48 */
} gloc_fgr_params;         /* 56 bytes */

void gloc_fgr_default_params(gloc_fgr_params* p);

/* Locate scan src_scan_id in each of the n targets (F3, then R1 - R4), shaped like gloc_reg_fpfh_batch_ids: out_T [n][16]
 * source -> target, out_inliers, out_n_pairs (M), out_ok (each may be NULL but out_T); stream_ids: the sample stream of
 * each job (NULL: 0 .. n - 1).  Job c equals its single call with stream_ids[c] bit for bit; the result does not depend
 * on whether a scan carries a target index.  The parameter block is checked before the handle.  GLOC_ERR_INVALID: null
 * arguments, an unknown id, n outside [1, 4096], a parameter outside its range (the message names the field);
 * GLOC_ERR_STATE: a batch in flight on the handle. */
int gloc_reg_fpfh_fgr_batch_ids(gloc_reg* h, uint32_t src_scan_id, const uint32_t* tgt_scan_ids, size_t n, const uint32_t* stream_ids,
                                const gloc_fgr_params* prm, float* out_T, uint32_t* out_inliers, uint32_t* out_n_pairs, int* out_ok);
/* ... with features of a radius support, and on the keypoints of `iss` alone (support == NULL there: the k-mode features
 * of prm): as the graph stage's two entries, argument for argument, plus stream_ids. */
int gloc_reg_fpfh_fgr_batch_ids_radius(gloc_reg* h, uint32_t src_scan_id, const uint32_t* tgt_scan_ids, size_t n, const uint32_t* stream_ids,
                                       const gloc_fgr_params* prm, const gloc_fpfh_radius_params* support, float* out_T,
                                       uint32_t* out_inliers, uint32_t* out_n_pairs, int* out_ok);
int gloc_reg_fpfh_fgr_batch_ids_keypoints(gloc_reg* h, uint32_t src_scan_id, const uint32_t* tgt_scan_ids, size_t n,
                                          const uint32_t* stream_ids, const gloc_fgr_params* prm, const gloc_fpfh_radius_params* support,
                                          const gloc_iss_params* iss, float* out_T, uint32_t* out_inliers, uint32_t* out_n_pairs,
                                          int* out_ok);

/* R1 - R4 on a host pair list (a building block and diagnostic): P, Q [m][3].  Every output but out_T may be NULL:
 * out_mult [m], out_n_tuples, out_d2 (D^2), out_system [27] (H's upper triangle, row-major, 21, then g, 6, of the last
 * update that was formed; zeros for m < 3), out_T [16], out_inliers, out_status (0 or 2), out_ok.  normal_k, feature_k
 * and mutual are checked and not used. */
int gloc_reg_fgr_pairs(gloc_reg* h, const float* P, const float* Q, size_t m, uint32_t stream_id, const gloc_fgr_params* prm,
                       uint32_t* out_mult, uint32_t* out_n_tuples, double* out_d2, double* out_system, float* out_T,
                       uint32_t* out_inliers, int* out_status, int* out_ok);

/* ============================ NetVLAD-FC pooling head ("next" row N2) ===================== *
 * Replaces NetVLAD.forward of the reference (model/netvlad_fc.py:73-109, built without gating at
 * main.py:594) -- the tail of the TorchScript module RpyPCLoopDetector::get_place_feature runs
 * (registration/loop_detector.cpp:152-163): per-position L2 normalisation, 1x1-conv soft assignment,
 * residual aggregation to `clusters` x `dim`, intra-normalisation, L2, FC to `out_dim`.
 * conv_w [clusters][dim], conv_b [clusters] or NULL (vladv2), centroids [clusters][dim],
 * fc_w [clusters*dim][out_dim] (hidden1_weights), all row-major fp32, copied to the device.
 * feat: n feature maps in NCHW order, [n][dim][hw]; out: [n][out_dim].  fp32 throughout.
 * Limits, checked by gloc_vlad_create (GLOC_ERR_INVALID, *out = NULL): 1 <= clusters <= 64; 1 <= dim <= 560 and one
 * tile of 64 positions must fit the 160 KiB of LDS, 65 * (dim + roundup16(clusters)) + 576 <= 40960 floats (more than 48
 * clusters: dim <= 557); 1 <= out_dim <= 65536, and <= 16384 with gating (gloc_vlad_set_gating).  The forward calls refuse
 * n = 0, hw = 0, n > 2^20 and hw > 2^24 (GLOC_ERR_INVALID). */
typedef struct gloc_vlad gloc_vlad;
int gloc_vlad_create(int device, size_t dim, size_t clusters, size_t out_dim, const float* conv_w,
                     const float* conv_b, const float* centroids, const float* fc_w,
                     int normalize_input, gloc_vlad** out);
/* Optional GatingContext after the FC (model/netvlad_fc.py:106-107,120-146; off in the reference's constructor
 * call, main.py:594): out = y * sigmoid((y W) * scale + shift), W [out_dim][out_dim] = gating_weights.  With
 * add_batch_norm (eval mode) scale = bn.weight / sqrt(bn.running_var + eps), shift = bn.bias -
 * bn.running_mean * scale; without, scale = 1, shift = gating_biases.  gating_w = NULL switches it off. */
int gloc_vlad_set_gating(gloc_vlad* h, const float* gating_w, const float* scale, const float* shift);
int gloc_vlad_destroy(gloc_vlad* h);
int gloc_vlad_set_stream(gloc_vlad* h, void* hip_stream);
int gloc_vlad_forward(gloc_vlad* h, const float* feat, size_t n, size_t hw, float* out);
int gloc_vlad_forward_device(gloc_vlad* h, const float* d_feat, size_t n, size_t hw, float* d_out);
int gloc_vlad_set_profile(gloc_vlad* h, int enable);
/* kernel families: "vlad_tile", "vlad_cluster", "vlad_fc", "vlad_gate" */
int gloc_vlad_profile(gloc_vlad* h, const char* kernel, double* total_ms, uint64_t* launches);

/* ============================ VGG16 place-descriptor encoder ============================= *
 * The encoder of the reference's i2i model, VGG16 features[:-2] (s2s_libtorch/gen_libtorch_i2i.py:36-60,
 * main.py:531-541): 13 3x3 convolutions (pad 1, stride 1, bias) with ReLU and four 2x2 max-pools, the last
 * convolution (conv5_3) without ReLU or pool.  Its input is the BEV tensor (gloc_bev, GLOC_BEV_F32_CHW) and its output
 * feeds gloc_vlad_forward_device (dim 512) as it is: together the TorchScript module RpyPCLoopDetector::get_place_feature
 * runs (registration/loop_detector.cpp:137-172).  Layers 0..12: Cin -> Cout = 3 -> 64, 64 -> 64 (pool), 64 -> 128,
 * 128 -> 128 (pool), 128 -> 256, 256 -> 256, 256 -> 256 (pool), 256 -> 512, 512 -> 512, 512 -> 512 (pool), 3 x 512 -> 512.
 * fp32 in and out.  Inside, each convolution is an implicit GEMM on the bf16 matrix cores with both operands split in
 * two bf16 halves (hi + lo, three products; the weights are split when they are set).  Contract for arbitrary fp32
 * input: max|out - fp32 reference| <= 1e-4 max|reference| per layer and for the whole encoder.
 * Each output has a fixed summation order: a batch gives the same bits as single calls. */
typedef struct gloc_vgg gloc_vgg;
int gloc_vgg_create(int device, gloc_vgg** out);
int gloc_vgg_destroy(gloc_vgg* h);
int gloc_vgg_set_stream(gloc_vgg* h, void* hip_stream);
int gloc_vgg_synchronize(gloc_vgg* h);
/* Cin, Cout, ReLU and pool of layer `layer` (0..12); needs no handle and no device.  Any pointer may be NULL. */
int gloc_vgg_layer_shape(int layer, uint32_t* cin, uint32_t* cout, int* relu, int* pool);
/* w [Cout][Cin][3][3] (torch's Conv2d layout), b [Cout], host fp32; copied and re-laid on the device before this
 * returns.  Every forward call needs the weights of the layers it runs (GLOC_ERR_STATE without). */
int gloc_vgg_set_layer(gloc_vgg* h, int layer, const float* w, const float* b);
/* images [n][3][H][W] -> out [n][512][H/16][W/16], NCHW fp32; H and W multiples of 16 (GLOC_ERR_INVALID otherwise).
 * Host buffers, synchronous. */
int gloc_vgg_forward(gloc_vgg* h, const float* images, size_t n, uint32_t H, uint32_t W, float* out);
/* The same on device buffers, on the handle's stream, without synchronisation. */
int gloc_vgg_forward_device(gloc_vgg* h, const float* d_images, size_t n, uint32_t H, uint32_t W, float* d_out);
/* One layer with its own epilogue (ReLU, pool) on device buffers: d_in [n][Cin][H][W] -> d_out [n][Cout][Ho][Wo],
 * NCHW fp32, Ho, Wo = H/2, W/2 for a pooled layer (which needs even H and W), else H, W.  Any H, W in [1, 8192]. */
int gloc_vgg_forward_layer(gloc_vgg* h, int layer, const float* d_in, size_t n, uint32_t H, uint32_t W, float* d_out);
int gloc_vgg_set_profile(gloc_vgg* h, int enable);
/* kernel families: "vgg_conv0" .. "vgg_conv12" (one per layer), "vgg_layout" (forward_layer's NCHW -> NHWC) */
int gloc_vgg_profile(gloc_vgg* h, const char* kernel, double* total_ms, uint64_t* launches);
int gloc_vgg_profile_reset(gloc_vgg* h);

/* ============================ BEV occupancy projection ("next" row N1) ==================== *
 * Replaces RpyPCLoopDetector::get_projected_grid + crop_pad_occupancy + the tensor packing of
 * get_place_feature (registration/loop_detector.cpp:83-106,122-151): one scan inserted into a fresh
 * Submap3D (3d/submap_3d.cpp:162-177, 3d/range_data_inserter_3d.cpp:27-78) and x-ray projected
 * (ProjectToCvMat, 3d/submap_3d.cpp:238-326), then centred-cropped / padded to the network's input
 * size.  Output is byte-identical to the reference's: a pixel is 0 where the column holds two or
 * more distinct hit voxels, else 255; the padding is (255, 0, 0) (cv::Mat::ones sets channel 0
 * only).  Scans are independent: a batch is n_scans scans back to back with host offsets. */
typedef struct gloc_bev gloc_bev;

enum {
  GLOC_BEV_U8_HWC3 = 0, /* [out_height][out_width][3] u8: crop_pad_occupancy's cv::Mat (CV_8UC3) */
  GLOC_BEV_F32_CHW = 1  /* [3][out_height][out_width] f32 in {0,1}: the module's input tensor */
};

typedef struct gloc_bev_params {
  float resolution;    /* 0.2 m: high_resolution_, loop_detector.h:116 */
  float max_range;     /* 100 m: loop_detector.cpp:113 and high_resolution_max_range_, loop_detector.h:115 */
  uint32_t out_width;  /* 768: loop_detector.cpp:142 */
  uint32_t out_height; /* 768: loop_detector.cpp:143 */
  uint32_t format;     /* GLOC_BEV_* */
  uint8_t pad_bgr[3];  /* 255, 0, 0: loop_detector.cpp:84 */
  uint8_t reserved_;
} gloc_bev_params;

typedef struct gloc_bev_info {
  int32_t min_ix, min_iy, max_ix, max_iy; /* voxel-index box of the occupied columns */
  uint32_t width, height;                 /* size of the uncropped image (occupancy_grid) */
  uint32_t n_returns;                     /* points kept by both range tests */
  uint32_t empty;                         /* 1: no point kept (the reference aborts); image = padding */
  double ox, oy, resolution;              /* xy_res: min index * resolution, loop_detector.cpp:133 */
} gloc_bev_info;

int gloc_bev_default_params(gloc_bev_params* p);
int gloc_bev_create(int device, gloc_bev** out);
int gloc_bev_destroy(gloc_bev* h);
int gloc_bev_set_stream(gloc_bev* h, void* hip_stream);
int gloc_bev_synchronize(gloc_bev* h);
/* One scan, host buffers: xyz = n points, stride_floats apart (3 packed, 4 for x y z i). */
int gloc_bev_project(gloc_bev* h, const float* xyz, size_t n, size_t stride_floats,
                     const gloc_bev_params* p, void* out_image, gloc_bev_info* info);
/* n_scans scans, device buffers: scan i = points [offsets[i], offsets[i+1]) of d_xyz (offsets on
 * the host, in points); d_out_images holds n_scans images back to back.  infos (host, n_scans) may
 * be NULL, in which case the call does not synchronise. */
int gloc_bev_project_batch_device(gloc_bev* h, const float* d_xyz, const uint64_t* offsets,
                                  size_t n_scans, size_t stride_floats, const gloc_bev_params* p,
                                  void* d_out_images, gloc_bev_info* infos);
/* The uncropped single-channel image of scan `scan` of the last projection (the occupancy_grid
 * get_place_feature hands back, loop_detector.cpp:139-140): [height][width] u8 into `out`. */
int gloc_bev_raw_image(gloc_bev* h, size_t scan, uint8_t* out, size_t capacity);
/* Device pointer of the column flags of scan `scan` of the last projection: flags[(iy + R) * S + (ix + R)]
 * != 0 iff the BEV pixel of voxel column (ix, iy) is occupied (value 0 in the image).  Valid until the
 * next projection on this handle; used by the coarse matcher to stay on the device. */
int gloc_bev_device_flags(gloc_bev* h, size_t scan, const uint8_t** d_flags, int* R, int* S);
int gloc_bev_set_profile(gloc_bev* h, int enable);
/* kernel families: "bev_clear", "bev_mark", "bev_flag", "bev_image" */
int gloc_bev_profile(gloc_bev* h, const char* kernel, double* total_ms, uint64_t* launches);

/* ============================ PointPillar scan front end ================================= *
 * The non-CNN head of the reference's scan descriptor PointPillarVLAD (exported by
 * s2s_libtorch/gen_libtorch_pointpillar.py, timed by s2s_libtorch/s2s_feature_extract.cpp):
 *  - gloc_pillar_inputs*: points_to_voxels and the traced model's input (model/voxel.py:23-133,
 *    gen_libtorch_pointpillar.py:47-62), [P][16] per scan: x y z i, the voxel's count of unpadded rows,
 *    p - centroid, centroid, p - voxel centre, voxel index (as a float), mask.  Bit for bit the reference
 *    module's on the CPU (tests/pillar_ref.py).  The index is x-major, x*gy*gz + y*gz + z
 *    (raval_index, voxel.py:14-20), not the C++ demo's layout.
 *  - gloc_pillar_canvas*: the PointNet (Conv1d 14 -> 64, BatchNorm1d eval, ReLU) times the row mask, and its
 *    mean per voxel over every row of the voxel (model/s2s_merged.py:113-127,204-218): [64][nv] per scan,
 *    nv = gx*gy*gz, empty voxels 0.  Sums in fp64 in a fixed order: the same bits on every run.
 * A scan is its first num_points points, then zero rows with mask 0 (pad_or_trim_to_np, dataset/kitti_s2s.py:
 * 222-227).  Points are x y z i, stride_floats >= 4 apart; a batch is n_scans scans back to back with host
 * offsets in points, as the BEV calls.  Outputs are scans back to back, 16-byte aligned. */
typedef struct gloc_pillar gloc_pillar;

enum {
  GLOC_PILLAR_MASK_INPUT = 0, /* features times input channel 15, the caller's mask (the traced model, s2s_merged.py:204-206) */
  GLOC_PILLAR_MASK_VALID = 1  /* features times 1 - padding (the training forward, model/pointpillar.py:199) */
};

typedef struct gloc_pillar_params {
  float xbound[3];     /* lo, hi, res: -35, 35, 0.5 m (gen_libtorch_pointpillar.py:27) */
  float ybound[3];     /* -20, 20, 0.5 m (:28) */
  float zbound[3];     /* -10, 10, 20 m (:29): one cell */
  uint32_t num_points; /* P = 122480 rows per scan (dataset/kitti_s2s.py:222-227, s2s_feature_extract.cpp:143) */
  uint32_t mask_mode;  /* GLOC_PILLAR_MASK_INPUT (default) or GLOC_PILLAR_MASK_VALID; canvas only */
} gloc_pillar_params;

int gloc_pillar_default_params(gloc_pillar_params* p);
int gloc_pillar_create(int device, gloc_pillar** out);
int gloc_pillar_destroy(gloc_pillar* h);
int gloc_pillar_set_stream(gloc_pillar* h, void* hip_stream);
int gloc_pillar_synchronize(gloc_pillar* h);
/* PointNet weights: w [64][14] (pn.pointnet.0.weight), BatchNorm1d weight, bias, running mean and variance [64],
 * eps (1e-5, torch's default).  Needed by the canvas calls (GLOC_ERR_STATE without). */
int gloc_pillar_set_pointnet(gloc_pillar* h, const float* w, const float* bn_weight, const float* bn_bias,
                             const float* bn_mean, const float* bn_var, float eps);
/* Host buffers: out [n_scans][num_points][16]. */
int gloc_pillar_inputs(gloc_pillar* h, const float* pts, const uint64_t* offsets, size_t n_scans, size_t stride_floats,
                       const gloc_pillar_params* p, float* out);
/* Device buffers on the handle's stream, no synchronisation. */
int gloc_pillar_inputs_device(gloc_pillar* h, const float* d_pts, const uint64_t* offsets, size_t n_scans,
                              size_t stride_floats, const gloc_pillar_params* p, float* d_out);
/* Host buffers: out [n_scans][64][gx*gy*gz]. */
int gloc_pillar_canvas(gloc_pillar* h, const float* pts, const uint64_t* offsets, size_t n_scans, size_t stride_floats,
                       const gloc_pillar_params* p, float* out);
int gloc_pillar_canvas_device(gloc_pillar* h, const float* d_pts, const uint64_t* offsets, size_t n_scans,
                              size_t stride_floats, const gloc_pillar_params* p, float* d_out);
/* The 2-D backbone behind the canvas, PointPillarTest after the scatter-mean in vlad_mode (model/s2s_merged.py:
 * 152-188,219-247): 13 convolutions 3x3, pad 1, no bias, each followed by BatchNorm2d in eval mode and (but the last)
 * ReLU.  Layers: 0-1 block1 64 -> 64; 2-4 block2 64 -> 128 (stride 2), 128 -> 128 x 2; 5-7 block3 128 -> 256
 * (stride 2), 256 -> 256 x 2; 8 up1 64 -> 64 on block1's output; 9 up2 128 -> 128 on block2's output upsampled x 2;
 * 10 up3 256 -> 256 on block3's output upsampled x 4 (bilinear, align_corners=True); 11 conv_out.0 448 -> 256 on the
 * concatenation of up1, up2, up3; 12 conv_out.3 256 -> 128 without ReLU.  The canvas [64][gx*gy] is viewed as
 * [64][H = gx][W = gy]; the output is .transpose(3, 2) of the last layer's, [128][gy][gx]: gloc_vlad_forward_device's
 * [n][128][hw] with hw = gy*gx.  Inside, each convolution is an implicit GEMM on the bf16 matrix cores with both
 * operands split in two bf16 halves (three products, as gloc_vgg); BatchNorm is applied to the fp32 sums.  Contract:
 * max|out - fp32 reference| <= 1e-4 max|reference| per layer and for the whole backbone.  Every
 * output has a fixed summation order: a batch gives the same bits as single calls. */
/* Cin, Cout, stride and ReLU of backbone layer `layer` (0..12); needs no handle and no device.  Any pointer may be NULL. */
int gloc_pillar_backbone_layer_shape(int layer, uint32_t* cin, uint32_t* cout, int* stride, int* relu);
/* w [Cout][Cin][3][3] (torch's Conv2d layout), BatchNorm2d weight, bias, running mean and variance [Cout], eps (1e-5,
 * torch's default); host fp32, copied and re-laid on the device before this returns.  The backbone and feature calls
 * need all 13 layers (GLOC_ERR_STATE without). */
int gloc_pillar_set_backbone_layer(gloc_pillar* h, int layer, const float* w, const float* bn_weight,
                                   const float* bn_bias, const float* bn_mean, const float* bn_var, float eps);
/* Device buffers on the handle's stream: canvas [n][64][gx*gy] -> out [n][128][gy*gx].  gx and gy multiples of 4 in
 * [4, 4096] (up2 and up3 must give block1's size back); GLOC_ERR_INVALID otherwise. */
int gloc_pillar_backbone_device(gloc_pillar* h, const float* d_canvas, size_t n, uint32_t gx, uint32_t gy,
                                float* d_out);
/* One layer with its BatchNorm and ReLU on device buffers, NCHW fp32: d_in [n][Cin][H][W] -> d_out [n][Cout][Ho][Wo],
 * Ho = (H - 1) / stride + 1 (likewise Wo).  Layers 9 and 10 take their input before the upsample: Ho = 2H, 4H.
 * Any H, W in [1, 4096] (after the upsample).  For tests and per-layer timing. */
int gloc_pillar_backbone_layer_device(gloc_pillar* h, int layer, const float* d_in, size_t n, uint32_t H, uint32_t W,
                                      float* d_out);
/* The backbone's bilinear upsample (nn.Upsample(scale_factor=factor, mode="bilinear", align_corners=True)) on its own,
 * NCHW: d_in [n][C][H][W] -> d_out [n][C][factor*H][factor*W].  For tests. */
int gloc_pillar_upsample_device(gloc_pillar* h, const float* d_in, size_t n, uint32_t C, uint32_t H, uint32_t W,
                                uint32_t factor, float* d_out);
/* Scans -> canvas -> backbone in one call: out [n_scans][128][gy*gx], ready for gloc_vlad_forward_device (dim 128).
 * The grid must give gz = 1 and gx, gy as gloc_pillar_backbone_device needs (GLOC_ERR_INVALID otherwise); needs the
 * PointNet and all 13 backbone layers (GLOC_ERR_STATE).  Host buffers, synchronous. */
int gloc_pillar_features(gloc_pillar* h, const float* pts, const uint64_t* offsets, size_t n_scans, size_t stride_floats,
                         const gloc_pillar_params* p, float* out);
/* The same on device buffers, on the handle's stream, without synchronisation. */
int gloc_pillar_features_device(gloc_pillar* h, const float* d_pts, const uint64_t* offsets, size_t n_scans,
                                size_t stride_floats, const gloc_pillar_params* p, float* d_out);
int gloc_pillar_set_profile(gloc_pillar* h, int enable);
/* kernel families: "pillar_classify", "pillar_sort", "pillar_runs", "pillar_voxel", "pillar_gather",
 * "pillar_partial", "pillar_canvas"; the backbone's "pillar_conv0" .. "pillar_conv12" (one per layer),
 * "pillar_upsample" (in front of layers 9 and 10), "pillar_layout" (the canvas or a layer's NCHW input to NHWC) */
int gloc_pillar_profile(gloc_pillar* h, const char* kernel, double* total_ms, uint64_t* launches);
int gloc_pillar_profile_reset(gloc_pillar* h);

/* ============================ coarse global (x, y, yaw) match (row a-12) =================== *
 * Replaces RpyPCLoopDetector::match(q_grid, db_idx, xy_yaw, scale) (registration/loop_detector.cpp:186-288):
 * the coarse pose of the query in a database place's frame from their two BEV occupancy images,
 * p_db = R(yaw) p_q + (x, y).  The reference finds it with SURF keypoints + FLANN matching + a RANSAC
 * partial-affine fit (OpenCV + contrib, absent here); this finds it with an exhaustive integer search on
 * the GPU -- every yaw step x every shift, scored by how many occupied query cells land on occupied
 * database cells (coarse_kernels.hpp) -- so a reverse-direction revisit is handled as well as a small
 * offset, and a scale estimate with the reference's |1 - scale| < 0.1 acceptance on top (round 3).
 * The result seeds the 3-D registration (init_T of gloc_reg_batch*), as the reference seeds its pose
 * composition (global_localization.cpp:526-570).  Parity: unpinned upstream (third-party arithmetic, no
 * fixtures); oracle/coarse_oracle.c states the search step by step and the GPU equals it exactly. */
typedef struct gloc_coarse gloc_coarse;

typedef struct gloc_coarse_params {
  float resolution;    /* 0.2 m: the BEV pixel (loop_detector.h:116) */
  uint32_t cell_px;    /* 2: a search cell is cell_px x cell_px pixels (0.4 m) */
  uint32_t n_yaw;      /* 360 yaw steps */
  uint32_t max_shift;  /* 64 cells: |x|, |y| <= 25.6 m */
  uint32_t top_yaw;    /* 12: yaw steps verified in 2-D (the identity is always verified too) */
  uint32_t refine;     /* 4 cells: 2-D window around the best x / y lags */
  float min_overlap;   /* 0.25: ok iff overlapping cells >= this x occupied query cells (and >= 16 cells) */
  uint32_t reserved_;
} gloc_coarse_params;

int gloc_coarse_default_params(gloc_coarse_params* p);
int gloc_coarse_create(int device, gloc_coarse** out);
int gloc_coarse_destroy(gloc_coarse* h);
/* A place's grid from its occupancy image as get_projected_grid returns it (OccupancyGrid of
 * loop_detector.h:36-39: [height][width] u8, below 100 = occupied as the reference's threshold,
 * ox_oy_res) -- what add_keyframe keeps in db_grids_ (loop_detector.cpp:16-19). */
int gloc_coarse_add_image(gloc_coarse* h, const uint8_t* occupancy, uint32_t width, uint32_t height, float ox,
                          float oy, float resolution, const gloc_coarse_params* params, uint32_t* grid_id);
/* The same straight from the scan (BEV projection at 0.2 m / 100 m on the device, no image round trip). */
int gloc_coarse_add_scan(gloc_coarse* h, const float* xyz, size_t n, size_t stride_floats,
                         const gloc_coarse_params* params, uint32_t* grid_id);
/* ... or from a scan resident in a scan store on the same device (no host copy of the points needed). */
int gloc_coarse_add_store_scan(gloc_coarse* h, gloc_scan_store* store, uint32_t scan_id,
                               const gloc_coarse_params* params, uint32_t* grid_id);
/* n scans of the store in one launch sequence (the query scans of a step, a database being loaded): two
 * synchronisations for the whole batch instead of three per grid. */
int gloc_coarse_add_store_scans(gloc_coarse* h, gloc_scan_store* store, const uint32_t* scan_ids, size_t n,
                                const gloc_coarse_params* params, uint32_t* grid_ids);
int gloc_coarse_release(gloc_coarse* h, uint32_t grid_id);
/* Occupied cells of a grid ((v << 16) | u, u / v in [0, 512): cell u spans the pixels
 * (u - 256) cell_px .. + cell_px - 1); out_cells may be NULL to get the count only. */
int gloc_coarse_cells(gloc_coarse* h, uint32_t grid_id, uint32_t* n_cells, uint32_t* out_cells,
                      size_t capacity);
/* One query grid against n_db database grids: out_xy_yaw [n_db][3] = (x, y, yaw in (-pi, pi]),
 * out_ratio = overlapping / occupied query cells, out_scale = the `scale` of the reference's match (the similarity
 * factor cv::estimateAffinePartial2D fits, loop_detector.cpp:262-266): here the factor in 0.88 .. 1.12 by which the
 * query, scaled about the sensor under the chosen rotation, overlaps the database grid most (parabola-refined; an end of
 * the range means "10 % or more off"; 0: no overlap at all); out_ok = enough overlap
 * AND |1 - scale| < 0.1, the reference's acceptance (loop_detector.cpp:268-272).  Any of the three may be NULL. */
int gloc_coarse_match(gloc_coarse* h, uint32_t q_grid, const uint32_t* db_grids, size_t n_db,
                      const gloc_coarse_params* params, float* out_xy_yaw, float* out_ratio, int* out_ok,
                      float* out_scale);
/* n independent (query grid, database grid) pairs in one launch sequence (several queries in flight). */
int gloc_coarse_match_pairs(gloc_coarse* h, const uint32_t* q_grids, const uint32_t* db_grids, size_t n_pairs,
                            const gloc_coarse_params* params, float* out_xy_yaw, float* out_ratio,
                            int* out_ok, float* out_scale);

/* ============================ Scan Context place descriptor ================================= *
 * NO COUNTERPART IN THE REFERENCE, whose descriptors come from trained networks (gloc_vgg_*, gloc_pillar_*): this is
 * the training-free LiDAR place descriptor of Kim & Kim, "Scan Context", IROS 2018, so that scan -> descriptor ->
 * retrieval -> registration runs on what the repository holds.  tests/sc_ref.py restates the contract in numpy.
 *
 * Descriptor [n_rings][n_sectors] fp32: for every finite point, r = hypot(x, y) (dropped when r >= max_radius),
 * ring = min(floor(r / max_radius * n_rings), n_rings - 1), theta = atan2(y, x) in [0, 2 pi),
 * sector = min(floor(theta / 2 pi * n_sectors), n_sectors - 1); a bin holds the maximum of max(z + sensor_height, 0)
 * (one fp32 addition) over its points, 0 when empty.  The same bits on every run and in every batch.
 * Ring key [n_rings]: the fp32 mean of each ring, summed in sector order.  (The paper's sector key, the mean of each
 * column, is not kept: nothing here reads it.)
 *
 * distance(q, c) = min over shift s of 1 - mean over the sectors j where column (j - s) mod n_sectors of q and column j
 * of c both hold a height above 0, of the cosine of the two columns -- np.roll(q, s, axis=1) against c; a shift with
 * fewer than max(min_common_columns, 1) such sectors scores 1.0; the lowest shift wins among equal fp32 distances, so a
 * descriptor without a non-empty column has distance 1.0 at shift 0.  Distances are fp32 in [0, 1], within 1e-5 of the
 * fp64 value; a pair's distance depends on the pair alone (any batch, any run: the same bits).  A query whose yaw in the
 * place's frame is +90 degrees matches at s = n_sectors / 4 (gloc_sc_shift_to_yaw): the seed of the 3-D stage for
 * reverse-direction revisits.  The search is exhaustive over the window, with no ring-key prefilter. */
typedef struct gloc_sc gloc_sc;

typedef struct gloc_sc_params {
  uint32_t n_rings;            /* 20 (1..32) */
  uint32_t n_sectors;          /* 60 (2..64) */
  float max_radius;            /* 80 m, finite and positive */
  float sensor_height;         /* 2.0 m, finite: added to z so that the ground is near 0 */
  uint32_t min_common_columns; /* 1 */
  uint32_t reserved_;
} gloc_sc_params;

int gloc_sc_default_params(gloc_sc_params* p);
/* The parameters are fixed for the handle's life; they are checked before the device is (GLOC_ERR_INVALID). */
int gloc_sc_create(int device, const gloc_sc_params* params, gloc_sc** out);
int gloc_sc_destroy(gloc_sc* h);
int gloc_sc_set_stream(gloc_sc* h, void* hip_stream);
int gloc_sc_synchronize(gloc_sc* h);
/* One host scan (x y z first in every stride_floats floats) -> out_desc [n_rings][n_sectors]; nothing is added. */
int gloc_sc_describe(gloc_sc* h, const float* xyz, size_t n, size_t stride_floats, float* out_desc);
/* n (<= 4096) scans resident in a store on the same device, one launch sequence, the points stay on the device. */
int gloc_sc_describe_store_scans(gloc_sc* h, gloc_scan_store* store, const uint32_t* scan_ids, size_t n,
                                 float* out_desc);
/* Append rows: given descriptors (finite, >= 0: GLOC_ERR_INVALID otherwise), a host scan (row: its index, may be
 * NULL), resident scans (first_row: the index of the first, may be NULL).  Rows are searchable when the call returns. */
int gloc_sc_add(gloc_sc* h, const float* desc, size_t n);
int gloc_sc_add_scan(gloc_sc* h, const float* xyz, size_t n, size_t stride_floats, uint64_t* row);
int gloc_sc_add_store_scans(gloc_sc* h, gloc_scan_store* store, const uint32_t* scan_ids, size_t n,
                            uint64_t* first_row);
int gloc_sc_size(const gloc_sc* h, size_t* n_rows);
int gloc_sc_clear(gloc_sc* h);
int gloc_sc_reserve(gloc_sc* h, size_t n_rows);
int gloc_sc_rows(gloc_sc* h, size_t first, size_t n, float* out_desc);
int gloc_sc_ring_keys(gloc_sc* h, size_t first, size_t n, float* out_keys /* [n][n_rings] */);
/* File: "GLOCSCTX", u32 version = 1, u32 rows, the gloc_sc_params block, rows x n_rings x n_sectors fp32.  load APPENDS;
 * a file written with other parameters than the handle's is refused (GLOC_ERR_INVALID). */
int gloc_sc_save(gloc_sc* h, const char* path);
int gloc_sc_load(gloc_sc* h, const char* path);
/* The k (1..64) nearest rows of [row_begin, row_end) for each of nq descriptors, ascending by (distance, row index);
 * out_shift (may be NULL): the shift of each.  The window is the SLAM-mode exclusion, as in gloc_knn_search: row_end is
 * clamped to the size (SIZE_MAX = all), and where the window holds fewer than k rows the tail is idx = UINT64_MAX,
 * dist = FLT_MAX, shift = 0. */
int gloc_sc_search(gloc_sc* h, const float* q_desc, size_t nq, size_t k, size_t row_begin, size_t row_end,
                   uint64_t* out_idx, float* out_dist, uint32_t* out_shift);
/* The same with the queries taken from resident scans: describe + search without a host round trip of the points. */
int gloc_sc_search_store_scans(gloc_sc* h, gloc_scan_store* store, const uint32_t* q_scan_ids, size_t nq, size_t k,
                               size_t row_begin, size_t row_end, uint64_t* out_idx, float* out_dist,
                               uint32_t* out_shift);
/* One descriptor against the listed rows only (rows may repeat): out_dist / out_shift [n], and, unless NULL,
 * out_by_shift [n][n_sectors]: the distance at every shift.  The test hook of the distance kernel. */
int gloc_sc_distances(gloc_sc* h, const float* q_desc, const uint64_t* rows, size_t n, float* out_dist,
                      uint32_t* out_shift, float* out_by_shift);
/* shift * 2 pi / n_sectors wrapped to (-pi, pi]: the query's yaw in the matched place's frame.  Host only. */
int gloc_sc_shift_to_yaw(const gloc_sc_params* params, uint32_t shift, float* yaw);
int gloc_sc_set_profile(gloc_sc* h, int enable);
/* kernel families: "sc_scatter", "sc_finish", "sc_dist", "sc_select" */
int gloc_sc_profile(gloc_sc* h, const char* kernel, double* total_ms, uint64_t* launches);
int gloc_sc_profile_reset(gloc_sc* h);

/* ============================ M2DP place descriptor ========================================= *
 * NO COUNTERPART IN THE REFERENCE, whose descriptors come from trained networks (gloc_vgg_*, gloc_pillar_*): this is
 * the training-free descriptor of He, Wang & Zhang, "M2DP: a novel 3D point cloud descriptor and its application in
 * loop closure detection", IROS 2016 -- a plain vector of dim = p q + l t floats (192 at the defaults), so that scan ->
 * descriptor -> gloc_knn_* -> registration runs on what the repository holds, at any database size the kNN handles.
 * tests/m2dp_ref.py restates the contract in numpy.
 *
 * M1 points: a point is used iff its three coordinates are finite and (x x + y y) + z z < max_range^2 in un-fused fp32.
 *    Fewer than min_points used points: "no descriptor" -- the zero row, the identity frame with centroid 0, counts 0.
 * M2 frame, fp64 from the fp32 inputs: c = mean; C = sum (p - c)(p - c)^T / n about c (two passes); eigenpairs by the
 *    cyclic Jacobi of the normals, sorted l1 >= l2 >= l3 with ties to the lower column; for a = 1, 2: e_a is negated iff
 *    sum ((p - c) . e_a)^3 < 0; e3 = e1 x e2; R = [e1 e2 e3] as columns.  The frame is R row-major followed by c: 12
 *    doubles.  With this sign rule the frame of a scan turns with the scan.  No floating-point atomics: the summation
 *    tree is fixed, two runs agree bit for bit and a scan in a batch equals the scan alone.
 * M3 signature: y = R^T (p - c); r = max |p - c| over the used points.  Plane a q + b has theta = -pi/2 + a pi / p,
 *    phi = b (pi/2) / q and the in-plane unit pair u = (-sin theta, cos theta, 0), v = (-sin phi cos theta,
 *    -sin phi sin theta, cos phi); alpha = y . u, beta = y . v, rho = hypot(alpha, beta);
 *    ring = min(floor(sqrt(rho / r) l), l - 1), sector = min(floor((atan2(beta, alpha) mod 2 pi) / 2 pi t), t - 1);
 *    rho = 0 gives bin 0, r = 0 puts everything into bin 0.  counts[plane][ring t + sector] is a u32 count.  The device
 *    decides ring and sector by fp64 comparisons against tabulated (k / l)^4 and border directions; a (point, plane) whose
 *    fractional coordinate is within 1e-12 of a border may fall on either side.
 * M4 descriptor: A = counts / n; u1, v1 = its first left and right singular vectors, both negated iff sum u1 < 0
 *    (A >= 0: the first pair can be taken non-negative); the descriptor is fp32([u1, v1]).  fp64 power iteration on
 *    A A^T, run until the vector moves by less than 2^-46 (at most 20 000 steps: sigma2 / sigma1 up to ~0.9996).
 * M5 seed (host): R_db R_q^T and t = c_db - R_db R_q^T c_q as a row-major fp32 4 x 4, query -> place.  The rotation is
 *    the rotation between the two scans at any yaw; the centroid of a ring scan sits at the sensor, so the translation
 *    carries little. */
typedef struct gloc_m2dp gloc_m2dp;

typedef struct gloc_m2dp_params {
  uint32_t n_azimuth;   /* p: 4  (>= 1, p q <= 64) */
  uint32_t n_elevation; /* q: 16 (>= 1, p q <= 64) */
  uint32_t n_rings;     /* l: 8  (>= 1, l t <= 128) */
  uint32_t n_sectors;   /* t: 16 (>= 2, l t <= 128) */
  float max_range;      /* 80 m, finite and positive */
  uint32_t min_points;  /* 16 (>= 4) */
  uint32_t reserved_;   /* must be 0 */
} gloc_m2dp_params;

int gloc_m2dp_default_params(gloc_m2dp_params* p);
/* dim = p q + l t of a valid block.  Host only. */
int gloc_m2dp_dim(const gloc_m2dp_params* params, size_t* dim);
/* The parameters are fixed for the handle's life; they are checked before the device is (GLOC_ERR_INVALID). */
int gloc_m2dp_create(int device, const gloc_m2dp_params* params, gloc_m2dp** out);
int gloc_m2dp_destroy(gloc_m2dp* h);
int gloc_m2dp_set_stream(gloc_m2dp* h, void* hip_stream);
int gloc_m2dp_synchronize(gloc_m2dp* h);
/* One host scan (x y z first in every stride_floats floats) -> out_desc [dim], out_frame12 [12] and out_counts
 * [p q][l t] (the test hook of M3); the last two may be NULL. */
int gloc_m2dp_describe(gloc_m2dp* h, const float* xyz, size_t n, size_t stride_floats, float* out_desc,
                       double* out_frame12, uint32_t* out_counts);
/* n (<= 4096) scans resident in a store on the same device: one launch sequence whose launch count does not depend on n,
 * the points stay on the device.  The original-order points are read: nothing depends on a target index. */
int gloc_m2dp_describe_store_scans(gloc_m2dp* h, gloc_scan_store* store, const uint32_t* scan_ids, size_t n,
                                   float* out_desc, double* out_frame12, uint32_t* out_counts);
/* The same with the rows left in device memory (d_out_desc [n][dim]), enqueued on the handle's stream: ready for
 * gloc_knn_add_device / gloc_knn_search_device on that stream without a host round trip. */
int gloc_m2dp_describe_store_scans_device(gloc_m2dp* h, gloc_scan_store* store, const uint32_t* scan_ids, size_t n,
                                          float* d_out_desc);
/* M4 alone on given counts [n_sig][p q][l t] with n_points [n_sig]: out_desc [n_sig][dim] and, unless NULL, out_sigma2
 * [n_sig][2] = sigma1, sigma2 of counts / n_points.  The test hook of the SVD kernel. */
int gloc_m2dp_signature_svd(gloc_m2dp* h, const uint32_t* counts, const uint32_t* n_points, size_t n_sig,
                            float* out_desc, double* out_sigma2);
/* M5.  Host only. */
int gloc_m2dp_frame_to_seed(const double* frame_q, const double* frame_db, float* T16);
int gloc_m2dp_set_profile(gloc_m2dp* h, int enable);
/* kernel families: "m2dp_frame", "m2dp_project", "m2dp_svd" */
int gloc_m2dp_profile(gloc_m2dp* h, const char* kernel, double* total_ms, uint64_t* launches);
int gloc_m2dp_profile_reset(gloc_m2dp* h);

/* ============================ ground pre-alignment ("next" row N3) ========================= *
 * Replaces GroundEstimator::EsitmateGroundAndTransform (registration/ground_estimator.cpp:196-228),
 * the optional 4th-argument mode of global_localization (registration/global_localization.cpp:431-436,
 * 495-499): points within 20 m -> a normal per point from its 10 nearest neighbours -> the fullest
 * 10-degree elevation bin outside 5..12 is the ground -> plane RANSAC (0.1 m) -> T_l2g (roll, pitch and
 * height; yaw removed).  The reference leaves the numerics to PCL and Eigen; the exact arithmetic of
 * this implementation is stated step by step in oracle/ground_oracle.c (parity unpinned). */
typedef struct gloc_ground gloc_ground;

typedef struct gloc_ground_params {
  float near_range2;     /* 400 = (20 m)^2: ground_estimator.cpp:203 */
  uint32_t knn;          /* 10: ground_estimator.cpp:79 (3..16) */
  float plane_thresh;    /* 0.1 m: ground_estimator.cpp:27 */
  uint32_t ransac_iters; /* 1000: pcl::SampleConsensus max_iterations_ default */
  float ransac_conf;     /* 0.99: pcl::SampleConsensus probability_ default; <= 0 or >= 1: no early stop */
  uint32_t reserved_;
  uint64_t seed;
} gloc_ground_params;

typedef struct gloc_ground_info {
  uint32_t n_near;      /* points within the range filter */
  uint32_t hist[18];    /* elevation bins of the normals, 0 = pointing down .. 17 = pointing up */
  int32_t ground_bin;   /* -1: none */
  uint32_t n_ground;
  uint32_t best_hyp, inliers, iters_used;
  float plane[4];       /* a x + b y + c z + d = 0 with unit normal, as fitted */
  int32_t found;        /* 0: no ground, T = identity (ground_estimator.cpp:218-220) */
} gloc_ground_info;

int gloc_ground_default_params(gloc_ground_params* p);
int gloc_ground_create(int device, gloc_ground** out);
int gloc_ground_destroy(gloc_ground* h);
int gloc_ground_set_stream(gloc_ground* h, void* hip_stream);
enum { GLOC_GROUND_OPT_KNN_EXHAUSTIVE = 1 /* 1: every pair instead of the chunk-culled search; same lists */ };
int gloc_ground_set_option(gloc_ground* h, int option, int64_t value);
/* T16: T_l2g, row-major 4x4 f32 (host).  out_xyz (may be NULL): the cloud transformed by T_l2g, same
 * layout as the input (extra channels copied) -- cloud_out of the reference. */
int gloc_ground_estimate(gloc_ground* h, const float* xyz, size_t n, size_t stride_floats,
                         const gloc_ground_params* p, float* T16, gloc_ground_info* info, float* out_xyz);
int gloc_ground_estimate_device(gloc_ground* h, const float* d_xyz, size_t n, size_t stride_floats,
                                const gloc_ground_params* p, float* T16, gloc_ground_info* info,
                                float* d_out_xyz);
/* Building blocks, exposed for tests (host buffers, packed xyz): the exact k nearest neighbours of every
 * point within the cloud itself ([n][k], ascending (d2, index), the point itself first); the normals
 * and their elevation bins. */
int gloc_ground_knn(gloc_ground* h, const float* xyz, size_t n, uint32_t k, uint32_t* out_idx, float* out_d2);
int gloc_ground_normals(gloc_ground* h, const float* xyz, size_t n, uint32_t k, float* out_normals,
                        uint8_t* out_bins);
/* T_l2g from plane coefficients (TransformPointsToGround, ground_estimator.cpp:163-194); host only. */
int gloc_ground_transform_from_plane(const float* plane4, float* T16);
int gloc_ground_set_profile(gloc_ground* h, int enable);
/* kernel families: "ground_knn", "ground_normals", "ground_plane", "ground_transform" */
int gloc_ground_profile(gloc_ground* h, const char* kernel, double* total_ms, uint64_t* launches);

/* ============================ synthetic inputs (bench / tests) ============================ *
 * On-device twin of gloc3d_amd/synth.py for databases too large to upload (SURVEY.md 8d cfg E).
 * kind 0: iid N(0,1)/sqrt(dim); kind 1: anchored trajectory (stride 16, noise 0.05).
 * Appends n rows of the global synthetic database to the handle: global rows first_row,
 * first_row + row_stride, ... (row_stride = G gives rank first_row's interleaved shard). */
int gloc_knn_add_synthetic(gloc_knn* h, int kind, uint64_t seed, uint64_t first_row, size_t n,
                           uint64_t row_stride);
int gloc_synth_fill_device(int device, void* hip_stream, int kind, uint64_t seed,
                           uint64_t first_row, size_t n, size_t dim, uint64_t row_stride,
                           float* d_out);
/* A new resident scan made on the device from scan `base_id`: point i = T p_i + sigma * gauss(seed, i)
 * per coordinate (T16 row-major 4x4 or NULL = identity; gloc3d_amd/synth.py::scan_variant gives the
 * same bits).  Fills a KITTI-00-sized store (4541 distinct scans) in seconds. */
int gloc_scan_store_add_variant(gloc_scan_store* st, uint32_t base_id, const float* T16,
                                float noise_sigma, uint64_t seed, uint32_t* scan_id);

/* `count` new resident scans RAY-CAST on the device (bench / tests; round 6): a spinning lidar of n_beams x n_az rays
 * (elevations linspace(fov_lo_deg, fov_hi_deg, n_beams), azimuths [0, 2 pi) -- ray r = beam * n_az + az) at the sensor
 * pose T16[i] (world <- sensor, row-major 4x4 DOUBLES) over a world of axis-aligned boxes [box_lo, box_hi] (doubles,
 * [n][3]; scan i sees boxes box_first[i] .. box_first[i + 1] - 1 of the arrays -- the caller passes the boxes within
 * reach of each pose) and a ground plane z = ground_z; a ray returns at the nearest hit below max_range (a box face
 * nearer than 0.5 m is ignored), its range gets noise_sigma * gauss(seeds[i], r), the point is kept in the SENSOR frame,
 * returns stay in ray order.  The twin of gloc3d_amd/synth.py::lidar_scan (fp64 throughout, one rounding to fp32): equal
 * to it to ~1e-6 m.  This is how bench.py makes SURVEY.md 8d cfg D's "4541-pose loop trajectory through one procedural
 * world" -- 4541 DISTINCT casts, the KITTI .bin point layout of registration/global_localization.cpp:160-182 minus the
 * intensity -- in seconds instead of rigid copies of a few host-cast views. */
typedef struct gloc_raycast_params {
  uint32_t n_beams, n_az;          /* 64 x 2000 (HDL-64E-like) */
  double max_range, noise_sigma;   /* 80 m, 0.02 m */
  double fov_lo_deg, fov_hi_deg;   /* -24.8, 2.0 */
} gloc_raycast_params;
int gloc_scan_store_add_raycast_batch(gloc_scan_store* st, size_t count, const double* box_lo, const double* box_hi,
                                      const uint32_t* box_first /* [count + 1] */, double ground_z,
                                      const double* T16 /* [count][16] */, const uint64_t* seeds /* [count] */,
                                      const gloc_raycast_params* params, uint32_t* scan_ids /* [count] */);

/* ---- pose-graph optimisation --------------------------------------------------------------------------- *
 * What turns the edges the entries above produce into corrected poses: gloc_reg_<m>_pairs gives an edge's Z, and
 * gloc_reg_evaluate_pairs its information matrix.  Levenberg-Marquardt over all node poses, block-Jacobi preconditioned
 * conjugate gradients inside, everything fp64 on the device.  The executable contract is tests/pgo_ref.py.
 *
 *   G1. Node k has pose T_k = (R_k, t_k), node frame -> map frame, [n][16] row-major DOUBLES on both sides of the ABI (a
 *       map is kilometres wide; the fp32 T16 of the per-pair entries would cap convergence at fp32 rounding).  Edge e is
 *       (i = edge_src[e], j = edge_tgt[e], Z, Omega): Z [16] fp32 maps source -> target, Z ~ T_j^-1 T_i -- exactly an
 *       out_T row of gloc_reg_<m>_pairs --, and Omega [36] is an out_info36 row of gloc_reg_evaluate_pairs, read from
 *       its UPPER triangle: the Hessian for Z <- exp(xi) Z, xi = (w, v), rotation first, (exp(w) R, exp(w) t + v).
 *   G2. The residual is the left perturbation that takes Z to the predicted relative pose, so Omega weights it as it is:
 *         R_E = R_j^T R_i R_Z^T,  t_E = R_j^T (t_i - t_j) - R_E t_Z,  r = (log R_E, t_E),  s2 = r^T Omega r.
 *       log R: v = vee(R - R^T) / 2, th = atan2(|v|, (tr R - 1) / 2), w = v th / |v| (v (1 + |v|^2 / 6) below |v| = 1e-8):
 *       residual rotations up to ~3 rad are exact to rounding, pi itself is not handled.
 *   G3. Nodes are perturbed the same way, T_k <- (exp(w_k) R_k, exp(w_k) t_k + v_k); to first order
 *       r(delta) = r + A (delta_i - delta_j) with ONE 6 x 6 Jacobian per edge,
 *         A = [ Jl^-1(w) R_j^T                      0     ]     Jl^-1(w) = I - [w]x / 2 + c [w]x^2,
 *             [ [R_E t_Z]x R_j^T - R_j^T [t_i]x     R_j^T ]     c = 1 / th^2 - (1 + cos th) / (2 th sin th), 1/12 below 1e-6
 *       (checked against central differences in tests/test_pgo_ref_cpu.py).  Per edge, with the robust weight w_e:
 *       W_e = w_e A^T Omega A, b_e = w_e A^T Omega r;  g_k = sum +- b_e, H_kk = sum W_e, (H x)_k = sum +- W_e (x_i - x_j),
 *       + where k is the edge's source, - where it is the target, over the edges at k in ascending edge index.
 *   G4. Translations are taken relative to the first fixed node's translation (subtracted in fp64 on input, added back on
 *       output): the lever arm [t_i]x has the size of the map, not of the distance to an arbitrary origin.  g and H_kk as
 *       gloc_pgo_linearize returns them refer to that origin.
 *   G5. Robust weighting: `robust` NULL or kind NONE is the plain sum of squares.  Otherwise w_e is gloc_robust_weight of
 *       s2 at `scale` (dimensionless, as for generalized ICP) for the edges robust_mask selects (NULL: all; odometry
 *       edges usually keep weight 1) and 1 for the others.  A schedule (scale_start != 0) is refused: the step control
 *       needs one objective.  That objective is F = sum rho_e: rho = s2 for an unweighted edge and otherwise, t = s2 / c^2,
 *         HUBER  t <= 1 ? s2 : c^2 (2 sqrt t - 1)     CAUCHY  c^2 log(1 + t)
 *         TUKEY  t <= 1 ? (c^2 / 3)(1 - (1 - t)^3) : c^2 / 3     GEMAN_MCCLURE  s2 / (1 + t).
 *   G6. A node is FREE if it is not fixed and has an edge.  Every other node gets no update and its pose is returned bit
 *       for bit.  D = blockdiag(H_kk) over the free nodes; a step solves (H + lambda D) delta = -g (Marquardt scaling: the
 *       damping does not depend on where the origin lies).  lambda starts at lambda_init; gain = (F - F_new) /
 *       (delta^T (lambda D delta - g)); the step is accepted iff gain > 0 and F_new is finite; then lambda <- lambda
 *       max(1/3, 1 - (2 gain - 1)^3), nu = 2 (Nielsen); otherwise lambda <- lambda nu, nu <- 2 nu.
 *   G7. The solve: preconditioned conjugate gradients from x = 0 with M = ((1 + lambda) H_kk)^-1 from the 6 x 6 Cholesky
 *       and pivot rule of the Gauss-Newton refinements (the factor of H_kk, scaled: the pivot rule does not see the
 *       factor 1 + lambda), until |residual|^2 <= pcg_tol^2 |g|^2 or pcg_max_iters.  A free node whose block fails the
 *       pivot rule ends the call with status 2 and the poses of the last accepted step.  Two limits follow from this
 *       choice of solver, both measured.  A node perturbed about the origin couples its rotation
 *       to its translation through the lever arm |t|: H_kk's smallest pivot is about (Omega_rot / (|t|^2 Omega_trans))^2 of
 *       its largest, so the 1e-12 rule refuses maps wider than about 1000 sqrt(Omega_rot / Omega_trans) metres from the
 *       first fixed node -- 20 km for the information matrices of gloc_reg_evaluate_pairs (Omega_rot / Omega_trans is the
 *       mean squared point range, some 400 m^2), a few km for edges with weak rotations.  And block-Jacobi PCG needs
 *       thousands of iterations per step on a loop of thousands of nodes: at the default cap every solve is cut short
 *       (an inexact step, still a descent step) and max_iters is reached before the minimum; raise pcg_max_iters there.
 *   G8. Stops, tested after an accepted step: max |w_k| <= rot_eps and max |v_k| <= trans_eps (both set): status 1;
 *       max |g| <= grad_eps (set; also tested before the first step): status 3; max_iters attempts: status 0; no free
 *       node: status 2 with zero iterations.  An eps of 0 switches its test off.
 *   G9. Deterministic: no floating-point atomics, every sum in a fixed order (a node's edges in ascending index spread
 *       over the 64 lanes of a wave, per-work-group partials in index order); two calls on the same input give the same bits.
 *
 * The checks come in this order, each refusing with GLOC_ERR_INVALID, before any device work and with the outputs
 * untouched: a null prm; max_iters = 0; pcg_max_iters = 0; lambda_init, pcg_tol not finite and positive; rot_eps,
 * trans_eps, grad_eps not finite or negative; reserved_ != 0; a robust block the robust entries refuse, or one with a
 * schedule; a null array (robust_mask may be); n outside [2, 2^20]; m outside [1, 2^22]; an edge end >= n; an edge from
 * a node to itself; no fixed node; a non-finite value in poses, Z or info; a null handle.  Duplicate edges, edges in both
 * directions and components without a fixed node are legal (the damping keeps such a component solvable).  Calls are
 * synchronous. */
typedef struct gloc_pgo gloc_pgo;
typedef struct gloc_pgo_params {
  uint32_t max_iters;      /* 50: Levenberg-Marquardt attempts */
  uint32_t pcg_max_iters;  /* 200 per attempt */
  double lambda_init;      /* 1e-4 (Ceres' initial trust radius inverted) */
  double pcg_tol;          /* 1e-8, relative to |g| */
  double rot_eps;          /* 1e-6 rad; 0: no step test */
  double trans_eps;        /* 1e-6 m; 0: no step test */
  double grad_eps;         /* 1e-6; 0: no gradient test */
  uint32_t reserved_[2];   /* 0 */
} gloc_pgo_params;         /* 56 bytes */
typedef struct gloc_pgo_result {
  uint32_t iters, accepted, pcg_iters;
  int32_t status;          /* G8 */
  double cost_initial, cost_final, lambda, grad_inf;
} gloc_pgo_result;         /* 48 bytes */

void gloc_pgo_default_params(gloc_pgo_params* p);
int gloc_pgo_create(int device, gloc_pgo** out);
int gloc_pgo_destroy(gloc_pgo* h);
int gloc_pgo_set_stream(gloc_pgo* h, void* hip_stream);
int gloc_pgo_synchronize(gloc_pgo* h);
/* families: pgo_setup, pgo_linearize, pgo_gather, pgo_pcg, pgo_step; pgo_consistency (gloc_pgo_consistency, below) */
int gloc_pgo_set_profile(gloc_pgo* h, int enable);
int gloc_pgo_profile(gloc_pgo* h, const char* kernel, double* total_ms, uint64_t* launches);
int gloc_pgo_profile_reset(gloc_pgo* h);

/* One linearisation at the given poses (G2-G5).  Any output may be NULL, but not all of them. */
int gloc_pgo_linearize(gloc_pgo* h, const double* poses /* [n][16] */, const uint8_t* fixed /* [n] */, size_t n,
                       const uint32_t* edge_src, const uint32_t* edge_tgt /* [m] */, const float* Z /* [m][16] */,
                       const double* info /* [m][36] */, const uint8_t* robust_mask /* [m], may be NULL */, size_t m,
                       const gloc_pgo_params* prm, const gloc_robust_params* robust /* NULL: plain */,
                       double* out_r6 /* [m][6] */, double* out_s2 /* [m] */, double* out_weight /* [m] */,
                       double* out_g6 /* [n][6] */, double* out_Hdiag36 /* [n][36] symmetric */, double* out_cost);

/* G6-G8.  out_s2 and out_weight (at the returned poses) may be NULL. */
int gloc_pgo_optimize(gloc_pgo* h, const double* poses, const uint8_t* fixed, size_t n, const uint32_t* edge_src,
                      const uint32_t* edge_tgt, const float* Z, const double* info, const uint8_t* robust_mask, size_t m,
                      const gloc_pgo_params* prm, const gloc_robust_params* robust, double* out_poses /* [n][16] */,
                      double* out_s2, double* out_weight, gloc_pgo_result* out);

/* ---- mutually consistent loop closures (pairwise consistency maximisation) -------------------------------- *
 * What stands between the closures and the optimiser: the robust kernel of gloc_pgo_optimize rejects a closure only
 * after it has bent the solution and cannot reject a group of wrong closures that agree with each other.  Two closures are
 * CONSISTENT when the cycle through both of them and the trajectory between their ends closes within its covariance; the
 * largest mutually consistent set found by a greedy clique search is kept (after Mangelson et al., ICRA 2018; parity with
 * their code is not claimed).  A stage of the gloc_pgo handle -- its stream, grow-only buffers and profile (family
 * pgo_consistency; its parts also as pgo_consistency_pairs, _score, _clique) --, fp64 throughout, no atomics.  The
 * executable contract is tests/pcm_ref.py.
 *
 * Inputs: poses [n][16] doubles, the current estimates (G1); L candidate closures src, tgt, Z [L][16] fp32, info [L][36]
 * fp64 read from the upper triangle (G1's edges); path [n] doubles or NULL (all zeros), a coordinate along the trajectory
 * in the caller's units (steps, metres travelled).
 *
 *   C1. Translations are taken relative to node 0's translation (fp64, on input).  Per closure a: Sigma_a = Omega_a^-1 by
 *       the 6 x 6 Cholesky and pivot rule of G7 -- column b the solve of the unit vector e_b, its rows a <= b kept and
 *       mirrored --, and B_a = (T_ja Z_a) T_ia^-1, the pose the closure predicts for the map seen from its source.  A closure
 *       whose Omega fails the pivot rule has status 1 and is consistent with nothing.
 *   C2. Pair statistic for a < b, with i = src, j = tgt:  X = T_ja^-1 T_jb;  r = G2's residual evaluated with
 *       T_i := B_b T_ia, T_j := T_ja, Z := Z_a (the same log and series branch), which is (log R_E, t_E) of
 *       E = X Z_b (T_ib^-1 T_ia) Z_a^-1;  Ad_X = [[R_X, 0], [[t_X]x R_X, R_X]], the first-order transport of the left
 *       perturbation (w, v);  d = |path_ia - path_ib| + |path_ja - path_jb|;
 *         M = Sigma_a + Ad_X Sigma_b Ad_X^T + diag(drift_rot^2 d (1,1,1), drift_trans^2 d (1,1,1)),  read from its upper triangle;
 *         s2_ab = r^T M^-1 r = |L^-1 r|^2 with M = L L^T by the same Cholesky.
 *       The drift term is isotropic and ignores the lever arm of rotation drift: a stated limit of the model.
 *   C3. C_ab = C_ba = 1 iff both closures have status 0, M passed the pivot rule, s2_min(a,b),max(a,b) is finite and
 *       s2 < chi2.  C_aa = 0.  Only the a < b form is ever evaluated (far from consistency the two directions differ
 *       freely), so the matrix is symmetric by definition.  out_s2 holds +inf wherever one of the conditions before the
 *       last fails, and on the diagonal: out_s2 < chi2 IS the matrix.
 *   C4. degree_a = sum_b C_ab;  S_ab = C_ab |{k : C_ak and C_bk}|,  score_a = sum_b S_ab (unsigned 64-bit; the
 *       correspondence graph's G2);  key_a = score_a + degree_a (an isolated consistent pair has score 0 but outranks an
 *       isolated closure).  The seeds are the n_seeds closures of largest key, ties to the smaller position; ranks past L
 *       hold 0xFFFFFFFF and a clique size of 0.
 *   C5. Per seed s: K = {s}, cand = row_s; while cand is not empty: v = the member of cand maximising
 *       popcount(row_v & cand), ties to the smaller position; K <- K + {v}; cand <- cand & row_v.  Integers only.
 *   C6. The winner is the largest clique, ties to the smaller seed rank; out_mask marks its members, out_clique_size and
 *       out_winner_rank describe it.  With fewer than min_clique members the mask is all zero and out_ok = 0.
 *
 * The checks come in this order, each refusing with GLOC_ERR_INVALID, before any device work and with the outputs
 * untouched: a null prm; chi2 not finite and positive; drift_rot, drift_trans not finite or negative; n_seeds outside
 * [1, 1024]; reserved_ != 0; a null array (path may be) or every output null; n outside [2, 2^20]; L outside
 * [1, 16384]; out_s2 given with L > 4096; a closure end >= n; a closure from a node to itself; a non-finite value in
 * poses, Z, info or path; a null handle.  Duplicate closures are legal (and consistent with each other).  Calls are
 * synchronous and deterministic: no floating-point sum crosses a lane.
 *
 * Use: select, then optimise; then select again on the corrected poses with a smaller drift to re-admit closures the
 * drifted start hid.  The defaults are conventions, not tuned. */
typedef struct gloc_pgo_consistency_params {
  double chi2;            /* 16.8119: the 99 % quantile of chi-squared with 6 degrees of freedom */
  double drift_rot;       /* 0: rad per square root of a unit of path */
  double drift_trans;     /* 0: m per square root of a unit of path */
  uint32_t n_seeds;       /* 64, 1 .. 1024 */
  uint32_t min_clique;    /* 2 */
  uint32_t reserved_[2];  /* 0 */
} gloc_pgo_consistency_params;   /* 40 bytes */

void gloc_pgo_consistency_default_params(gloc_pgo_consistency_params* p);

/* C1-C6.  Any output may be NULL, but not all of them.  out_s2 is a diagnostic of L^2 doubles. */
int gloc_pgo_consistency(gloc_pgo* h, const double* poses /* [n][16] */, size_t n, const uint32_t* src, const uint32_t* tgt /* [L] */,
                         const float* Z /* [L][16] */, const double* info /* [L][36] */, const double* path /* [n] or NULL */, size_t L,
                         const gloc_pgo_consistency_params* prm, uint8_t* out_mask /* [L] */, uint32_t* out_clique_size,
                         uint32_t* out_winner_rank, uint32_t* out_ok, uint8_t* out_status /* [L] */, uint32_t* out_degree /* [L] */,
                         uint64_t* out_score /* [L] */, uint32_t* out_seeds /* [n_seeds] */, uint32_t* out_clique_sizes /* [n_seeds] */,
                         double* out_s2 /* [L][L] */);

#ifdef __cplusplus
}
#endif
#endif /* GLOC3D_H */
