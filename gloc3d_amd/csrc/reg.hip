// reg.hip -- C ABI of the batched candidate registration (include/gloc3d.h) over reg_kernels.hpp.
// Replaces icp_match_3d (registration/global_registration.cpp:237-248) and the per-candidate RANSAC
// transform estimate (registration/loop_detector.cpp:256-257) of the reference, batched over the
// top-k candidates of GlocEvaluator::global_registraion (registration/global_localization.cpp:511-574)
// and over any number of queries in flight (one launch covers all their candidates).
#include <algorithm>
#include <cmath>
#include <vector>

#include "common.hpp"

#include "eval.hpp"
#include "fgr.hpp"
#include "fpfh.hpp"
#include "ndt.hpp"
#include "nn_compact.hpp"
#include "gicp.hpp"
#include "p2l.hpp"
#include "pairgraph.hpp"
#include "reg_kernels.hpp"
#include "robust.hpp"
#include "scan_store.hpp"
#include "vgicp.hpp"
#include "vmap.hpp"

using namespace gloc;
using namespace gloc::reg;

struct gloc_reg : Handle {
  hipEvent_t done_ev = nullptr;  // a batch waits for ITS OWN results, not for the stream: handles that share a stream
                                 // (gloc_reg_set_stream) queue their batches back to back while the host reads results
  gloc_scan_store* store = nullptr;  // scans are looked up here (attached, or the handle's own)
  gloc_scan_store* own_store = nullptr;
  DevBuf jobs, states;           // Job[], CandState[]
  DevBuf corr, d2, pairs;        // [job][ld]
  DevBuf Rt, valid;              // RANSAC hypotheses; valid: [job][hyp] valid, [job][hyp] inliers behind it (one fill clears both)
  DevBuf alive;                  // all-hypotheses RANSAC: [job][H] list of the hypotheses still in the race + [job] counts
  DevBuf partials;               // [job][n_part][ACC_NV] fp64
  DevBuf export_idx, export_d2;  // gloc_reg_nn: results in the caller's index space
  DevBuf counters;               // pairs evaluated by the culled search: NN_STAT_SLOTS partial counts (profiling only)
  // pinned host staging: job table up, per-job state up and down.  Pageable memory would make the "async" copies
  // wait for the stream, i.e. for the batch BEFORE this one when handles share a stream
  void* pin = nullptr;
  size_t pin_cap = 0;
  CandState* h_states = nullptr;  // [n_jobs], inside pin; a profiled batch's stamps behind them (up and down with the states)
  Job* h_jobs = nullptr;          // [n_jobs], inside pin
  // a batch between gloc_reg_batch_multi_begin and _end
  struct Pending {
    bool active = false;
    std::vector<size_t> slot;     // job -> output row
    std::vector<size_t> n_src;    // per job
    std::vector<float> def_T;     // output rows before the jobs' results go in (initial guess / identity)
    size_t total = 0;
    float max_rmse = 0.f, max_final_step = 0.f;
    bool icp = false;
    gloc_scan_store* store = nullptr;  // the store whose scans this batch pins ...
    std::vector<uint32_t> pinned;      // ... and their ids (store_pin)
  } pending;
  std::vector<float> last_final_step;  // per job of the last collected batch (gloc_reg_final_steps)
  int nn_mode = 0;        // 0 culled + compacted (default), 1 exhaustive
  int nn_src_per_lane = 2;  // culled kernel: source points per lane (1, 2, 4)
  int nn_job_group = 24;    // culled kernel: jobs interleaved in the launch order (a multiple of 8: see nn_compact.hpp)
  bool nn_job_group_set = false;  // by the caller (else a small batch takes its own: launch_order)
  int nn_sub_jobs = 0;      // culled kernel: interleaved shares of a job's work-groups that get their own slot (0: by batch size)
  bool temp_target_index = false;  // kd-ordered target index for the temporary scans of the host-buffer calls
  // heavy source groups over several waves (nn_compact.hpp, NnSplit): helper waves per job (-1: by batch size, 0: off)
  // and the work estimate (cycles) above which a group is split
  int nn_split_helpers = -1;
  uint32_t nn_split_thresh = 60000;
  bool nn_split_thresh_set = false;  // by the caller (GLOC_REG_OPT_NN_SPLIT_THRESH): else 60000, or 85000 where the passes are chained
  DevBuf split_zero, split_ff;     // [work | plan | ticket] and [skey | helper] of the batch
  NnSplit split{};                 // views into them for the batch being enqueued (hx = 0: off)
  // the groups a cold pass's waves give up and a second launch searches with NN_HEAVY_PARTS waves each (NnHeavy)
  int nn_heavy_thresh = 32;        // processed chunks at which a cold wave gives up (0: off)
  DevBuf heavy_buf;                // [count | list | ticket | skey | hkey]
  size_t heavy_cap = 0;            // entries the buffer holds (its ticket / skey parts are self-resetting)
  NnHeavy heavy{};                 // the view for the batch being enqueued (cap = 0: off)
  std::atomic<uint64_t> nn_launches{0};
  // the warm passes of a small batch chained in one launch (NnChain): 1 on (default), 0 off; stopped for good on a handle
  // whose chain once ran out of time
  int nn_chain = 1;
  bool chain_broken = false;
  bool chain_stall = false;       // test aid (gloc_reg_debug_chain_stall): the solvers wait for one wave more than there is
  DevBuf chain_buf;               // [ready | done | sdone | err] then the reducers' sub-sums
  uint32_t* h_chain_err = nullptr; // pinned: the batch's err word, copied behind the states
  bool chain_in_batch = false;    // the batch enqueued last ran a chained launch
  // ... and what it takes to run that batch again launch by launch should the chain's waits run out (collect_jobs):
  // the jobs as enqueue_jobs saw them (JobHost, kept as bytes: the type is this file's) with their initial poses, the parameters
  std::vector<unsigned char> retry_jobs;
  std::vector<float> retry_T;
  gloc_reg_params retry_prm{};
  std::atomic<uint64_t> chain_launches{0}, chain_timeouts{0};
  size_t last_ld = 0;      // shape of the last batch (gloc_reg_debug_corr)
  uint32_t last_jobs = 0;
  gloc::ndt::Ws* ndt = nullptr;  // NDT workspace (ndt.hip), made on first use
  gloc::p2l::Ws* p2l = nullptr;  // point-to-plane / generalized ICP workspace (gn6.hpp), made on first use
  gloc::vgicp::Ws* vgicp = nullptr;  // voxelized generalized ICP's voxel maps (vgicp.hip), made on first use
  gloc::vmap::Set* vmaps = nullptr;  // the resident voxel maps this handle owns (vmap.hip): they go with it
  gloc::fpfh::Ws* fpfh = nullptr;    // the feature matcher's keys and tables (fpfh.hip), made on first use
  gloc::pairgraph::Ws* pgraph = nullptr;  // the correspondence graph's bit matrices and seed rows (pairgraph.hip), made on first use
  size_t pgraph_budget = 0;          // bytes of them in flight at a time (GLOC_REG_OPT_PAIRGRAPH_BUDGET; 0: pairgraph::BUDGET_BYTES)
  gloc::fgr::Ws* fgr = nullptr;      // Fast Global Registration's pass bits, multiplicities and results (fgr.hip), made on first use
  ~gloc_reg() {  // (the handle's work has been waited for: destroy_handle)
    if (pending.active && pending.store) store_pin(pending.store, pending.pinned.data(), pending.pinned.size(), -1);
    if (store) store->attached--;
    if (own_store) (void)gloc_scan_store_destroy(own_store);
    gloc::ndt::ws_free(ndt);
    gloc::p2l::ws_free(p2l);
    gloc::vgicp::ws_free(vgicp);
    gloc::vmap::set_free(vmaps);
    gloc::fpfh::ws_free(fpfh);
    gloc::pairgraph::ws_free(pgraph);
    gloc::fgr::ws_free(fgr);
    if (done_ev) (void)hipEventDestroy(done_ev);
    if (pin) (void)hipHostFree(pin);
  }
};

namespace {

struct JobHost {
  DevScan src, tgt;
  uint32_t stream_id;
  const float* init_T;  // 16 floats or null
};

const float I16[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};

void init_state(CandState& st, const float* T16, uint32_t ransac_iters = 0) {
  memset(&st, 0, sizeof(st));
  const float* T = T16 ? T16 : I16;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) {
      st.Tf[3 * i + j] = T[4 * i + j];
      st.Td[3 * i + j] = (double)T[4 * i + j];
    }
    st.Tf[9 + i] = T[4 * i + 3];
    st.Td[9 + i] = (double)T[4 * i + 3];
  }
  st.best_h = 0xFFFFFFFFu;
  st.niters = ransac_iters;
  st.last_step = 0.f;
}

// The fp32 pose of a job's state as a row-major 4 x 4.
void pose_to_T16(const CandState& st, float* T) {
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) T[4 * i + j] = st.Tf[3 * i + j];
    T[4 * i + 3] = st.Tf[9 + i];
  }
  T[12] = 0.f; T[13] = 0.f; T[14] = 0.f; T[15] = 1.f;
}

// A pair list on the host in the layout the RANSAC kernels read ([ld] x f32x4[2], zero behind the n-th pair):
// (P[i], Q[i]), or with `corr` (P[i], Q[corr[i]]).
std::vector<float> pack_pairs(const float* P, const float* Q, const uint32_t* corr, size_t n, size_t ld) {
  std::vector<float> hp(ld * 8, 0.f);
  for (size_t i = 0; i < n; ++i)
    for (int a = 0; a < 3; ++a) {
      hp[i * 8 + a] = P[3 * i + a];
      hp[i * 8 + 4 + a] = Q[3 * (corr ? (size_t)corr[i] : i) + a];
    }
  return hp;
}

// What a job on a list of M pairs found: a winner at all, and -- ok -- one with the inliers the stage itself asks for:
// max(3, ceil(min_inlier_ratio M)), the product in fp64.
void pair_verdict(const CandState& cs, uint32_t M, float min_inlier_ratio, bool* found, bool* ok) {
  *found = cs.best_h != 0xFFFFFFFFu && M >= 3;
  const double need = std::max(3.0, std::ceil((double)min_inlier_ratio * (double)M));
  *ok = *found && (double)cs.best_inl >= need;
}

// Source groups (a wave's worth of sources at `cs` per lane) of a scan of n points.
uint32_t src_groups(size_t n, int cs) { return (uint32_t)((n + 64 * cs - 1) / (64 * cs)); }

struct BatchDims {
  uint32_t n_jobs, max_src, max_groups, n_part;
  size_t ld;
};

// A batch as the launches see it: the stream and the handle's workspaces.
struct WsView {
  hipStream_t s;
  uint32_t n_jobs;
  Job* jobs;
  CandState* states;
  uint32_t* corr;
  float* d2;
  f32x4* pairs;
  float* Rt;
  uint32_t *valid, *inliers;
  double* partials;
  uint32_t *a_idx, *a_cnt;  // (ransac_alive_kernel's lists; set when they are allocated)
  NnSplit split;
  NnHeavy heavy;
};

// Helper wave slots per job of the split plan (NnSplit) for a batch; 0: no plan.  One query alone (20 jobs) is the case
// that needs it: its launch is as long as its longest wave.  A launch of hundreds of jobs only loses its tail to such waves
// (5 % at 500 jobs, measured per XCD) and the kernel with the plan in it is 3 % slower: off by default there.
uint32_t split_helpers(const gloc_reg* h, uint32_t n_jobs) {
  if (h->nn_mode == 1 || h->nn_split_helpers == 0 || h->nn_split_thresh == 0) return 0;
  const uint32_t hx = h->nn_split_helpers > 0 ? (uint32_t)h->nn_split_helpers : (n_jobs <= 64 ? 256u : (n_jobs <= 256 ? 64u : 0u));
  return std::min<uint32_t>((hx + NN_WPB - 1) / NN_WPB * NN_WPB, 1u << 12);
}

// The split plan's buffers for a batch (NnSplit) with `hx` helper slots per job: everything starts as "no group is split";
// the first pass of a batch therefore runs one wave per group and leaves the estimates the first plan is made from.
int setup_split(gloc_reg* h, const BatchDims& bd, int cs, uint32_t hx, bool chained) {
  h->split = NnSplit{};
  if (hx == 0) return GLOC_OK;
  const size_t S = 64 * (size_t)cs, nj = bd.n_jobs, np = bd.n_part;
  const size_t zero_words = nj * np * 2 + nj * hx;
  const size_t ff_bytes = nj * hx * S * 8 + nj * hx * 4;
  hipStream_t s = h->stream;
  GLOC_TRY(h->split_zero.ensure(zero_words * 4, s));
  GLOC_TRY(h->split_ff.ensure(ff_bytes, s));
  GLOC_HIP(hipMemsetAsync(h->split_zero.p, 0, zero_words * 4, s));
  GLOC_HIP(hipMemsetAsync(h->split_ff.p, 0xFF, ff_bytes, s));
  NnSplit& sp = h->split;
  sp.work = h->split_zero.as<uint32_t>();
  sp.plan = sp.work + nj * np;
  sp.ticket = sp.plan + nj * np;
  sp.skey = h->split_ff.as<unsigned long long>();
  sp.helper = reinterpret_cast<uint32_t*>(sp.skey + nj * hx * S);
  sp.hx = hx;
  // (the chained launch hides a job's longest wave behind the other jobs' work, so fewer groups need splitting: one query
  // alone, registration of 20 jobs, threshold 45 / 60 / 75 / 90 / 120 thousand cycles: 2.92 / 2.89 / 2.79 / 2.78 / 3.03 ms)
  sp.thresh = h->nn_split_thresh_set || !chained ? h->nn_split_thresh : 85000u;
  return GLOC_OK;
}

// The list of a cold pass's heavy groups (NnHeavy): 16 entries per job, at most 16 384; only at two sources per lane.
int setup_heavy(gloc_reg* h, const BatchDims& bd, int cs) {
  h->heavy = NnHeavy{};
  if (h->nn_mode == 1 || cs != 2 || h->nn_heavy_thresh <= 0) return GLOC_OK;
  const size_t cap = std::min<size_t>((size_t)bd.n_jobs * 16, 16384), S = 64 * (size_t)cs;
  hipStream_t s = h->stream;
  // [count | list (cap x 2 words) | ticket (cap words) | skey | hkey], laid out for the largest list the buffer has held
  auto keys_at = [](size_t c) { return (256 + c * 8 + c * 4 + 255) & ~(size_t)255; };
  if (cap > h->heavy_cap) {
    GLOC_TRY(h->heavy_buf.ensure(keys_at(cap) + 2 * cap * S * 8 + 256, s));
    GLOC_HIP(hipMemsetAsync(h->heavy_buf.p, 0, keys_at(cap), s));                                   // count, list, tickets
    GLOC_HIP(hipMemsetAsync(h->heavy_buf.as<char>() + keys_at(cap), 0xFF, cap * S * 8, s));  // fold keys (hkey behind them: written before read)
    h->heavy_cap = cap;
  }
  char* b = h->heavy_buf.as<char>();
  NnHeavy& hv = h->heavy;
  hv.count = reinterpret_cast<uint32_t*>(b);
  hv.list = reinterpret_cast<uint32_t*>(b + 256);
  hv.ticket = reinterpret_cast<uint32_t*>(b + 256 + h->heavy_cap * 8);
  hv.skey = reinterpret_cast<unsigned long long*>(b + keys_at(h->heavy_cap));
  hv.hkey = hv.skey + h->heavy_cap * S;
  hv.cap = (uint32_t)cap;
  hv.thresh = (uint32_t)h->nn_heavy_thresh;
  return GLOC_OK;
}

// The launch order of a batch's 1-NN passes (nn_compact.hpp): slots per group and interleaved shares of a job.  A batch of
// 48 jobs or more: groups of 24 slots, a job per slot (the headline's launches: tuned in rounds 2-6).  A SMALL batch left
// alone (no GLOC_REG_OPT_NN_JOB_GROUP / NN_SUB_JOBS): rows of 8 slots -- one per XCD -- and as few shares of a job as
// spread the batch evenly over the 8 XCDs (20 jobs: 2 shares, 40 slots, five rows; an odd number of jobs: 8): an XCD then
// works on ONE job's share at a time and its L2 holds that job's target instead of three.  Round 5 chose 24 slots x 8 shares on
// rigid copies; on the distinct casts, one query alone, registration of 20 jobs, slots x shares 24 x 8 / 24 x 4 / 24 x 2 /
// 8 x 4 / 8 x 2: launch by launch 3.24 / 3.21 / 3.10 / 3.21 / 3.08 ms, chained 2.69 / 2.66 / 2.72 / 2.68 / 2.62
// (profiles/r06_chain_split_sweep.txt).
void launch_order(const gloc_reg* h, uint32_t n_jobs, uint32_t& jg, uint32_t& subs) {
  subs = h->nn_sub_jobs > 0 ? (uint32_t)h->nn_sub_jobs : (n_jobs < 48 ? 8u : 1u);
  jg = (uint32_t)h->nn_job_group;
  if (h->nn_sub_jobs > 0 || h->nn_job_group_set || n_jobs >= 48) return;
  jg = 8u;
  subs = n_jobs % 4u == 0u ? 2u : (n_jobs % 2u == 0u ? 4u : 8u);
}

// What every launch of the culled search takes (NN_COMPACT_PARAMS, nn_compact.hpp) besides its own grid, start and lists.
struct NnArgs {
  const WsView& v;
  const BatchDims& bd;
  uint32_t jg, n_wg, subs;  // the launch order (launch_order)
  float gate2;
  unsigned long long* stat_pairs;  // profiling only, else null
  unsigned long long* stamp;       // a profiled batch: the slot of the scope this launch opens (ProfScope), else null
  bool keep_d2 = true;             // false: a warm moments pass whose distances nobody reads leaves d2 as it is
};

// One launch of an instance of the culled search; `chain`: the chained launch's NnChain.
template <auto KERNEL, typename... Chain>
void launch_compact(const NnArgs& a, dim3 grid, const uint32_t* prev_corr, bool pairs, NnHeavy hv, Chain... chain) {
  hipLaunchKernelGGL(KERNEL, grid, dim3(64 * NN_WPB), 0, a.v.s, a.v.jobs, a.v.n_jobs, a.jg, a.n_wg, a.subs, a.v.states, prev_corr,
                     a.v.corr, a.keep_d2 ? a.v.d2 : (float*)nullptr, a.v.pairs, pairs ? (double*)nullptr : a.v.partials, a.bd.n_part, a.bd.ld, a.gate2, a.v.split, hv,
                     a.stat_pairs, a.stamp, chain...);
}

// The instance of a pass: sources per lane x pass kind x the split plan.  The warm moments pass with the plan -- what one
// query alone runs pass after pass -- is a kernel of its own at two sources per lane (nn_compact_split_warm_kernel).
template <int CS, bool PAIRS, bool WARM>
void launch_pass(const NnArgs& a, dim3 grid, const uint32_t* prev_corr, NnHeavy hv) {
  if (!a.v.split.hx) {
    if constexpr (CS == 2 && !WARM) launch_compact<nn_compact_cold_kernel<PAIRS>>(a, grid, prev_corr, PAIRS, hv);  // (six waves per SIMD)
    else launch_compact<nn_compact_kernel<CS, PAIRS, false, WARM>>(a, grid, prev_corr, PAIRS, hv);
  }
  else if constexpr (CS == 2 && !PAIRS && WARM) launch_compact<nn_compact_split_warm_kernel<2>>(a, grid, prev_corr, PAIRS, hv);
  else launch_compact<nn_compact_kernel<CS, PAIRS, true, WARM>>(a, grid, prev_corr, PAIRS, hv);
}

// (the pass that writes the pairs is a batch's first: a cold one)
template <int CS>
void launch_kind(const NnArgs& a, dim3 grid, const uint32_t* prev_corr, NnHeavy hv, bool want_pairs, bool warm) {
  if (want_pairs) launch_pass<CS, true, false>(a, grid, prev_corr, hv);
  else if (warm) launch_pass<CS, false, true>(a, grid, prev_corr, hv);
  else launch_pass<CS, false, false>(a, grid, prev_corr, hv);
}

// S1 for every job of the batch.  warm: corr holds the previous pass's result.  want_pairs: write the (moved
// source, matched target) pairs INSTEAD of the moments (the RANSAC stage refits from the pairs: accum_kernel<1>).  The culled search leaves the wave partials of the
// fp64 moments in h->partials (per source group); the exhaustive one needs accum_kernel<0> afterwards.
// join: the pass follows a profiled scope with nothing enqueued in between (a warm pass behind its solve).
// keep_d2 = false: a warm moments pass of the culled search that another pass follows -- nothing reads its distances (the
// exhaustive mode's accum_kernel<0>, gloc_reg_debug_corr and the refinements read those of the pass before them) and it
// does not write them.
int launch_nn(gloc_reg* h, const BatchDims& bd, const WsView& v, bool warm, bool want_pairs, float gate2, ProfScope::Join join = ProfScope::Apart,
              bool keep_d2 = true) {
  // (the first pass of a batch -- no previous correspondence, or the pass that writes the pairs -- is another
  // instantiation and ~1.6 x a warm pass: also counted in its own family, on the same span, so that "nn" - "nn_cold"
  // is the warm passes alone)
  ProfScope ps(h->prof, "nn", v.s, join, (want_pairs || !warm) ? "nn_cold" : nullptr);
  h->nn_launches++;
  if (h->nn_mode == 1) {
    dim3 grid((bd.max_src + 256 * NN_S - 1) / (256 * NN_S), v.n_jobs);
    hipLaunchKernelGGL(nn_kernel, grid, dim3(256), 0, v.s, v.jobs, v.states,
                       v.corr, v.d2, bd.ld, ps.stamp);
    if (want_pairs)
      hipLaunchKernelGGL(gather_pairs_kernel, dim3((bd.max_src + 255) / 256, v.n_jobs), dim3(256), 0, v.s,
                         v.jobs, v.states, v.corr, bd.ld,
                         v.pairs);
  } else {
    const int cs = h->nn_src_per_lane;
    const bool cold = want_pairs || !warm;
    const NnHeavy hv = cold ? v.heavy : NnHeavy{};
    if (hv.cap) GLOC_HIP(hipMemsetAsync(hv.count, 0, 4, v.s));
    const uint32_t n_wg_job = (bd.max_groups + v.split.hx + NN_WPB - 1) / NN_WPB;  // helper waves first, then one per group
    // slots of the launch order (nn_compact.hpp): a job each, or -- few jobs -- `subs` interleaved shares of a job, so
    // that the 8 XCDs get equal numbers of slots
    // (8 shares -- one per XCD -- since round 5: one query alone 105.4 -> 104.1 / 104.4 us per pass against 4)
    uint32_t jg, subs;
    launch_order(h, v.n_jobs, jg, subs);
    // (one group of all the slots of a small batch, so that every job's helpers start at the head of the launch, was
    // tried: one query alone 0.115 ms per pass against 0.108 with groups of 24)
    const uint32_t n_slots = v.n_jobs * subs;
    const uint32_t n_wg = (n_wg_job + subs - 1) / subs;
    const unsigned grid = n_wg * jg * ((n_slots + jg - 1) / jg);
    // (launched as (slots of a group, work-groups of a slot, groups): the same linear order without the divisions)
    GLOC_REQUIRE(n_wg <= 65535u && (n_slots + jg - 1) / jg <= 65535u, GLOC_ERR_INVALID,
                 "the culled search's grid: %u work-groups per job slot (scans above ~8 M points) or %u job groups exceed 65535", n_wg,
                 (n_slots + jg - 1) / jg);
    if (grid) {
      NnArgs a{v, bd, jg, n_wg, subs, gate2, h->prof.enabled ? h->counters.as<unsigned long long>() : nullptr, ps.stamp,
               keep_d2 || !warm || want_pairs};
      const dim3 g3(jg, n_wg, (n_slots + jg - 1) / jg);
      const uint32_t* prev_corr = warm ? v.corr : nullptr;
      if (cs == 1) launch_kind<1>(a, g3, prev_corr, hv, want_pairs, warm);
      else if (cs == 2) launch_kind<2>(a, g3, prev_corr, hv, want_pairs, warm);
      else launch_kind<4>(a, g3, prev_corr, hv, want_pairs, warm);
      if (hv.cap) {  // the groups the cold pass's waves gave up: NN_HEAVY_PARTS waves each (the list's length stays on the device)
        const dim3 gh(hv.cap * NN_HEAVY_PARTS);
        a.stamp = nullptr;  // (the scope's second launch: its time is the scope's)
        if (want_pairs) launch_compact<nn_compact_heavy_kernel<2, true>>(a, gh, nullptr, true, hv);
        else launch_compact<nn_compact_heavy_kernel<2, false>>(a, gh, nullptr, false, hv);
      }
    }
  }
  GLOC_HIP(hipGetLastError());
  return GLOC_OK;
}

// Will the warm passes of a batch -- `warm_passes` of them behind its first, cold, pass -- run as ONE launch (NnChain,
// reg_kernels.hpp; nn_chain_kernel, nn_compact.hpp): search, reduce, solve, plan, pass after pass?  Decided once per
// batch, before the split threshold (setup_split) and for every pass of it: a small batch at two sources per lane with the
// split plan (`hx` helper slots per job) and at least two warm passes; else the batch goes on launch by launch.
bool batch_chains(const gloc_reg* h, const BatchDims& bd, uint32_t hx, uint32_t warm_passes) {
  if (!h->nn_chain || h->chain_broken || h->nn_mode == 1 || h->nn_src_per_lane != 2 || h->prof.enabled || NN_WPB != 1) return false;
  if (hx == 0 || warm_passes < 2) return false;
  uint32_t jg, subs;
  launch_order(h, bd.n_jobs, jg, subs);
  if (bd.n_jobs >= 48 || (jg & 7u) || jg % subs) return false;  // (small batches; a group of slots holds whole jobs)
  if ((bd.n_part & 31u) || (hx & 31u)) return false;            // (a job's rows of the per-pass tables are whole cache lines)
  const uint32_t n_wg = ((bd.max_groups + hx + NN_WPB - 1) / NN_WPB + subs - 1) / subs;
  const uint32_t groups = (bd.n_jobs * subs + jg - 1) / jg;
  const uint64_t grp_size = ((uint64_t)jg * n_wg + (jg / subs) * NN_CHAIN_ROLES + 7) & ~7ull;
  return grp_size * groups * warm_passes < (1ull << 31);
}

int launch_nn_chain(gloc_reg* h, const BatchDims& bd, const WsView& v, uint32_t n_pass, float gate2) {
  uint32_t jg, subs;
  launch_order(h, v.n_jobs, jg, subs);
  const uint32_t n_wg = ((bd.max_groups + v.split.hx + NN_WPB - 1) / NN_WPB + subs - 1) / subs;
  const uint32_t groups = (v.n_jobs * subs + jg - 1) / jg;
  NnChain ch{};
  ch.n_pass = n_pass;
  ch.expected = subs * n_wg * NN_WPB + (h->chain_stall ? 1u : 0u);
  ch.jobs_per_grp = jg / subs;
  ch.grp_size = (jg * n_wg + ch.jobs_per_grp * NN_CHAIN_ROLES + 7u) & ~7u;
  ch.pass_size = ch.grp_size * groups;
  // [ready | done | go | sdone] a 256-byte line per (pass, job), the err word's line; then (never cleared: written before
  // read) the per-pass poses, plans and helpers' tables, the reducers' sub-sums
  const size_t cells = (size_t)n_pass * v.n_jobs, line = NN_CHAIN_PAD * 4;
  const size_t head = (4 * cells + 1) * line;
  const size_t t_bytes = cells * NN_CHAIN_T_STRIDE * 4;
  const size_t plan_bytes = (size_t)(n_pass - 1) * v.n_jobs * bd.n_part * 4, help_bytes = (size_t)(n_pass - 1) * v.n_jobs * v.split.hx * 4;
  const size_t sub_bytes = sizeof(double) * ACC_NV * NN_CHAIN_RED * v.n_jobs;
  GLOC_TRY(h->chain_buf.ensure(head + t_bytes + plan_bytes + help_bytes + sub_bytes + 256, v.s));
  GLOC_HIP(hipMemsetAsync(h->chain_buf.p, 0, head, v.s));
  char* base = h->chain_buf.as<char>();
  ch.ready = reinterpret_cast<uint32_t*>(base);
  ch.done = reinterpret_cast<uint32_t*>(base + cells * line);
  ch.go = reinterpret_cast<uint32_t*>(base + 2 * cells * line);
  ch.sdone = reinterpret_cast<uint32_t*>(base + 3 * cells * line);
  ch.err = reinterpret_cast<uint32_t*>(base + 4 * cells * line);
  ch.Tp = reinterpret_cast<float*>(base + head);
  ch.planp = reinterpret_cast<uint32_t*>(base + head + t_bytes);
  ch.helperp = reinterpret_cast<uint32_t*>(base + head + t_bytes + plan_bytes);
  ch.sub = reinterpret_cast<double*>(base + head + t_bytes + plan_bytes + help_bytes);
  h->nn_launches += n_pass;
  h->chain_launches++;
  h->chain_in_batch = true;
  const NnArgs a{v, bd, jg, n_wg, subs, gate2, nullptr, nullptr};
  launch_compact<nn_chain_kernel<2>>(a, dim3(ch.pass_size * n_pass), v.corr, false, NnHeavy{}, ch);
  GLOC_HIP(hipGetLastError());
  GLOC_HIP(hipMemcpyAsync(h->h_chain_err, ch.err, 4, hipMemcpyDeviceToHost, v.s));
  return GLOC_OK;
}

int ensure_pinned(gloc_reg* h, uint32_t n_jobs, uint32_t n_stamps) {
  static_assert(sizeof(CandState) % 8 == 0 && sizeof(Job) % 4 == 0, "the stamps behind the states are 64-bit words, the jobs behind them 32-bit");
  const size_t need = (sizeof(CandState) + sizeof(Job)) * (size_t)n_jobs + 8 * (size_t)n_stamps + 64;
  if (need > h->pin_cap) {
    if (h->pin) (void)hipHostFree(h->pin);
    h->pin = nullptr;
    h->pin_cap = 0;
    const size_t cap = need + need / 2 + 4096;
    GLOC_HIP(hipHostMalloc(&h->pin, cap, hipHostMallocDefault));
    h->pin_cap = cap;
  }
  h->h_states = reinterpret_cast<CandState*>(h->pin);
  h->h_jobs = reinterpret_cast<Job*>(reinterpret_cast<unsigned long long*>(h->h_states + n_jobs) + n_stamps);
  h->h_chain_err = reinterpret_cast<uint32_t*>(h->h_jobs + n_jobs);
  return GLOC_OK;
}

// What a batch asks of the handle's workspaces (open_batch).
struct BatchSpec {
  uint32_t n_jobs, max_src;
  uint32_t max_groups;   // source groups of its longest source (0: the batch never searches)
  bool search;           // it runs launch_nn: corr / d2, the counters, the heavy list
  bool pairs;            // it runs on pairs: the pairs and, for `hyp` hypotheses per job, Rt / valid / inliers ...
  size_t hyp;
  bool alive;            // ... and ransac_alive_kernel's lists
  uint32_t split_hx;     // helper slots per job of the split plan (split_helpers; 0: none) ...
  uint32_t warm_passes;  // ... and the passes behind its first that could run chained (batch_chains)
  uint32_t stamps = 0;   // a profiled registration batch: the words of its time line (Profiler::open_stamps), behind the states
  // a batch that searches (and no more: RANSAC and the split plan are added by enqueue_jobs) / a batch on pairs alone
  static BatchSpec searching(uint32_t n_jobs, size_t max_src, uint32_t max_groups) {
    return BatchSpec{n_jobs, (uint32_t)max_src, max_groups, true, false, 0, false, 0u, 0u, 0u};
  }
  static BatchSpec on_pairs(uint32_t n_jobs, size_t max_src, size_t hyp, bool alive) {
    return BatchSpec{n_jobs, (uint32_t)max_src, 0u, false, true, hyp, alive, 0u, 0u, 0u};
  }
};

// An open batch: its shape, accum_kernel's blocks per job, whether its warm passes are one launch, the workspaces.
struct Batch {
  BatchDims bd;
  uint32_t nblocks;
  bool chained;
  WsView v;
};

// Opens a batch on the handle -- the ONE place where its workspaces are laid out: the shape, the pinned staging, the
// buffers the spec asks for, fill(jobs, states) into the staging and both tables up, the split plan and the heavy list (or
// none), the view the launches take.  It also owns what gloc_reg_debug_corr may read afterwards: last_ld / last_jobs
// describe a searching batch, and a batch on pairs -- whose job table has no scans behind it -- leaves last_jobs = 0, as
// does a batch that failed to open.
template <class Fill>
int open_batch(gloc_reg* h, const BatchSpec& sp, Batch* out, Fill&& fill) {
  const uint32_t n_jobs = sp.n_jobs;
  const int cs = h->nn_src_per_lane;
  hipStream_t s = h->stream;
  Batch& b = *out;
  b = Batch{};
  BatchDims& bd = b.bd;
  bd = BatchDims{n_jobs, sp.max_src, sp.max_groups, 0, 0};
  b.nblocks = (bd.max_src + ACC_PER_BLOCK - 1) / ACC_PER_BLOCK;
  bd.n_part = (std::max<uint32_t>(std::max(bd.max_groups, b.nblocks), 1) + 31u) & ~31u;  // (a job's row of a [job][n_part] table: whole 128-byte lines)
  bd.ld = ((size_t)bd.max_src + 127) & ~(size_t)127;
  h->last_jobs = 0;
  GLOC_TRY(ensure_pinned(h, n_jobs, sp.stamps));
  h->prof.slots.clear();  // (a profiled batch that was never collected: its time line lay in the staging this batch takes)
  h->prof.h_stamps = nullptr;
  h->chain_in_batch = false;
  *h->h_chain_err = 0u;
  fill(h->h_jobs, h->h_states);
  // (the stamps start at zero: they go up with the states, in the same copy, and come down with them)
  const size_t state_bytes = sizeof(CandState) * n_jobs + 8 * (size_t)sp.stamps;
  if (sp.stamps) memset(h->h_states + n_jobs, 0, 8 * (size_t)sp.stamps);
  WsView& v = b.v;
  v.s = s;
  v.n_jobs = n_jobs;
  GLOC_TRY(h->jobs.ensure(sizeof(Job) * n_jobs, s));
  GLOC_TRY(h->states.ensure(state_bytes, s));
  GLOC_TRY(h->partials.ensure(sizeof(double) * ACC_NV * (size_t)bd.n_part * n_jobs, s));
  v.jobs = h->jobs.as<Job>();
  v.states = h->states.as<CandState>();
  v.partials = h->partials.as<double>();
  if (sp.search) {
    if (!h->counters.p) {
      GLOC_TRY(h->counters.ensure(8 * NN_STAT_SLOTS, s));
      GLOC_HIP(hipMemsetAsync(h->counters.p, 0, 8 * NN_STAT_SLOTS, s));
    }
    GLOC_TRY(h->corr.ensure(sizeof(uint32_t) * std::max<size_t>(bd.ld, 1) * n_jobs, s));
    GLOC_TRY(h->d2.ensure(sizeof(float) * std::max<size_t>(bd.ld, 1) * n_jobs, s));
    v.corr = h->corr.as<uint32_t>();
    v.d2 = h->d2.as<float>();
  }
  if (sp.pairs) {
    GLOC_TRY(h->pairs.ensure(sizeof(f32x4) * 2 * bd.ld * n_jobs, s));
    GLOC_TRY(h->Rt.ensure(sizeof(float) * 12 * sp.hyp * n_jobs, s));
    GLOC_TRY(h->valid.ensure(sizeof(uint32_t) * 2 * sp.hyp * n_jobs, s));
    v.pairs = h->pairs.as<f32x4>();
    v.Rt = h->Rt.as<float>();
    v.valid = h->valid.as<uint32_t>();
    v.inliers = v.valid + sp.hyp * n_jobs;
    if (sp.alive) {
      GLOC_TRY(h->alive.ensure(sizeof(uint32_t) * (sp.hyp + 1) * n_jobs, s));
      v.a_idx = h->alive.as<uint32_t>();
      v.a_cnt = v.a_idx + sp.hyp * n_jobs;
    }
  }
  GLOC_HIP(hipMemcpyAsync(v.jobs, h->h_jobs, sizeof(Job) * n_jobs, hipMemcpyHostToDevice, s));
  GLOC_HIP(hipMemcpyAsync(v.states, h->h_states, state_bytes, hipMemcpyHostToDevice, s));
  b.chained = batch_chains(h, bd, sp.split_hx, sp.warm_passes);
  GLOC_TRY(setup_split(h, bd, cs, sp.split_hx, b.chained));  // (no helper slots: h->split = NnSplit{})
  if (sp.search) GLOC_TRY(setup_heavy(h, bd, cs));
  else h->heavy = NnHeavy{};
  v.split = h->split;
  v.heavy = h->heavy;
  if (sp.search) {
    h->last_ld = bd.ld;
    h->last_jobs = n_jobs;
  }
  return GLOC_OK;
}

// The geometry of ransac_score_kernel's grid.  Pairs per work-group: 4096 -- or 1024 in a small batch (one query alone:
// 20 jobs x 31 chunks = 620 work-groups for 256 CUs, each walking 16 tiles behind two barriers: 75 us for the first 16
// hypotheses).
uint32_t score_chunk_len(uint32_t n_jobs, uint32_t max_src) {
  static_assert(1024 % SC_STAGE == 0 && SC_CHUNK % SC_STAGE == 0, "whole tiles");
  return (size_t)n_jobs * ((max_src + SC_CHUNK - 1) / SC_CHUNK) >= 2048 ? (uint32_t)SC_CHUNK : 1024u;
}

// Hypotheses per work-group for `len` of them: 16 / 64 (its four waves share them and split every staged tile) or
// thread <-> hypothesis.
uint32_t score_hpb(uint32_t len) { return len <= 16 ? 16u : (len <= 64 ? 64u : 256u); }

// The refit on the winning hypothesis' inliers among the pairs, behind the scan that chose it.
int enqueue_refit(gloc_reg* h, const BatchDims& bd, const WsView& v, float thr2, uint32_t nblocks) {
  const uint32_t n_jobs = v.n_jobs;
  {  // (both callers come straight from their last ransac_score scope)
    ProfScope ps(h->prof, "accum", v.s, ProfScope::Joined);
    hipLaunchKernelGGL(accum_kernel<1>, dim3(nblocks, n_jobs), dim3(ACC_THREADS), 0, v.s, v.jobs, v.states, v.corr, v.d2, v.pairs, bd.ld, thr2,
                       v.partials, bd.n_part, ps.stamp);
    GLOC_HIP(hipGetLastError());
  }
  {
    ProfScope ps(h->prof, "solve", v.s, ProfScope::Joined);
    hipLaunchKernelGGL(solve_kernel<1>, dim3(v.split.hx ? 2 * n_jobs : n_jobs), dim3(v.split.hx ? SOLVE_THREADS : SOLVE_THREADS_LIGHT), 0, v.s, v.partials, bd.n_part, false, v.jobs,
                       v.states, v.split, n_jobs, ps.stamp);
    GLOC_HIP(hipGetLastError());
  }
  return GLOC_OK;
}

// The RANSAC stage on the pairs in v.pairs (jobs[c].n_src of them per job, sampled through jobs[c].src_inv when it is set):
// hypotheses, scores, the sequential rule with its adaptive stop, the refit on the winner's inliers.  What
// gloc_reg_batch_* runs behind its pairs pass and gloc_reg_fpfh_batch_ids behind its descriptor matches.
struct RansacRule {
  uint32_t iters;
  float inlier_thresh, min_inlier_ratio, confidence;
  uint64_t seed;
};

int enqueue_ransac(gloc_reg* h, const BatchDims& bd, const RansacRule& r, const WsView& v, uint32_t nblocks) {
  const uint32_t n_jobs = v.n_jobs;
  hipStream_t s = v.s;
  const uint32_t H = r.iters;
  // Phases of hypotheses, each generated, scored and scanned before the next: with the adaptive stop (the
  // reference's call: confidence 0.99) and ~85 % inliers the iteration count drops to 5 - 8 at the first good
  // hypothesis, so [0, 16) settles nearly every job, [16, 64) most of the rest; a job that is done is skipped by the
  // later phases (its blocks exit at once).  The rule is sequential in h (ransac_scan_kernel), so the split does not
  // change the result.  (Round 2 scored 64 first: 2.1 ms per step of 500 jobs, 0.6 with 16.  A first phase of 8 takes the
  // first score launch from 490 to 353 us, and the step nowhere: a third launch and hand-over, LAB_NOTES.md.)
  const bool adaptive = r.confidence > 0.f && r.confidence < 1.f;
  uint32_t bounds[4] = {0u, 0u, 0u, 0u};
  int n_ph = 0;
  for (uint32_t b : {adaptive ? 16u : 256u, adaptive ? 64u : H, H})
    if (b <= H && b > bounds[n_ph]) bounds[++n_ph] = b;
  if (bounds[n_ph] < H) bounds[++n_ph] = H;
  // never-generated = invalid, no inliers counted: one fill, the two tables lie end to end (open_batch, for both callers'
  // batches: H hypotheses per job)
  GLOC_REQUIRE(v.inliers == v.valid + (size_t)H * n_jobs, GLOC_ERR_STATE, "the batch was not opened for %u hypotheses per job", H);
  GLOC_HIP(hipMemsetAsync(v.valid, 0, 2 * sizeof(uint32_t) * (size_t)H * n_jobs, s));
  const float thr2 = r.inlier_thresh * r.inlier_thresh;
  const uint32_t chunk_len = score_chunk_len(n_jobs, bd.max_src);
  const unsigned cchunks = (bd.max_src + chunk_len - 1) / chunk_len;
  for (int ph = 0; ph < n_ph; ++ph) {
    const uint32_t h0 = bounds[ph], h1 = bounds[ph + 1], len = h1 - h0;
    const CandState* st = ph ? v.states : (const CandState*)nullptr;
    {
      ProfScope ps(h->prof, "ransac_hyp", s, ph ? ProfScope::Joined : ProfScope::Apart);  // (behind the phase before; the first behind the fills)
      hipLaunchKernelGGL(ransac_hyp_kernel, dim3((len + 127) / 128, n_jobs), dim3(128), 0, s, v.pairs, bd.ld,
                         v.jobs, r.seed, H, h0, h1, st, v.Rt, v.valid, ps.stamp);
      GLOC_HIP(hipGetLastError());
    }
    ProfScope ps(h->prof, "ransac_score", s, ProfScope::Joined);
    const uint32_t hpb = score_hpb(len);
    const unsigned NP = 8;
    if (!adaptive && ph > 0 && len >= 512 && cchunks >= NP) {
      // every hypothesis scored, not every pair of every hypothesis: an eighth of the pairs at a time, the hypotheses
      // that can no longer beat the first phase's winner dropped in between (ransac_alive_kernel)
      uint32_t* a_idx = v.a_idx;
      uint32_t* a_cnt = v.a_cnt;
      for (unsigned q = 0; q < NP; ++q) {
        const unsigned c0 = q * cchunks / NP, c1 = (q + 1) * cchunks / NP;
        hipLaunchKernelGGL(ransac_alive_kernel, dim3(n_jobs), dim3(1024), 0, s, v.inliers, v.valid,
                           H, h0, h1, v.jobs, v.states, (uint32_t)(c0 * chunk_len), a_idx, a_cnt, q ? nullptr : ps.stamp);
        hipLaunchKernelGGL(ransac_score_kernel, dim3((len + 255) / 256, c1 - c0, n_jobs), dim3(256), 0, s,
                           v.pairs, bd.ld, v.jobs, H, h0, 256u, v.Rt,
                           v.valid, thr2, st, v.inliers, a_idx, a_cnt, (uint32_t)c0, chunk_len, (unsigned long long*)nullptr);
      }
    } else {
      hipLaunchKernelGGL(ransac_score_kernel, dim3((len + hpb - 1) / hpb, cchunks, n_jobs), dim3(256), 0, s,
                         v.pairs, bd.ld, v.jobs, H, h0, hpb, v.Rt,
                         v.valid, thr2, st, v.inliers, (const uint32_t*)nullptr,
                         (const uint32_t*)nullptr, 0u, chunk_len, ps.stamp);
    }
    if (ph + 1 < n_ph)
      hipLaunchKernelGGL(ransac_scan_kernel<false>, dim3(n_jobs), dim3(64), 0, s, v.inliers,
                         v.valid, v.Rt, H, h0, h1, v.jobs, r.confidence,
                         r.min_inlier_ratio, v.states);
    else
      hipLaunchKernelGGL(ransac_scan_kernel<true>, dim3(n_jobs), dim3(64), 0, s, v.inliers,
                         v.valid, v.Rt, H, h0, h1, v.jobs, r.confidence,
                         r.min_inlier_ratio, v.states);
    GLOC_HIP(hipGetLastError());
  }
  return enqueue_refit(h, bd, v, thr2, nblocks);
}

// The launches of a batch: S1 -> S2 (RANSAC + refit) -> S3 (ICP).  chained: its warm passes are one launch (batch_chains).
int enqueue_pipeline(gloc_reg* h, const BatchDims& bd, const gloc_reg_params* prm, const WsView& v, bool can, bool any_tgt,
                     uint32_t nblocks, bool chained) {
  const uint32_t n_jobs = v.n_jobs;
  hipStream_t s = v.s;
  const bool culled = h->nn_mode != 1;
  const float gate2 = prm->max_corr_dist > 0.f ? prm->max_corr_dist * prm->max_corr_dist : 0.f;
  bool have_corr = false;  // corr holds a previous pass's result: warm start for the next one

  if (can && any_tgt && prm->ransac_iters > 0) {
    GLOC_TRY(launch_nn(h, bd, v, false, true, 0.f));
    have_corr = true;
    GLOC_TRY(enqueue_ransac(h, bd, RansacRule{prm->ransac_iters, prm->inlier_thresh, prm->min_inlier_ratio, prm->ransac_confidence, prm->seed},
                            v, nblocks));
  }
  for (uint32_t it = 0; it < prm->icp_iters && can && any_tgt; ++it) {
    if (chained && have_corr) {  // a small batch: all the passes that are left in one launch
      GLOC_TRY(launch_nn_chain(h, bd, v, prm->icp_iters - it, gate2));
      break;
    }
    // (profiled scopes end to end: this pass behind the refit's or the previous pass's solve -- a batch's first launch
    // apart, behind the preamble's copies and fills -- and the solve behind its pass)
    GLOC_TRY(launch_nn(h, bd, v, have_corr, false, gate2, have_corr ? ProfScope::Joined : ProfScope::Apart, it + 1 == prm->icp_iters));
    have_corr = true;
    if (!culled) {
      ProfScope ps(h->prof, "accum", s, ProfScope::Joined);
      hipLaunchKernelGGL(accum_kernel<0>, dim3(nblocks, n_jobs), dim3(ACC_THREADS), 0, s, v.jobs,
                         v.states, v.corr, v.d2,
                         (const f32x4*)nullptr, bd.ld, gate2, v.partials, bd.n_part, ps.stamp);
      GLOC_HIP(hipGetLastError());
    }
    {
      ProfScope ps(h->prof, "solve", s, ProfScope::Joined);
      hipLaunchKernelGGL(solve_kernel<0>, dim3(v.split.hx ? 2 * n_jobs : n_jobs), dim3(v.split.hx ? SOLVE_THREADS : SOLVE_THREADS_LIGHT), 0, s, v.partials,
                         bd.n_part, culled, v.jobs, v.states, v.split, n_jobs, ps.stamp);
      GLOC_HIP(hipGetLastError());
    }
  }
  return GLOC_OK;
}

// The whole pipeline for a batch of jobs, device resident: S1 -> S2 (RANSAC + refit) -> S3 (ICP), ENQUEUED on the
// handle's stream with the copy of the per-job results behind it and an event behind that: returns without waiting.
int enqueue_jobs(gloc_reg* h, const std::vector<JobHost>& jh, const gloc_reg_params* prm) {
  const uint32_t n_jobs = (uint32_t)jh.size();
  if (n_jobs == 0) return GLOC_OK;
  const int cs = h->nn_src_per_lane;
  uint32_t max_src = 0;
  bool can = false, any_tgt = false;
  for (const JobHost& j : jh) {
    max_src = std::max<uint32_t>(max_src, (uint32_t)j.src.n);
    can |= j.src.n >= 3;
    any_tgt |= j.tgt.n >= 1;
  }
  const bool ransac = can && any_tgt && prm->ransac_iters > 0;
  const bool adaptive = prm->ransac_confidence > 0.f && prm->ransac_confidence < 1.f;
  // the warm passes: the ICP passes behind the batch's first, cold, pass (RANSAC's pairs pass, else the first ICP pass)
  const uint32_t warm_passes = !(can && any_tgt) ? 0u : (ransac ? prm->icp_iters : std::max<uint32_t>(prm->icp_iters, 1u) - 1u);
  BatchSpec spec = BatchSpec::searching(n_jobs, max_src, src_groups(max_src, cs));
  spec.pairs = ransac;
  spec.hyp = prm->ransac_iters;
  spec.alive = !adaptive;
  spec.split_hx = split_helpers(h, n_jobs);
  spec.warm_passes = warm_passes;
  // Profiled: the batch's time line is stamped on the device (Profiler::open_stamps).  The scopes it can open, each a slot:
  // per ICP pass the search and the solve -- and between them, in the exhaustive mode, accum_kernel<0>'s; RANSAC's pairs pass,
  // its hypotheses and scores of at most three phases, the refit's accum and solve (9); and the closing stamp's word.
  const bool stamped = h->prof.enabled;
  if (stamped) spec.stamps = (h->nn_mode == 1 ? 3u : 2u) * prm->icp_iters + 9u + 1u;
  Batch b;
  GLOC_TRY(open_batch(h, spec, &b, [&](Job* jd, CandState* st) {
    for (uint32_t c = 0; c < n_jobs; ++c) {
      const DevScan &s = jh[c].src, &t = jh[c].tgt;
      jd[c] = Job{s.idx.pts, s.order, s.idx.inv, t.xyz, t.idx, (uint32_t)s.n, src_groups(s.n, cs), jh[c].stream_id, 0u};
      init_state(st[c], jh[c].init_T, prm->ransac_iters);
      if (s.n < 3) st[c].frozen = 1;  // nothing to estimate: T stays the initial guess
    }
  }));
  hipStream_t s = h->stream;
  unsigned long long* d_stamps = reinterpret_cast<unsigned long long*>(b.v.states + n_jobs);
  if (stamped) GLOC_TRY(h->prof.open_stamps(h->device, d_stamps, spec.stamps));
  const int rc = enqueue_pipeline(h, b.bd, prm, b.v, can, any_tgt, b.nblocks, b.chained);
  if (stamped) {  // (also where the pipeline failed: no scope after this takes a slot)
    unsigned long long* last = h->prof.close_stamps(reinterpret_cast<const unsigned long long*>(h->h_states + n_jobs));
    if (rc == GLOC_OK) hipLaunchKernelGGL(stamp_kernel, dim3(1), dim3(64), 0, s, last);
    // (a scope without a slot would be counted with no time, and its time would go to the family of the last slot)
    GLOC_REQUIRE(rc != GLOC_OK || h->prof.slots.size() < spec.stamps, GLOC_ERR_STATE,
                 "the profiled batch opened %zu scopes, its time line has %u slots", h->prof.slots.size(), spec.stamps - 1u);
  }
  GLOC_TRY(rc);
  GLOC_HIP(hipGetLastError());
  GLOC_HIP(hipMemcpyAsync(h->h_states, h->states.p, sizeof(CandState) * n_jobs + 8 * (size_t)spec.stamps, hipMemcpyDeviceToHost, s));
  GLOC_HIP(hipEventRecord(h->done_ev, s));
  if (h->chain_in_batch) {  // (a small batch: a few KB)
    h->retry_jobs.resize(sizeof(JobHost) * n_jobs);
    memcpy(h->retry_jobs.data(), jh.data(), sizeof(JobHost) * n_jobs);
    h->retry_T.assign((size_t)16 * n_jobs, 0.f);
    for (uint32_t c = 0; c < n_jobs; ++c)
      if (jh[c].init_T) memcpy(&h->retry_T[(size_t)16 * c], jh[c].init_T, sizeof(float) * 16);
    h->retry_prm = *prm;
  }
  return GLOC_OK;
}

// Waits for the results of the batch enqueue_jobs() queued last (its own event: not for the stream, which may carry the
// next batch of a handle sharing it) and unpacks them, per job, in job order.
int collect_jobs(gloc_reg* h, uint32_t n_jobs, const size_t* n_src_of, float max_rmse, float max_final_step, float* out_T,
                 float* out_rmse, uint32_t* out_inliers, int* out_ok) {
  h->last_final_step.assign(n_jobs, 0.f);
  if (n_jobs == 0) return GLOC_OK;
  GLOC_HIP(hipEventSynchronize(h->done_ev));
  if (h->chain_in_batch && *h->h_chain_err) {
    // A wait inside the chained launch ran out (NN_CHAIN_WAIT_TICKS): its waves left without finishing the passes -- the
    // poses are not results.  The handle goes back to one launch per pass for good, and THIS batch is run again that
    // way, here (its scans are still pinned: the batch has not been collected): the caller gets the launch-by-launch bits,
    // late.  Counted (gloc_reg_debug_chain) and said on stderr once per handle.
    const bool first = !h->chain_broken;
    h->chain_broken = true;
    h->chain_timeouts++;
    if (first)
      fprintf(stderr, "[gloc3d] the chained ICP passes of a batch of %u jobs timed out on the device (a wait for a job's solve ran out): "
                      "the batch is run again launch by launch, and this handle launches pass by pass from now on\n", n_jobs);
    GLOC_REQUIRE(h->retry_jobs.size() == sizeof(JobHost) * n_jobs, GLOC_ERR_HIP,
                 "the chained ICP passes of a batch of %u jobs timed out on the device and the batch cannot be run again", n_jobs);
    std::vector<JobHost> jh(n_jobs);
    memcpy(jh.data(), h->retry_jobs.data(), sizeof(JobHost) * n_jobs);
    for (uint32_t c = 0; c < n_jobs; ++c)
      if (jh[c].init_T) jh[c].init_T = &h->retry_T[(size_t)16 * c];
    const gloc_reg_params prm = h->retry_prm;
    if (const int rc = enqueue_jobs(h, jh, &prm)) {
      // (what it queued before failing may still read the batch's scans, and done_ev is the first run's: as multi_begin)
      (void)hipStreamSynchronize(h->stream);
      return rc;
    }
    GLOC_HIP(hipEventSynchronize(h->done_ev));
  }
  h->prof.fold_stamps();  // (a profiled batch: its time line came down with the states)
  for (uint32_t c = 0; c < n_jobs; ++c) {
    const CandState& st = h->h_states[c];
    const size_t n_src = n_src_of[c];
    pose_to_T16(st, out_T + 16 * (size_t)c);
    const float rmse = n_src ? (float)std::sqrt(st.sum_d2 / (double)n_src) : 0.f;
    if (out_rmse) out_rmse[c] = rmse;
    if (out_inliers) out_inliers[c] = st.best_inl;
    // plausibility of the estimate (include/gloc3d.h: max_final_step, max_rmse): the ICP converged, the residual is bounded
    h->last_final_step[c] = st.last_step;
    if (out_ok)
      out_ok[c] = st.ok && !(max_rmse > 0.f && !(rmse <= max_rmse)) && !(max_final_step > 0.f && !(st.last_step <= max_final_step));
  }
  return GLOC_OK;
}

int run_jobs(gloc_reg* h, const std::vector<JobHost>& jh, const gloc_reg_params* prm, float* out_T, float* out_rmse,
             uint32_t* out_inliers, int* out_ok) {
  GLOC_TRY(enqueue_jobs(h, jh, prm));
  std::vector<size_t> n_src(jh.size());
  for (size_t c = 0; c < jh.size(); ++c) n_src[c] = jh[c].src.n;
  return collect_jobs(h, (uint32_t)jh.size(), n_src.data(), prm->max_rmse, prm->icp_iters ? prm->max_final_step : 0.f, out_T,
                      out_rmse, out_inliers, out_ok);
}

// Every entry point that runs jobs on the handle's workspaces (enqueue_jobs / launch_nn: pinned staging, job table,
// states, corr, partials, the done event) is refused while a batch is between gloc_reg_batch_multi_begin and _end:
// it would overwrite what that batch's D2H copy and unpacking still read.
#define GLOC_NOT_PENDING(h) \
  GLOC_REQUIRE(!(h)->pending.active, GLOC_ERR_STATE, "a batch is in flight on this handle: call gloc_reg_batch_multi_end first")

int check_params(const gloc_reg_params* p) {
  GLOC_REQUIRE(p, GLOC_ERR_INVALID, "params is null");
  GLOC_REQUIRE(p->ransac_iters <= (1u << 20), GLOC_ERR_INVALID, "ransac_iters too large");
  GLOC_REQUIRE(p->icp_iters <= 10000, GLOC_ERR_INVALID, "icp_iters too large");
  GLOC_REQUIRE(p->ransac_iters == 0 || p->inlier_thresh > 0.f, GLOC_ERR_INVALID,
               "inlier_thresh must be > 0");
  return GLOC_OK;
}

int ensure_store(gloc_reg* h) {
  if (h->store) return GLOC_OK;
  GLOC_TRY(gloc_scan_store_create(h->device, &h->own_store));
  h->store = h->own_store;
  h->store->attached++;
  return GLOC_OK;
}

// Temporary resident copies of caller-owned host scans (uploaded + indexed), released by the caller.
struct TempScans {
  gloc_scan_store* st;
  std::vector<DevScan> scans;
  explicit TempScans(gloc_scan_store* s) : st(s) {}
  // Scan 0 = the source (launch order for `cs` sources per lane), scans 1.. = targets: uploaded and indexed in ONE
  // launch sequence (round 2: one sequence of ~25 launches per scan, 21 scans for a top-20 registration)
  int add_all(const float* src, size_t n_src, int cs, const float* const* tgt, const size_t* n_tgt, size_t n_tgts,
              bool target_index) {
    std::lock_guard<std::mutex> lk(st->mu);
    std::vector<const float*> p(1 + n_tgts);
    std::vector<size_t> n(1 + n_tgts);
    p[0] = src;
    n[0] = n_src;
    for (size_t c = 0; c < n_tgts; ++c) {
      p[1 + c] = tgt[c];
      n[1 + c] = n_tgt[c];
    }
    scans.resize(1 + n_tgts);
    const int rc = store_make_scans(st, 1 + n_tgts, p.data(), n.data(), 3, false, scans.data());
    if (rc != GLOC_OK) {
      scans.clear();  // (store_make_scans released what it had allocated)
      return rc;
    }
    if (target_index && n_tgts) {
      std::vector<DevScan*> ps(n_tgts);
      for (size_t c = 0; c < n_tgts; ++c) ps[c] = &scans[1 + c];
      GLOC_TRY(store_build_target_indices(st, ps.data(), n_tgts));
    }
    GLOC_TRY(store_build_order(st, scans[0], cs));
    for (size_t c = 0; c < n_tgts; ++c) scans[1 + c].order = nullptr;  // a target's launch order is never read
    return GLOC_OK;
  }
  ~TempScans() {
    std::lock_guard<std::mutex> lk(st->mu);
    for (auto& s : scans) store_free_scan(st, s, true);
  }
};

// Point-to-plane or generalized ICP refinement (p2l.hip, gicp.hip) of the jobs of a call (gn6::Call: one source against n
// targets, or a list of (source, target) pairs): the scans of the call resolved and pinned (CallScans, scan_store.hpp,
// shared with vgicp::run: ids checked before anything is enqueued, targets without normals given them with normal_k and
// with src_normals so is every distinct source), then a searching batch (open_batch) over the longest source -- job table,
// fp32 poses in the CandState array the search reads, corr / d2 as [job][ld(longest source)] -- without a split plan (it is
// solve_kernel that makes one), and `refine` (p2l::run or gicp::run with the method's block) drives the passes through
// launch_nn.  Synchronous: the scans stay pinned for the call.  A row without a target has no source group to search and
// no source slot to sum, and comes out as the row of an empty target.  `refine` is handed every job's target as the
// search indexes it, and through the Ctx its source (normals null without src_normals): DevScan::nrm is in the order of
// idx.pts whatever that order is (curve or kd: scan_store.hpp), the order of the slots corr is indexed by.
struct P2lPass {
  gloc_reg* h;
  BatchDims bd;
  WsView v;
  static int run(void* self, bool warm) {
    P2lPass* p = static_cast<P2lPass*>(self);
    return launch_nn(p->h, p->bd, p->v, warm, false, 0.f);
  }
};

template <class Refine>
int run_refine(gloc_reg* h, const gloc::gn6::Call& call, uint32_t normal_k, bool src_normals, Refine&& refine) {
  hipStream_t s = h->stream;
  const int cs = h->nn_src_per_lane;
  CallScans rs(h->store, s);
  GLOC_TRY(rs.resolve(call, normal_k, src_normals, cs));
  const uint32_t n_jobs = (uint32_t)call.n;
  size_t max_src = 0;
  for (size_t u = 0; u < rs.n_srcs; ++u) max_src = std::max<size_t>(max_src, rs.pins.scans[u].n);
  std::vector<gloc::gn6::Target> tv(n_jobs, gloc::gn6::Target{nullptr, nullptr, 0u, 0u});
  for (uint32_t c = 0; c < n_jobs; ++c)
    if (const DevScan* t = rs.tgt(c)) tv[c] = gloc::gn6::Target{t->idx.pts, t->nrm, (uint32_t)t->n, 0u};
  Batch b;
  GLOC_TRY(open_batch(h, BatchSpec::searching(n_jobs, max_src, src_groups(max_src, cs)), &b, [&](Job* jd, CandState* cst) {
    for (uint32_t c = 0; c < n_jobs; ++c) {
      const DevScan& src = rs.src(c);
      if (const DevScan* t = rs.tgt(c)) {
        jd[c] = Job{src.idx.pts, src.order, src.idx.inv, t->xyz, t->idx, (uint32_t)src.n, src_groups(src.n, cs), c, 0u};
      } else {
        jd[c] = Job{src.idx.pts, src.order, src.idx.inv, nullptr, ScanIndexDev{}, 0u, 0u, c, 0u};
      }
      init_state(cst[c], call.init_T ? call.init_T + 16 * (size_t)c : nullptr);
    }
  }));
  const BatchDims& bd = b.bd;
  P2lPass pass{h, bd, b.v};
  static_assert(sizeof(CandState) % sizeof(float) == 0, "the fp32 poses are a whole number of floats apart");
  gloc::p2l::Ctx x{};
  x.stream = s;
  x.prof = &h->prof;
  x.ws = &h->p2l;
  x.srcs = rs.srcs.data();
  x.n_jobs = n_jobs;
  x.pose_f32 = reinterpret_cast<float*>(h->states.as<char>() + offsetof(CandState, Tf));
  x.pose_stride = sizeof(CandState) / sizeof(float);
  x.corr = pass.v.corr;
  x.d2 = pass.v.d2;
  x.ld = bd.ld;
  x.nn_pass = &P2lPass::run;
  x.self = &pass;
  return refine(x, tv.data());
}

int run_p2l(gloc_reg* h, const gloc::gn6::Call& call, const gloc_p2l_params* prm) {
  return run_refine(h, call, prm->normal_k, false,
                    [&](const gloc::p2l::Ctx& x, const gloc::gn6::Target* tv) { return gloc::p2l::run(x, tv, call, prm); });
}

int run_gicp(gloc_reg* h, const gloc::gn6::Call& call, const gloc_gicp_params* prm) {
  return run_refine(h, call, prm->normal_k, true,
                    [&](const gloc::p2l::Ctx& x, const gloc::gn6::Target* tv) { return gloc::gicp::run(x, tv, call, prm); });
}

// The point-to-point evaluation of a pair list (eval.hip): run_refine's batch without any scan's normals (normal_k 0), the
// ONE cold pass the system form of the loop makes, and the rows' figures from its sums.
int run_eval(gloc_reg* h, const gloc::gn6::Call& call, const gloc_eval_params* prm, const gloc::eval::Out& out) {
  return run_refine(h, call, 0, false,
                    [&](const gloc::p2l::Ctx& x, const gloc::gn6::Target* tv) { return gloc::eval::run(x, tv, call.init_T, prm, out); });
}

// FPFH feature-based global registration (fpfh.hip): the descriptor matches of the source against every target, forward and
// -- mutual -- backward in ONE launch, compacted per job into the pairs layout, and enqueue_ransac on them from the
// identity.  The Job of such a batch carries what the RANSAC kernels read: the pair count as n_src (written on the device
// by the compaction), no src_inv (the sampled ids ARE positions of the list), the stream id.  Synchronous; scans pinned.
__global__ void set_pair_counts_kernel(Job* __restrict__ jobs, const uint32_t* __restrict__ counts, uint32_t n_jobs) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < n_jobs) jobs[c].n_src = counts[c];
}

// What the two stages that turn the match list into a pose differ in, as the shared part below sees it: the features'
// and the matcher's parameters, the hypotheses per job, and whether all of them are scored (the alive lists).
struct FpfhFront {
  Support normal, feature;  // what the scans' normals and features are built from
  uint32_t mutual, n_hyp;
  bool adaptive;
  float min_inlier_ratio;
  const gloc_iss_params* iss = nullptr;  // match the scans' keypoints of these parameters alone (I4); null: every point
  bool ok_from_state = false;            // the stage leaves a verdict of its own in the state's ok, which ok also asks for (R4)
};

// stage(bd, v, nblocks, m_max): the launches from the pairs in v.pairs (M of job c in jobs[c].n_src; none above m_max) to
// the pose in the states -- enqueue_ransac (F4), enqueue_graph (G1 - G4) or enqueue_fgr (R1 - R4).
template <class Stage>
int run_fpfh_pairs(gloc_reg* h, uint32_t src_id, const uint32_t* tgt_ids, size_t n, const uint32_t* stream_ids, const FpfhFront* prm,
                   float* out_T, uint32_t* out_inliers, uint32_t* out_n_pairs, int* out_ok, Stage&& stage) {
  GLOC_REQUIRE(n >= 1 && n <= 4096, GLOC_ERR_INVALID, "n = %zu outside [1, 4096]", n);
  GLOC_REQUIRE(h->store, GLOC_ERR_INVALID, "unknown scan id %u", src_id);
  gloc_scan_store* st = h->store;
  hipStream_t s = h->stream;
  std::vector<uint32_t> ids(1 + n);
  ids[0] = src_id;
  std::copy(tgt_ids, tgt_ids + n, ids.begin() + 1);
  GLOC_TRY(store_ensure_fpfh(st, ids.data(), ids.size(), prm->normal, prm->feature));
  if (prm->iss) GLOC_TRY(store_ensure_keypoints(st, ids.data(), ids.size(), *prm->iss));
  ScopedPins pins(st, s);
  GLOC_TRY(pins.pin(ids.data(), nullptr, ids.size()));
  const std::vector<DevScan>& scans = pins.scans;
  const DevScan& src = scans[0];
  GLOC_REQUIRE(src.n < (1ull << 31), GLOC_ERR_INVALID, "the source scan is too large");
  for (const DevScan& sc : scans) {
    GLOC_REQUIRE(sc.n == 0 || (sc.fpfh && sc.has_fpfh(prm->normal, prm->feature)), GLOC_ERR_STATE, "a scan lost its features during the call");
    GLOC_REQUIRE(!prm->iss || (sc.has_keypoints(*prm->iss) && (sc.kp_n == 0 || (sc.kp && sc.kp_feat))), GLOC_ERR_STATE,
                 "a scan lost its keypoints during the call");
  }
  // On keypoints the searches run in RANK space: the rows are the scans' gathered tables, already in ascending original
  // index, so a row's number is its rank, the smaller rank is the smaller original index (F3's tie rule as it stands), and
  // the compaction turns ranks into points through the keypoint lists.
  const bool on_kp = prm->iss != nullptr;
  auto rows_of = [&](const DevScan& sc) { return on_kp ? sc.kp_n : sc.n; };
  const size_t src_rows = rows_of(src);
  const uint32_t n_jobs = (uint32_t)n;
  const bool mutual = prm->mutual != 0;
  for (uint32_t c = 0; c < n_jobs; ++c) {
    memcpy(out_T + 16 * (size_t)c, I16, sizeof(I16));
    if (out_inliers) out_inliers[c] = 0;
    if (out_n_pairs) out_n_pairs[c] = 0;
    if (out_ok) out_ok[c] = 0;
  }
  if (src_rows < 3) return GLOC_OK;  // fewer than three pairs whatever matches
  GLOC_TRY(ensure_ws(&h->fpfh));
  gloc::fpfh::Ws& w = *h->fpfh;
  // keys: [job][src.n] forward, then each job's backward row of its target's length
  std::vector<size_t> back_off(n_jobs, 0);
  size_t n_keys = (size_t)n_jobs * src_rows;
  for (uint32_t c = 0; c < n_jobs && mutual; ++c) {
    back_off[c] = n_keys;
    n_keys += rows_of(scans[1 + c]);
  }
  GLOC_TRY(w.keys.ensure(sizeof(unsigned long long) * n_keys, s));
  GLOC_HIP(hipMemsetAsync(w.keys.p, 0xFF, sizeof(unsigned long long) * n_keys, s));
  unsigned long long* keys = w.keys.as<unsigned long long>();
  std::vector<gloc::fpfh::MatchTask> tasks;
  std::vector<gloc::fpfh::PairJob> pj(n_jobs);
  for (uint32_t c = 0; c < n_jobs; ++c) {
    const DevScan& t = scans[1 + c];
    unsigned long long* fwd = keys + (size_t)c * src_rows;
    unsigned long long* bwd = mutual ? keys + back_off[c] : nullptr;
    if (on_kp) {
      if (t.kp_n) {
        tasks.push_back(gloc::fpfh::MatchTask{src.kp_feat, nullptr, t.kp_feat, nullptr, fwd, (uint32_t)src.kp_n, (uint32_t)t.kp_n});
        if (mutual) tasks.push_back(gloc::fpfh::MatchTask{t.kp_feat, nullptr, src.kp_feat, nullptr, bwd, (uint32_t)t.kp_n, (uint32_t)src.kp_n});
      }
      pj[c] = gloc::fpfh::PairJob{fwd, bwd, src.xyz, t.xyz, (uint32_t)src.kp_n, (uint32_t)t.kp_n, src.kp, t.kp};
      continue;
    }
    if (t.n) {
      tasks.push_back(gloc::fpfh::MatchTask{src.fpfh, src.idx.pts, t.fpfh, t.idx.pts, fwd, (uint32_t)src.n, (uint32_t)t.n});
      if (mutual) tasks.push_back(gloc::fpfh::MatchTask{t.fpfh, t.idx.pts, src.fpfh, src.idx.pts, bwd, (uint32_t)t.n, (uint32_t)src.n});
    }
    pj[c] = gloc::fpfh::PairJob{fwd, bwd, src.xyz, t.xyz, (uint32_t)src.n, (uint32_t)t.n};
  }
  Batch b;
  GLOC_TRY(open_batch(h, BatchSpec::on_pairs(n_jobs, src_rows, prm->n_hyp, !prm->adaptive), &b, [&](Job* jd, CandState* cst) {
    for (uint32_t c = 0; c < n_jobs; ++c) {
      jd[c] = Job{nullptr, nullptr, nullptr, nullptr, ScanIndexDev{}, 0u, 0u, stream_ids ? stream_ids[c] : c, 0u};
      init_state(cst[c], nullptr, prm->n_hyp);
    }
  }));
  const BatchDims& bd = b.bd;
  const WsView& v = b.v;
  GLOC_TRY(w.counts.ensure(sizeof(uint32_t) * n_jobs, s));
  {
    ProfScope ps(h->prof, "fpfh_match", s);
    GLOC_TRY(gloc::fpfh::match(s, w, tasks));
  }
  {
    ProfScope ps(h->prof, "fpfh_pairs", s);
    GLOC_TRY(gloc::fpfh::pairs(s, w, pj, bd.ld, v.pairs, w.counts.as<uint32_t>()));
  }
  hipLaunchKernelGGL(set_pair_counts_kernel, dim3((n_jobs + 255) / 256), dim3(256), 0, s, v.jobs, w.counts.as<uint32_t>(), n_jobs);
  GLOC_HIP(hipGetLastError());
  // (the compaction has been waited for: the counts come down here, where the graph stage sizes its workspace by them)
  std::vector<uint32_t> counts(n_jobs);
  GLOC_HIP(hipMemcpyAsync(counts.data(), w.counts.p, sizeof(uint32_t) * n_jobs, hipMemcpyDeviceToHost, s));
  GLOC_HIP(hipStreamSynchronize(s));
  const uint32_t m_max = *std::max_element(counts.begin(), counts.end());
  GLOC_TRY(stage(bd, v, b.nblocks, m_max));
  GLOC_HIP(hipMemcpyAsync(h->h_states, h->states.p, sizeof(CandState) * n_jobs, hipMemcpyDeviceToHost, s));
  GLOC_HIP(hipStreamSynchronize(s));
  for (uint32_t c = 0; c < n_jobs; ++c) {
    const CandState& cs = h->h_states[c];
    const uint32_t M = counts[c];
    bool found, ok;
    pair_verdict(cs, M, prm->min_inlier_ratio, &found, &ok);
    if (prm->ok_from_state) ok = ok && cs.ok != 0;
    pose_to_T16(cs, out_T + 16 * (size_t)c);
    if (out_n_pairs) out_n_pairs[c] = M;
    if (out_inliers) out_inliers[c] = found ? cs.best_inl : 0u;
    if (out_ok) out_ok[c] = ok;
  }
  return GLOC_OK;
}

int run_fpfh(gloc_reg* h, uint32_t src_id, const uint32_t* tgt_ids, size_t n, const uint32_t* stream_ids, const gloc_fpfh_params* prm,
             const Support& normal, const Support& feature, float* out_T, uint32_t* out_inliers, uint32_t* out_n_pairs, int* out_ok,
             const gloc_iss_params* iss = nullptr) {
  const FpfhFront f{normal, feature, prm->mutual, prm->ransac_iters, prm->ransac_confidence > 0.f && prm->ransac_confidence < 1.f,
                    prm->min_inlier_ratio, iss};
  return run_fpfh_pairs(h, src_id, tgt_ids, n, stream_ids, &f, out_T, out_inliers, out_n_pairs, out_ok,
                        [&](const BatchDims& bd, const WsView& v, uint32_t nblocks, uint32_t) {
                          return enqueue_ransac(h, bd, RansacRule{prm->ransac_iters, prm->inlier_thresh, prm->min_inlier_ratio,
                                                                  prm->ransac_confidence, prm->seed}, v, nblocks);
                        });
}

// The fit of a consensus set from its raw moments (pairgraph.hip): one thread per (job, seed); centroids and covariance as
// solve_compose forms them for the refit, kabsch_from_cov, the hypothesis rounded to fp32 as ransac_hyp_kernel leaves its own.
__global__ void graph_solve_kernel(const double* __restrict__ moments, const uint32_t* __restrict__ valid, float* __restrict__ Rt, uint32_t count) {
  const uint32_t o = blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= count || !valid[o]) return;
  const double* v = moments + (size_t)o * gloc::pairgraph::MOMENTS;
  const double cnt = v[0], inv = 1.0 / cnt;
  double pbar[3], qbar[3], M[9], Rd[9], td[3];
  for (int a = 0; a < 3; ++a) {
    pbar[a] = v[1 + a] * inv;
    qbar[a] = v[4 + a] * inv;
  }
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) M[3 * a + b] = v[7 + 3 * a + b] - cnt * (pbar[a] * qbar[b]);
  kabsch_from_cov(M, pbar, qbar, Rd, td);
  float* out = Rt + (size_t)o * 12;
  for (int i = 0; i < 9; ++i) out[i] = (float)Rd[i];
  for (int i = 0; i < 3; ++i) out[9 + i] = (float)td[i];
}

// Correspondence-graph global registration (pairgraph.hip): G1 - G3 make n_seeds hypotheses per job in the RANSAC stage's
// Rt / valid layout; G4 is that stage's own kernels, unchanged: ransac_score_kernel counts the inliers of all of them,
// ransac_scan_kernel's sequential rule without the adaptive stop IS "the most inliers, then the smaller rank", and
// accum_kernel<1> / solve_kernel<1> refit on the winner's inliers.  The states start as init_state(.., n_seeds) leaves them.
int enqueue_graph(gloc_reg* h, const BatchDims& bd, const gloc_fpfh_graph_params* prm, const WsView& v, const uint32_t* counts, uint32_t nblocks,
                  uint32_t m_max) {
  const uint32_t n_jobs = v.n_jobs, S = prm->n_seeds;
  hipStream_t s = v.s;
  GLOC_TRY(ensure_ws(&h->pgraph));
  GLOC_TRY(gloc::pairgraph::consensus_sets(s, h->prof, *h->pgraph, gloc::pairgraph::Batch{v.pairs, bd.ld, counts, n_jobs, m_max}, *prm,
                                           h->pgraph_budget, v.valid));
  if (m_max) {
    ProfScope ps(h->prof, "pg_fit", s);
    hipLaunchKernelGGL(graph_solve_kernel, dim3((S * n_jobs + 63) / 64), dim3(64), 0, s, h->pgraph->moments.as<double>(), v.valid, v.Rt, S * n_jobs);
    GLOC_HIP(hipGetLastError());
  }
  GLOC_HIP(hipMemsetAsync(v.inliers, 0, sizeof(uint32_t) * (size_t)S * n_jobs, s));
  const float thr2 = prm->inlier_thresh * prm->inlier_thresh;
  {
    ProfScope ps(h->prof, "ransac_score", s);
    const uint32_t chunk_len = score_chunk_len(n_jobs, bd.max_src), hpb = score_hpb(S);
    const unsigned cchunks = (std::max<uint32_t>(m_max, 1u) + chunk_len - 1) / chunk_len;
    hipLaunchKernelGGL(ransac_score_kernel, dim3((S + hpb - 1) / hpb, cchunks, n_jobs), dim3(256), 0, s, v.pairs, bd.ld, v.jobs, S, 0u, hpb, v.Rt,
                       v.valid, thr2, (const CandState*)nullptr, v.inliers, (const uint32_t*)nullptr, (const uint32_t*)nullptr, 0u, chunk_len,
                       (unsigned long long*)nullptr);
    hipLaunchKernelGGL(ransac_scan_kernel<true>, dim3(n_jobs), dim3(64), 0, s, v.inliers, v.valid, v.Rt, S, 0u, S, v.jobs, 0.f,
                       prm->min_inlier_ratio, v.states);
    GLOC_HIP(hipGetLastError());
  }
  return enqueue_refit(h, bd, v, thr2, nblocks);  // (a batch on pairs has no split plan: one solve block per job)
}

int run_fpfh_graph(gloc_reg* h, uint32_t src_id, const uint32_t* tgt_ids, size_t n, const gloc_fpfh_graph_params* prm,
                   const Support& normal, const Support& feature, float* out_T, uint32_t* out_inliers, uint32_t* out_n_pairs, int* out_ok,
                   const gloc_iss_params* iss = nullptr) {
  const FpfhFront f{normal, feature, prm->mutual, prm->n_seeds, true, prm->min_inlier_ratio, iss};
  return run_fpfh_pairs(h, src_id, tgt_ids, n, nullptr, &f, out_T, out_inliers, out_n_pairs, out_ok,
                        [&](const BatchDims& bd, const WsView& v, uint32_t nblocks, uint32_t m_max) {
                          return enqueue_graph(h, bd, prm, v, h->fpfh->counts.as<uint32_t>(), nblocks, m_max);
                        });
}

// gloc_reg_pair_graph: one job on a host list, every diagnostic brought down.
int run_pair_graph(gloc_reg* h, const float* P, const float* Q, size_t m, const gloc_fpfh_graph_params* prm, uint32_t* out_degree,
                   uint64_t* out_score, uint32_t* out_seeds, uint32_t* out_set_sizes, uint32_t* out_seed_inliers, float* out_T,
                   uint32_t* out_inliers, uint32_t* out_winner_rank, int* out_ok) {
  const uint32_t S = prm->n_seeds, M = (uint32_t)m;
  if (out_T) memcpy(out_T, I16, sizeof(I16));
  if (out_inliers) *out_inliers = 0;
  if (out_winner_rank) *out_winner_rank = 0xFFFFFFFFu;
  if (out_ok) *out_ok = 0;
  for (uint32_t r = 0; r < S; ++r) {
    if (out_seeds) out_seeds[r] = 0xFFFFFFFFu;
    if (out_set_sizes) out_set_sizes[r] = 0;
    if (out_seed_inliers) out_seed_inliers[r] = 0;
  }
  if (M == 0) return GLOC_OK;
  hipStream_t s = h->stream;
  Batch b;
  GLOC_TRY(open_batch(h, BatchSpec::on_pairs(1, M, S, false), &b, [&](Job* jd, CandState* cst) {
    jd[0] = Job{nullptr, nullptr, nullptr, nullptr, ScanIndexDev{}, M, 0u, 0u, 0u};
    init_state(cst[0], nullptr, S);
  }));
  const WsView& v = b.v;
  const std::vector<float> hp = pack_pairs(P, Q, nullptr, m, b.bd.ld);
  GLOC_HIP(hipMemcpyAsync(v.pairs, hp.data(), sizeof(float) * hp.size(), hipMemcpyHostToDevice, s));
  GLOC_TRY(ensure_ws(&h->pgraph));
  GLOC_TRY(h->pgraph->counts.ensure(sizeof(uint32_t), s));
  GLOC_HIP(hipMemcpyAsync(h->pgraph->counts.p, &h->h_jobs[0].n_src, sizeof(uint32_t), hipMemcpyHostToDevice, s));
  GLOC_TRY(enqueue_graph(h, b.bd, prm, v, h->pgraph->counts.as<uint32_t>(), b.nblocks, M));
  const gloc::pairgraph::Ws& w = *h->pgraph;
  GLOC_HIP(hipMemcpyAsync(h->h_states, h->states.p, sizeof(CandState), hipMemcpyDeviceToHost, s));
  if (out_degree) GLOC_HIP(hipMemcpyAsync(out_degree, w.degree.p, sizeof(uint32_t) * m, hipMemcpyDeviceToHost, s));
  if (out_score) GLOC_HIP(hipMemcpyAsync(out_score, w.score.p, sizeof(uint64_t) * m, hipMemcpyDeviceToHost, s));
  if (out_seeds) GLOC_HIP(hipMemcpyAsync(out_seeds, w.seeds.p, sizeof(uint32_t) * S, hipMemcpyDeviceToHost, s));
  if (out_set_sizes) GLOC_HIP(hipMemcpyAsync(out_set_sizes, w.set_sizes.p, sizeof(uint32_t) * S, hipMemcpyDeviceToHost, s));
  if (out_seed_inliers) GLOC_HIP(hipMemcpyAsync(out_seed_inliers, v.inliers, sizeof(uint32_t) * S, hipMemcpyDeviceToHost, s));
  GLOC_HIP(hipStreamSynchronize(s));  // (hp, too, is done with)
  const CandState& cs = h->h_states[0];
  bool found, ok;
  pair_verdict(cs, M, prm->min_inlier_ratio, &found, &ok);
  if (out_T) pose_to_T16(cs, out_T);
  if (out_inliers) *out_inliers = found ? cs.best_inl : 0u;
  if (out_winner_rank) *out_winner_rank = found ? cs.best_h : 0xFFFFFFFFu;
  if (out_ok) *out_ok = ok;
  return GLOC_OK;
}

// Fast Global Registration (fgr.hip): R1 - R4 on the pairs in v.pairs.  The stage has its own job table (the list's length
// and the sample stream, taken from the batch's on the device) and its own results, which fgr_state_kernel turns into
// what the shared part reads from the states: the fp32 pose, best_h = 0 once an update has completed (else none: the
// identity and 0 inliers), the inliers, and ok = (status 0).
__global__ void fgr_jobs_kernel(const Job* __restrict__ jobs, uint32_t n_jobs, gloc::fgr::JobIn* __restrict__ out) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < n_jobs) out[c] = gloc::fgr::JobIn{jobs[c].n_src, jobs[c].cand_id};
}

__global__ void fgr_state_kernel(const gloc::fgr::Result* __restrict__ res, uint32_t n_jobs, CandState* __restrict__ states) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n_jobs) return;
  const gloc::fgr::Result& r = res[c];
  CandState& st = states[c];
  if (r.updates) {
    for (int k = 0; k < 12; ++k) {
      st.Td[k] = r.Td[k];
      st.Tf[k] = r.Tf[k];
    }
    st.best_h = 0u;
    st.best_inl = r.inliers;
  }
  st.ok = r.status == 0 ? 1 : 0;
}

int enqueue_fgr(gloc_reg* h, const BatchDims& bd, const gloc_fgr_params* prm, const WsView& v, uint32_t m_max) {
  const uint32_t n_jobs = v.n_jobs;
  hipStream_t s = v.s;
  GLOC_TRY(ensure_ws(&h->fgr));
  gloc::fgr::Ws& w = *h->fgr;
  GLOC_TRY(w.jobs.ensure(sizeof(gloc::fgr::JobIn) * n_jobs, s));
  hipLaunchKernelGGL(fgr_jobs_kernel, dim3((n_jobs + 255) / 256), dim3(256), 0, s, v.jobs, n_jobs, w.jobs.as<gloc::fgr::JobIn>());
  GLOC_HIP(hipGetLastError());
  GLOC_TRY(gloc::fgr::enqueue(s, h->prof, w, gloc::fgr::Batch{v.pairs, bd.ld, n_jobs, m_max}, *prm));
  hipLaunchKernelGGL(fgr_state_kernel, dim3((n_jobs + 255) / 256), dim3(256), 0, s, w.results.as<gloc::fgr::Result>(), n_jobs, v.states);
  GLOC_HIP(hipGetLastError());
  return GLOC_OK;
}

int run_fpfh_fgr(gloc_reg* h, uint32_t src_id, const uint32_t* tgt_ids, size_t n, const uint32_t* stream_ids, const gloc_fgr_params* prm,
                 const Support& normal, const Support& feature, float* out_T, uint32_t* out_inliers, uint32_t* out_n_pairs, int* out_ok,
                 const gloc_iss_params* iss = nullptr) {
  const FpfhFront f{normal, feature, prm->mutual, 1u, true, prm->min_inlier_ratio, iss, true};
  return run_fpfh_pairs(h, src_id, tgt_ids, n, stream_ids, &f, out_T, out_inliers, out_n_pairs, out_ok,
                        [&](const BatchDims& bd, const WsView& v, uint32_t, uint32_t m_max) { return enqueue_fgr(h, bd, prm, v, m_max); });
}

// gloc_reg_fgr_pairs: one job on a host list, every diagnostic brought down.
int run_fgr_pairs(gloc_reg* h, const float* P, const float* Q, size_t m, uint32_t stream_id, const gloc_fgr_params* prm, uint32_t* out_mult,
                  uint32_t* out_n_tuples, double* out_d2, double* out_system, float* out_T, uint32_t* out_inliers, int* out_status,
                  int* out_ok) {
  const uint32_t M = (uint32_t)m;
  memcpy(out_T, I16, sizeof(I16));
  if (out_n_tuples) *out_n_tuples = 0;
  if (out_d2) *out_d2 = 0.0;
  if (out_system) std::fill(out_system, out_system + gloc::fgr::NSYS, 0.0);
  if (out_inliers) *out_inliers = 0;
  if (out_status) *out_status = 2;
  if (out_ok) *out_ok = 0;
  if (out_mult) std::fill(out_mult, out_mult + m, 0u);
  if (M == 0) return GLOC_OK;
  hipStream_t s = h->stream;
  Batch b;
  GLOC_TRY(open_batch(h, BatchSpec::on_pairs(1, M, 1, false), &b, [&](Job* jd, CandState* cst) {
    jd[0] = Job{nullptr, nullptr, nullptr, nullptr, ScanIndexDev{}, M, 0u, stream_id, 0u};
    init_state(cst[0], nullptr, 1);
  }));
  const WsView& v = b.v;
  const std::vector<float> hp = pack_pairs(P, Q, nullptr, m, b.bd.ld);
  GLOC_HIP(hipMemcpyAsync(v.pairs, hp.data(), sizeof(float) * hp.size(), hipMemcpyHostToDevice, s));
  GLOC_TRY(enqueue_fgr(h, b.bd, prm, v, M));
  const gloc::fgr::Ws& w = *h->fgr;
  gloc::fgr::Result res;
  GLOC_HIP(hipMemcpyAsync(h->h_states, h->states.p, sizeof(CandState), hipMemcpyDeviceToHost, s));
  GLOC_HIP(hipMemcpyAsync(&res, w.results.p, sizeof(res), hipMemcpyDeviceToHost, s));
  if (out_mult) GLOC_HIP(hipMemcpyAsync(out_mult, w.mult.p, sizeof(uint32_t) * m, hipMemcpyDeviceToHost, s));
  GLOC_HIP(hipStreamSynchronize(s));  // (hp, too, is done with)
  const CandState& cs = h->h_states[0];
  bool found, ok;
  pair_verdict(cs, M, prm->min_inlier_ratio, &found, &ok);
  pose_to_T16(cs, out_T);
  if (out_n_tuples) *out_n_tuples = res.n_tuples;
  if (out_d2) *out_d2 = res.d2;
  if (out_system) std::copy(res.system, res.system + gloc::fgr::NSYS, out_system);
  if (out_inliers) *out_inliers = found ? cs.best_inl : 0u;
  if (out_status) *out_status = res.status;
  if (out_ok) *out_ok = ok && cs.ok != 0;
  return GLOC_OK;
}

gloc::ndt::Ctx ndt_ctx(gloc_reg* h) { return gloc::ndt::Ctx{h->store, h->stream, &h->prof, &h->ndt}; }
gloc::vgicp::Ctx vgicp_ctx(gloc_reg* h) { return gloc::vgicp::Ctx{h->store, h->stream, &h->prof, &h->vgicp, &h->p2l}; }

// Voxelized generalized ICP (vgicp.hip): no 1-NN search, so none of this file's batch set-up -- the call builds its
// targets' voxel maps and runs the shared loop of passes on the handle's stream.
int run_vgicp(gloc_reg* h, const gloc::gn6::Call& call, const gloc_vgicp_params* prm) { return gloc::vgicp::run(vgicp_ctx(h), call, prm); }

// ... and against the handle's resident voxel maps (vmap.hip): call.tgt_ids are map ids, no map is built.
gloc::vmap::Ctx vmap_ctx(gloc_reg* h) { return gloc::vmap::Ctx{h->store, h->stream, &h->prof, &h->vmaps}; }
int run_vgicp_vmap(gloc_reg* h, const gloc::gn6::Call& call, const gloc_vgicp_params* prm) {
  return gloc::vmap::refine(vmap_ctx(h), vgicp_ctx(h), call, prm);
}

// What the map entries that are no refinement start with: the handle, a batch in flight, the map's id -- before any
// device work.
int vmap_entry(gloc_reg* h, uint32_t map_id) {
  GLOC_REQUIRE(h, GLOC_ERR_INVALID, "null argument");
  GLOC_NOT_PENDING(h);
  GLOC_TRY(gloc::vmap::check_id(vmap_ctx(h), map_id));
  GLOC_HIP(hipSetDevice(h->device));
  return GLOC_OK;
}

// The two shapes of a Gauss-Newton refinement call (gn6::Call, p2l.hpp) as the C entries fill them; an entry with a robust
// block sets the robust half behind it.
gloc::gn6::Call batch_call(const uint32_t* src_ids, bool pairs, const uint32_t* tgt_ids, size_t n, const float* init_T, float* out_T,
                           float* out_rmse, uint32_t* out_iters, int* out_status) {
  gloc::gn6::Call c;
  c.src_ids = src_ids;
  c.pairs = pairs;
  c.tgt_ids = tgt_ids;
  c.n = n;
  c.init_T = init_T;
  c.out_T = out_T;
  c.out_rmse = out_rmse;
  c.out_iters = out_iters;
  c.out_status = out_status;
  return c;
}

gloc::gn6::Call system_call(const uint32_t* src_id, const uint32_t* tgt_id, const float* T16, double* out_H36, double* out_g6, double* out_sum,
                            uint64_t* out_count) {
  gloc::gn6::Call c;
  c.src_ids = src_id;
  c.tgt_ids = tgt_id;
  c.n = 1;
  c.init_T = T16;
  c.system = true;
  c.out_H36 = out_H36;
  c.out_g6 = out_g6;
  c.out_sum = out_sum;
  c.out_count = out_count;
  return c;
}

// The system form over a pair list: every row evaluated once at init_T + 16 c.  robust null: the plain step.
gloc::gn6::Call pairs_system_call(const uint32_t* src_ids, const uint32_t* tgt_ids, size_t n, const float* T, const gloc_robust_params* robust,
                                  uint32_t pass, double* out_H36, double* out_g6, double* out_sum, uint64_t* out_count, double* out_wsum) {
  gloc::gn6::Call c = system_call(src_ids, tgt_ids, T, out_H36, out_g6, out_sum, out_count);
  c.pairs = true;
  c.n = n;
  c.robust = robust;
  c.pass = pass;
  c.out_wsum = out_wsum;
  return c;
}

gloc::gn6::Call robust_call(gloc::gn6::Call c, const gloc_robust_params* robust, uint32_t pass, float* out_weight, double* out_wsum) {
  c.robust = robust;
  c.need_robust = true;
  c.pass = pass;
  c.out_weight = out_weight;
  c.out_wsum = out_wsum;
  return c;
}

// What every entry of the three refinements does with its call, and the ONE order of its refusals: the method's own
// block, the robust block (a null one only where the entry has to have one), the arrays and n, the handle, a batch in
// flight -- and then the method's run.
template <class Params>
int refine_entry(gloc_reg* h, const gloc::gn6::Call& c, const Params* prm, int (*check)(const Params*),
                 int (*run)(gloc_reg*, const gloc::gn6::Call&, const Params*)) {
  GLOC_TRY(check(prm));
  if (c.robust || c.need_robust) GLOC_TRY(gloc::robust::check_params(c.robust));
  if (c.system) {
    GLOC_REQUIRE(!c.pairs || (c.src_ids && c.tgt_ids), GLOC_ERR_INVALID, "null scan ids");
    GLOC_REQUIRE(c.out_H36 && c.out_g6 && c.out_sum && c.out_count && (c.out_wsum || !c.need_robust), GLOC_ERR_INVALID, "null argument");
  } else if (c.pairs) {
    GLOC_REQUIRE(c.src_ids && c.tgt_ids, GLOC_ERR_INVALID, "null scan ids");
    GLOC_REQUIRE(c.out_T, GLOC_ERR_INVALID, "out_T is null");
  } else {
    GLOC_REQUIRE(c.out_T && c.tgt_ids, GLOC_ERR_INVALID, "null argument");
  }
  GLOC_REQUIRE(c.n >= 1 && c.n <= 4096, GLOC_ERR_INVALID, "n = %zu outside [1, 4096]", c.n);
  GLOC_REQUIRE(h, GLOC_ERR_INVALID, "null argument");
  GLOC_NOT_PENDING(h);
  GLOC_HIP(hipSetDevice(h->device));
  return run(h, c, prm);
}

}  // namespace

extern "C" {

void gloc_reg_default_params(gloc_reg_params* p) {
  if (!p) return;
  p->ransac_iters = 3000;   // registration/loop_detector.cpp:257
  p->inlier_thresh = 0.6f;  // 3 * 0.2 m: loop_detector.cpp:257, loop_detector.h:116
  p->min_inlier_ratio = 0.3f;
  p->icp_iters = 30;  // registration/global_registration.cpp:242
  p->max_corr_dist = 0.f;
  p->seed = 1234;
  p->ransac_confidence = 0.99f;  // cv::estimateAffinePartial2D's default, used by the reference
  p->max_rmse = 0.f;
  p->max_final_step = 0.f;  // off, as the reference: its 3-D stage takes what the ICP returns (GLOC_REG_FINAL_STEP_SUGGESTED: see the header)
}

int gloc_reg_create(int device, gloc_reg** out) {
  GLOC_TRY(create_handle(device, out));
  gloc_reg* h = *out;
  hipError_t e = hipEventCreateWithFlags(&h->done_ev, hipEventDisableTiming);
  if (e != hipSuccess) {
    set_err("hipEventCreate failed: %s", hipGetErrorString(e));
    *out = nullptr;
    delete h;
    return GLOC_ERR_HIP;
  }
  return GLOC_OK;
}

int gloc_reg_attach_store(gloc_reg* h, gloc_scan_store* store) {
  GLOC_REQUIRE(h, GLOC_ERR_INVALID, "null handle");
  GLOC_REQUIRE(!store || store->device == h->device, GLOC_ERR_INVALID, "store lives on device %d, the handle on %d",
               store ? store->device : -1, h->device);
  GLOC_HIP(hipSetDevice(h->device));
  GLOC_HIP(hipStreamSynchronize(h->stream));
  if (h->store) h->store->attached--;
  h->store = store ? store : h->own_store;
  if (h->store) h->store->attached++;
  return GLOC_OK;
}

int gloc_reg_scan_clear(gloc_reg* h) {
  GLOC_REQUIRE(h, GLOC_ERR_INVALID, "null handle");
  GLOC_HIP(hipSetDevice(h->device));
  GLOC_HIP(hipStreamSynchronize(h->stream));
  if (!h->store) return GLOC_OK;
  return gloc_scan_store_clear(h->store);
}

int gloc_reg_destroy(gloc_reg* h) { return destroy_handle(h); }

int gloc_reg_set_stream(gloc_reg* h, void* hip_stream) { return handle_set_stream(h, hip_stream); }

int gloc_reg_synchronize(gloc_reg* h) { return handle_synchronize(h); }

int gloc_reg_set_option(gloc_reg* h, int option, int64_t value) {
  GLOC_REQUIRE(h, GLOC_ERR_INVALID, "null handle");
  if (option == GLOC_REG_OPT_PROFILE) {
    h->prof.enabled = value != 0;
    return GLOC_OK;
  }
  if (option == GLOC_REG_OPT_NN_MODE) {
    GLOC_REQUIRE(value == GLOC_REG_NN_CULLED || value == GLOC_REG_NN_EXHAUSTIVE, GLOC_ERR_INVALID,
                 "bad nn mode %lld", (long long)value);
    h->nn_mode = (int)value;
    return GLOC_OK;
  }
  if (option == GLOC_REG_OPT_NN_JOB_GROUP) {
    GLOC_REQUIRE(value >= 1 && value <= 65536, GLOC_ERR_INVALID, "must be in [1, 65536]");
    h->nn_job_group = (int)value;
    h->nn_job_group_set = true;
    return GLOC_OK;
  }
  if (option == GLOC_REG_OPT_TEMP_TARGET_INDEX) {
    h->temp_target_index = value != 0;
    return GLOC_OK;
  }
  if (option == GLOC_REG_OPT_NN_SUB_JOBS) {
    GLOC_REQUIRE(value >= 0 && value <= 64, GLOC_ERR_INVALID, "must be in [0, 64]");
    h->nn_sub_jobs = (int)value;
    return GLOC_OK;
  }
  if (option == GLOC_REG_OPT_NN_SPLIT_HELPERS) {
    GLOC_REQUIRE(value >= -1 && value <= 4096, GLOC_ERR_INVALID, "must be in [-1, 4096]");
    h->nn_split_helpers = (int)value;
    return GLOC_OK;
  }
  if (option == GLOC_REG_OPT_SUB_BATCHES) {
    GLOC_REQUIRE(value >= -1 && value <= 8, GLOC_ERR_INVALID, "must be in [-1, 8]");
    return GLOC_OK;  // (accepted for existing callers; a batch is always enqueued on the handle's stream)
  }
  if (option == GLOC_REG_OPT_NN_CHAIN) {
    GLOC_REQUIRE(value == 0 || value == 1, GLOC_ERR_INVALID, "must be 0 or 1");
    h->nn_chain = (int)value;
    if (value) h->chain_broken = false;
    return GLOC_OK;
  }
  if (option == GLOC_REG_OPT_NN_HEAVY_THRESH) {
    GLOC_REQUIRE(value >= 0 && value <= 65535, GLOC_ERR_INVALID, "must be in [0, 65535]");
    h->nn_heavy_thresh = (int)value;
    return GLOC_OK;
  }
  if (option == GLOC_REG_OPT_NN_SPLIT_THRESH) {
    GLOC_REQUIRE(value >= 0 && value <= 0x3FFFFFFF, GLOC_ERR_INVALID, "must be in [0, 2^30)");
    h->nn_split_thresh = (uint32_t)value;
    h->nn_split_thresh_set = true;
    return GLOC_OK;
  }
  if (option == GLOC_REG_OPT_NN_SRC_PER_LANE) {
    GLOC_REQUIRE(value == 1 || value == 2 || value == 4, GLOC_ERR_INVALID, "must be 1, 2 or 4");
    h->nn_src_per_lane = (int)value;
    return GLOC_OK;
  }
  if (option == GLOC_REG_OPT_PAIRGRAPH_BUDGET) {
    GLOC_REQUIRE(value >= 0 && (uint64_t)value <= gloc::pairgraph::BUDGET_BYTES, GLOC_ERR_INVALID, "must be in [0, 2^30]");
    h->pgraph_budget = (size_t)value;
    return GLOC_OK;
  }
  set_err("unknown option %d", option);
  return GLOC_ERR_INVALID;
}

int gloc_reg_scan_upload(gloc_reg* h, const float* pts, size_t n, size_t stride_floats,
                         uint32_t* scan_id) {
  GLOC_REQUIRE(h, GLOC_ERR_INVALID, "null handle");
  GLOC_HIP(hipSetDevice(h->device));
  GLOC_TRY(ensure_store(h));
  return gloc_scan_store_add(h->store, pts, n, stride_floats, scan_id);
}

int gloc_reg_scan_add_submaps(gloc_reg* h, const uint32_t* member_ids, const float* member_T, const uint32_t* first, size_t count,
                              const gloc_submap_params* prm, uint32_t* new_ids, gloc_submap_info* info) {
  GLOC_REQUIRE(h, GLOC_ERR_INVALID, "null handle");
  GLOC_REQUIRE(h->store, GLOC_ERR_INVALID, "no scan store: upload the member scans or attach a store first");
  GLOC_HIP(hipSetDevice(h->device));
  return gloc_scan_store_add_submaps(h->store, member_ids, member_T, first, count, prm, new_ids, info);
}

int gloc_reg_scan_build_target_index(gloc_reg* h, uint32_t scan_id) {
  GLOC_REQUIRE(h, GLOC_ERR_INVALID, "null handle");
  GLOC_REQUIRE(h->store, GLOC_ERR_INVALID, "unknown scan id %u", scan_id);
  GLOC_HIP(hipSetDevice(h->device));
  GLOC_HIP(hipStreamSynchronize(h->stream));  // no launch of this handle may still read the scan
  return gloc_scan_store_build_target_index(h->store, scan_id);
}

int gloc_reg_scan_release(gloc_reg* h, uint32_t scan_id) {
  GLOC_REQUIRE(h, GLOC_ERR_INVALID, "null handle");
  GLOC_REQUIRE(h->store, GLOC_ERR_INVALID, "unknown scan id %u", scan_id);
  GLOC_HIP(hipSetDevice(h->device));
  GLOC_HIP(hipStreamSynchronize(h->stream));  // no launch of this handle may still read the scan
  return gloc_scan_store_release(h->store, scan_id);
}

int gloc_reg_scan_count(const gloc_reg* h, size_t* n_scans) {
  GLOC_REQUIRE(h && n_scans, GLOC_ERR_INVALID, "null argument");
  *n_scans = 0;
  if (!h->store) return GLOC_OK;
  return gloc_scan_store_count(h->store, n_scans);
}

int gloc_reg_batch(gloc_reg* h, const float* q_xyz, size_t nq_pts, const float* const* cand_xyz,
                   const size_t* cand_npts, size_t n_cand, const uint32_t* cand_stream_ids,
                   const float* init_T, const gloc_reg_params* params, float* out_T,
                   float* out_rmse, uint32_t* out_inliers, int* out_ok) {
  GLOC_REQUIRE(h && out_T && (q_xyz || nq_pts == 0), GLOC_ERR_INVALID, "null argument");
  GLOC_REQUIRE(n_cand >= 1 && n_cand <= 4096 && cand_xyz && cand_npts, GLOC_ERR_INVALID,
               "n_cand = %zu outside [1,4096] or null candidate arrays", n_cand);
  GLOC_REQUIRE(nq_pts < (1ull << 31), GLOC_ERR_INVALID, "query scan too large");
  GLOC_NOT_PENDING(h);
  GLOC_TRY(check_params(params));
  GLOC_HIP(hipSetDevice(h->device));
  for (size_t c = 0; c < n_cand; ++c) {
    GLOC_REQUIRE(cand_xyz[c] || cand_npts[c] == 0, GLOC_ERR_INVALID, "candidate %zu is null", c);
    GLOC_REQUIRE(cand_npts[c] < (1ull << 31), GLOC_ERR_INVALID, "candidate scan too large");
  }
  GLOC_TRY(ensure_store(h));
  TempScans tmp(h->store);  // released on return
  GLOC_TRY(tmp.add_all(q_xyz, nq_pts, h->nn_src_per_lane, cand_xyz, cand_npts, n_cand, h->temp_target_index));
  std::vector<JobHost> jh(n_cand);
  for (size_t c = 0; c < n_cand; ++c)
    jh[c] = JobHost{tmp.scans[0], tmp.scans[c + 1], cand_stream_ids ? cand_stream_ids[c] : (uint32_t)c,
                    init_T ? init_T + 16 * c : nullptr};
  int rc = run_jobs(h, jh, params, out_T, out_rmse, out_inliers, out_ok);
  (void)hipStreamSynchronize(h->stream);
  return rc;
}

int gloc_reg_batch_multi_begin(gloc_reg* h, size_t n_queries, const uint32_t* q_scan_ids, const uint32_t* cand_scan_ids,
                               size_t n_cand, const uint32_t* cand_stream_ids, const float* init_T,
                               const gloc_reg_params* params) {
  GLOC_REQUIRE(h && q_scan_ids && cand_scan_ids, GLOC_ERR_INVALID, "null argument");
  GLOC_REQUIRE(n_queries >= 1 && n_cand >= 1 && n_queries * n_cand <= 65536, GLOC_ERR_INVALID,
               "n_queries x n_cand = %zu x %zu outside [1, 65536]", n_queries, n_cand);
  GLOC_REQUIRE(h->store, GLOC_ERR_INVALID, "no scan store: upload scans or attach a store first");
  GLOC_REQUIRE(!h->pending.active, GLOC_ERR_STATE, "a batch is already in flight on this handle: call gloc_reg_batch_multi_end first");
  GLOC_TRY(check_params(params));
  GLOC_HIP(hipSetDevice(h->device));
  const size_t total = n_queries * n_cand;
  std::vector<JobHost> jh;
  gloc_reg::Pending& P = h->pending;
  P.slot.clear();
  P.n_src.clear();
  // The scans the jobs read: views and pins in ONE step under the store's mutex, BEFORE anything is launched
  // (gloc_scan_store_build_target_index refuses to re-sort them in place and gloc_scan_store_release to free them until
  // _end); released again if the enqueue fails part-way -- whatever was launched is waited for first.
  P.pinned.assign(q_scan_ids, q_scan_ids + n_queries);
  std::vector<int> cs_of(n_queries, h->nn_src_per_lane);
  for (size_t o = 0; o < total; ++o)
    if (cand_scan_ids[o] != 0xFFFFFFFFu) {  // (0xFFFFFFFF: "no candidate", a retrieval list shorter than k)
      P.pinned.push_back(cand_scan_ids[o]);
      cs_of.push_back(0);  // a target's launch order is never read
    }
  std::vector<DevScan> view(P.pinned.size());
  {
    const int rc = store_get_pinned(h->store, P.pinned.data(), cs_of.data(), P.pinned.size(), view.data());
    if (rc != GLOC_OK) {
      P.pinned.clear();
      return rc;
    }
  }
  jh.reserve(total);
  size_t vi = n_queries;
  for (size_t q = 0; q < n_queries; ++q) {
    const DevScan& src = view[q];
    for (size_t c = 0; c < n_cand; ++c) {
      const size_t o = q * n_cand + c;
      if (cand_scan_ids[o] == 0xFFFFFFFFu) continue;
      JobHost j;
      j.src = src;
      j.tgt = view[vi++];
      j.stream_id = cand_stream_ids ? cand_stream_ids[o] : (uint32_t)c;
      j.init_T = init_T ? init_T + 16 * o : nullptr;
      jh.push_back(j);
      P.slot.push_back(o);
      P.n_src.push_back(src.n);
    }
  }
  // rows without a candidate keep the initial guess (identity), not ok
  P.def_T.resize(16 * total);
  for (size_t o = 0; o < total; ++o)
    std::copy_n(init_T ? init_T + 16 * o : I16, 16, P.def_T.begin() + 16 * o);
  P.total = total;
  P.max_rmse = params->max_rmse;
  P.max_final_step = params->icp_iters ? params->max_final_step : 0.f;
  const int rc = enqueue_jobs(h, jh, params);
  if (rc != GLOC_OK) {
    (void)hipStreamSynchronize(h->stream);
    store_pin(h->store, P.pinned.data(), P.pinned.size(), -1);
    P.pinned.clear();
    return rc;
  }
  P.active = true;
  P.store = h->store;
  return GLOC_OK;
}

int gloc_reg_batch_multi_end(gloc_reg* h, float* out_T, float* out_rmse, uint32_t* out_inliers, int* out_ok) {
  GLOC_REQUIRE(h && out_T, GLOC_ERR_INVALID, "null argument");
  GLOC_REQUIRE(h->pending.active, GLOC_ERR_STATE, "no batch in flight on this handle");
  GLOC_HIP(hipSetDevice(h->device));
  gloc_reg::Pending& P = h->pending;
  P.active = false;
  struct Done {  // whatever happens below, the batch no longer reads the store's scans once its event has been waited for
    gloc_reg* h;
    gloc_scan_store* st;
    ~Done() {
      (void)hipEventSynchronize(h->done_ev);
      if (st) store_pin(st, h->pending.pinned.data(), h->pending.pinned.size(), -1);
      h->pending.pinned.clear();
    }
  } done{h, P.store};
  P.store = nullptr;
  for (size_t o = 0; o < P.total; ++o) {
    std::copy(P.def_T.begin() + 16 * o, P.def_T.begin() + 16 * (o + 1), out_T + 16 * o);
    if (out_rmse) out_rmse[o] = 0.f;
    if (out_inliers) out_inliers[o] = 0;
    if (out_ok) out_ok[o] = 0;
  }
  const size_t nj = P.slot.size();
  std::vector<float> T(16 * std::max<size_t>(nj, 1)), rm(std::max<size_t>(nj, 1));
  std::vector<uint32_t> inl(std::max<size_t>(nj, 1));
  std::vector<int> ok(std::max<size_t>(nj, 1));
  GLOC_TRY(collect_jobs(h, (uint32_t)nj, P.n_src.data(), P.max_rmse, P.max_final_step, T.data(), rm.data(), inl.data(), ok.data()));
  for (size_t j = 0; j < nj; ++j) {
    const size_t o = P.slot[j];
    std::copy(T.begin() + 16 * j, T.begin() + 16 * (j + 1), out_T + 16 * o);
    if (out_rmse) out_rmse[o] = rm[j];
    if (out_inliers) out_inliers[o] = inl[j];
    if (out_ok) out_ok[o] = ok[j];
  }
  return GLOC_OK;
}

int gloc_reg_batch_multi(gloc_reg* h, size_t n_queries, const uint32_t* q_scan_ids,
                         const uint32_t* cand_scan_ids, size_t n_cand, const uint32_t* cand_stream_ids,
                         const float* init_T, const gloc_reg_params* params, float* out_T,
                         float* out_rmse, uint32_t* out_inliers, int* out_ok) {
  GLOC_REQUIRE(out_T, GLOC_ERR_INVALID, "null argument");
  GLOC_TRY(gloc_reg_batch_multi_begin(h, n_queries, q_scan_ids, cand_scan_ids, n_cand, cand_stream_ids, init_T, params));
  return gloc_reg_batch_multi_end(h, out_T, out_rmse, out_inliers, out_ok);
}

int gloc_reg_first_success_multi(gloc_reg* h, size_t n_queries, const uint32_t* q_scan_ids,
                                 const uint32_t* cand_scan_ids, size_t n_cand, const float* init_T,
                                 const gloc_reg_params* params, int* out_rank, float* out_T, float* out_rmse,
                                 uint32_t* out_inliers, uint64_t* out_jobs_run) {
  GLOC_REQUIRE(h && q_scan_ids && cand_scan_ids && out_rank && out_T, GLOC_ERR_INVALID, "null argument");
  GLOC_NOT_PENDING(h);
  GLOC_REQUIRE(n_queries >= 1 && n_cand >= 1 && n_queries * n_cand <= 65536, GLOC_ERR_INVALID,
               "n_queries x n_cand = %zu x %zu outside [1, 65536]", n_queries, n_cand);
  GLOC_REQUIRE(h->store, GLOC_ERR_INVALID, "no scan store: upload scans or attach a store first");
  GLOC_TRY(check_params(params));
  GLOC_HIP(hipSetDevice(h->device));
  std::vector<DevScan> src(n_queries);
  for (size_t q = 0; q < n_queries; ++q) {
    GLOC_TRY(store_get(h->store, q_scan_ids[q], h->nn_src_per_lane, &src[q]));
    out_rank[q] = -1;
    std::copy_n(I16, 16, out_T + 16 * q);
    if (out_rmse) out_rmse[q] = 0.f;
    if (out_inliers) out_inliers[q] = 0;
  }
  std::vector<size_t> pending(n_queries);
  for (size_t q = 0; q < n_queries; ++q) pending[q] = q;
  uint64_t jobs_run = 0;
  std::vector<JobHost> jh;
  std::vector<size_t> who;
  std::vector<float> T, rm;
  std::vector<uint32_t> inl;
  std::vector<int> ok;
  // rank by rank, as GlocEvaluator::global_registraion walks a query's candidates
  // (registration/global_localization.cpp:519-572), but for all pending queries at once
  for (size_t r = 0; r < n_cand && !pending.empty(); ++r) {
    jh.clear();
    who.clear();
    for (size_t q : pending) {
      const size_t o = q * n_cand + r;
      if (cand_scan_ids[o] == 0xFFFFFFFFu) continue;
      JobHost j;
      j.src = src[q];
      GLOC_TRY(store_get(h->store, cand_scan_ids[o], 0, &j.tgt));  // a target's launch order is never read
      j.stream_id = (uint32_t)r;  // the RANSAC stream of retrieval rank r: the same job as in gloc_reg_batch_multi
      j.init_T = init_T ? init_T + 16 * o : nullptr;
      jh.push_back(j);
      who.push_back(q);
    }
    if (jh.empty()) continue;
    const size_t nj = jh.size();
    T.resize(16 * nj);
    rm.resize(nj);
    inl.resize(nj);
    ok.resize(nj);
    GLOC_TRY(run_jobs(h, jh, params, T.data(), rm.data(), inl.data(), ok.data()));
    jobs_run += nj;
    std::vector<size_t> still;
    size_t k = 0;
    for (size_t q : pending) {
      if (k < nj && who[k] == q) {
        if (ok[k]) {
          out_rank[q] = (int)r;
          std::copy(T.begin() + 16 * k, T.begin() + 16 * (k + 1), out_T + 16 * q);
          if (out_rmse) out_rmse[q] = rm[k];
          if (out_inliers) out_inliers[q] = inl[k];
        } else {
          still.push_back(q);
        }
        ++k;
      } else {
        still.push_back(q);  // no candidate at this rank
      }
    }
    pending.swap(still);
  }
  if (out_jobs_run) *out_jobs_run = jobs_run;
  return GLOC_OK;
}

int gloc_reg_batch_ids(gloc_reg* h, uint32_t q_scan_id, const uint32_t* cand_scan_ids,
                       size_t n_cand, const uint32_t* cand_stream_ids, const float* init_T,
                       const gloc_reg_params* params, float* out_T, float* out_rmse,
                       uint32_t* out_inliers, int* out_ok) {
  GLOC_REQUIRE(n_cand >= 1 && n_cand <= 4096, GLOC_ERR_INVALID, "n_cand = %zu outside [1,4096]", n_cand);
  if (cand_scan_ids)
    for (size_t c = 0; c < n_cand; ++c)
      GLOC_REQUIRE(cand_scan_ids[c] != 0xFFFFFFFFu, GLOC_ERR_INVALID, "unknown scan id %u", cand_scan_ids[c]);
  return gloc_reg_batch_multi(h, 1, &q_scan_id, cand_scan_ids, n_cand, cand_stream_ids, init_T, params, out_T,
                              out_rmse, out_inliers, out_ok);
}

int gloc_reg_final_steps(gloc_reg* h, float* out, size_t n) {
  GLOC_REQUIRE(h && (out || !n), GLOC_ERR_INVALID, "null argument");
  GLOC_REQUIRE(n <= h->last_final_step.size(), GLOC_ERR_INVALID, "the last batch had %zu jobs", h->last_final_step.size());
  std::copy(h->last_final_step.begin(), h->last_final_step.begin() + n, out);
  return GLOC_OK;
}

int gloc_reg_select_first_ok(const int* ok, size_t n_cand) {
  if (!ok) return -1;
  for (size_t i = 0; i < n_cand; ++i)
    if (ok[i]) return (int)i;
  return -1;
}

int gloc_reg_nn(gloc_reg* h, const float* src_xyz, size_t n_src, const float* tgt_xyz,
                size_t n_tgt, const float* T16, uint32_t* out_idx, float* out_d2) {
  GLOC_REQUIRE(h && out_idx && out_d2 && (src_xyz || !n_src) && (tgt_xyz || !n_tgt),
               GLOC_ERR_INVALID, "null argument");
  GLOC_REQUIRE(n_src < (1ull << 31) && n_tgt < (1ull << 31), GLOC_ERR_INVALID, "scan too large");
  GLOC_NOT_PENDING(h);
  if (n_src == 0) return GLOC_OK;
  GLOC_HIP(hipSetDevice(h->device));
  GLOC_TRY(ensure_store(h));
  hipStream_t s = h->stream;
  TempScans tmp(h->store);
  GLOC_TRY(tmp.add_all(src_xyz, n_src, h->nn_src_per_lane, &tgt_xyz, &n_tgt, 1, h->temp_target_index));
  // (whatever happens below, the temporary scans are not freed under a launch that reads them)
  struct SyncOnExit {
    hipStream_t s;
    ~SyncOnExit() { (void)hipStreamSynchronize(s); }
  } sync{s};
  const DevScan &sc = tmp.scans[0], &tg = tmp.scans[1];
  const uint32_t ng = src_groups(n_src, h->nn_src_per_lane);
  Batch b;  // (one cold pass: there is no estimate to plan a split from)
  GLOC_TRY(open_batch(h, BatchSpec::searching(1, n_src, ng), &b, [&](Job* jd, CandState* st) {
    jd[0] = Job{sc.idx.pts, sc.order, sc.idx.inv, tg.xyz, tg.idx, (uint32_t)n_src, ng, 0u, 0u};
    init_state(st[0], T16);
  }));
  const size_t ld = b.bd.ld;
  GLOC_TRY(h->export_idx.ensure(sizeof(uint32_t) * ld, s));
  GLOC_TRY(h->export_d2.ensure(sizeof(float) * ld, s));
  GLOC_TRY(launch_nn(h, b.bd, b.v, false, false, 0.f));
  hipLaunchKernelGGL(export_corr_kernel, dim3((unsigned)((n_src + 255) / 256), 1), dim3(256), 0, s, b.v.jobs, b.v.corr, b.v.d2, ld,
                     h->export_idx.as<uint32_t>(), h->export_d2.as<float>());
  GLOC_HIP(hipGetLastError());
  GLOC_HIP(hipMemcpyAsync(out_idx, h->export_idx.p, sizeof(uint32_t) * n_src, hipMemcpyDeviceToHost, s));
  GLOC_HIP(hipMemcpyAsync(out_d2, h->export_d2.p, sizeof(float) * n_src, hipMemcpyDeviceToHost, s));
  GLOC_HIP(hipStreamSynchronize(s));
  return GLOC_OK;
}

int gloc_reg_ransac_hypotheses(gloc_reg* h, const float* src_xyz, const float* tgt_xyz,
                               const uint32_t* corr, size_t n, uint64_t seed, uint32_t cand,
                               uint32_t n_hyp, float* out_Rt, uint32_t* out_valid,
                               uint32_t* out_inliers, float inlier_thresh) {
  GLOC_REQUIRE(h && src_xyz && tgt_xyz && corr && out_Rt && out_valid && out_inliers,
               GLOC_ERR_INVALID, "null argument");
  GLOC_REQUIRE(n >= 3 && n < (1ull << 31) && n_hyp >= 1 && n_hyp <= (1u << 20), GLOC_ERR_INVALID,
               "bad sizes");
  GLOC_NOT_PENDING(h);
  GLOC_HIP(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  // pairs are built on the host from (src, tgt[corr]) -- src is taken as already moved; slots are the
  // caller's indices (no inverse permutation)
  Batch b;
  GLOC_TRY(open_batch(h, BatchSpec::on_pairs(1, n, n_hyp, false), &b, [&](Job* jd, CandState* st) {
    jd[0] = Job{};
    jd[0].n_src = (uint32_t)n;
    jd[0].cand_id = cand;
    init_state(st[0], nullptr);  // (not read: the hypotheses are generated and scored, never scanned)
  }));
  const WsView& v = b.v;
  const size_t ld = b.bd.ld;
  const std::vector<float> hp = pack_pairs(src_xyz, tgt_xyz, corr, n, ld);
  GLOC_HIP(hipMemcpyAsync(v.pairs, hp.data(), sizeof(float) * hp.size(), hipMemcpyHostToDevice, s));
  GLOC_HIP(hipMemsetAsync(v.inliers, 0, sizeof(uint32_t) * (size_t)n_hyp, s));
  hipLaunchKernelGGL(ransac_hyp_kernel, dim3((n_hyp + 127) / 128, 1), dim3(128), 0, s, v.pairs, ld, v.jobs, seed, n_hyp, 0u, n_hyp,
                     (const CandState*)nullptr, v.Rt, v.valid, (unsigned long long*)nullptr);
  GLOC_HIP(hipGetLastError());
  dim3 grid((n_hyp + 255) / 256, (unsigned)((n + SC_CHUNK - 1) / SC_CHUNK), 1);
  hipLaunchKernelGGL(ransac_score_kernel, grid, dim3(256), 0, s, v.pairs, ld, v.jobs, n_hyp, 0u, 256u /* thread <-> hypothesis */, v.Rt,
                     v.valid, inlier_thresh * inlier_thresh, (const CandState*)nullptr, v.inliers, (const uint32_t*)nullptr,
                     (const uint32_t*)nullptr, 0u, (uint32_t)SC_CHUNK, (unsigned long long*)nullptr);
  GLOC_HIP(hipGetLastError());
  GLOC_HIP(hipMemcpyAsync(out_Rt, v.Rt, sizeof(float) * 12 * (size_t)n_hyp, hipMemcpyDeviceToHost, s));
  GLOC_HIP(hipMemcpyAsync(out_valid, v.valid, sizeof(uint32_t) * (size_t)n_hyp, hipMemcpyDeviceToHost, s));
  GLOC_HIP(hipMemcpyAsync(out_inliers, v.inliers, sizeof(uint32_t) * (size_t)n_hyp, hipMemcpyDeviceToHost, s));
  GLOC_HIP(hipStreamSynchronize(s));
  return GLOC_OK;
}

int gloc_reg_nn_stats(gloc_reg* h, uint64_t* pairs_evaluated, uint64_t* launches) {
  GLOC_REQUIRE(h, GLOC_ERR_INVALID, "null handle");
  GLOC_HIP(hipSetDevice(h->device));
  unsigned long long c = 0;
  if (h->counters.p) {
    std::vector<unsigned long long> part(NN_STAT_SLOTS);
    GLOC_HIP(hipMemcpyAsync(part.data(), h->counters.p, 8 * NN_STAT_SLOTS, hipMemcpyDeviceToHost, h->stream));
    GLOC_HIP(hipStreamSynchronize(h->stream));
    for (unsigned long long v : part) c += v;
  }
  if (pairs_evaluated) *pairs_evaluated = c;
  if (launches) *launches = h->nn_launches;
  return GLOC_OK;
}

// Developer / test aid (not part of include/gloc3d.h): the correspondences of the LAST 1-NN pass of the
// last batch for job `job`, in the caller's index space (original source index -> original target index).
int gloc_reg_debug_corr(gloc_reg* h, uint32_t job, uint32_t n_src, uint32_t* out_idx, float* out_d2) {
  GLOC_REQUIRE(h && out_idx && out_d2, GLOC_ERR_INVALID, "null argument");
  GLOC_HIP(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  const size_t ld = h->last_ld;
  GLOC_NOT_PENDING(h);
  GLOC_REQUIRE(job < h->last_jobs && n_src <= ld, GLOC_ERR_INVALID, "no such job in the last batch");
  GLOC_TRY(h->export_idx.ensure(sizeof(uint32_t) * ld * h->last_jobs, s));
  GLOC_TRY(h->export_d2.ensure(sizeof(float) * ld * h->last_jobs, s));
  hipLaunchKernelGGL(export_corr_kernel, dim3((unsigned)((ld + 255) / 256), h->last_jobs), dim3(256), 0, s,
                     h->jobs.as<Job>(), h->corr.as<uint32_t>(), h->d2.as<float>(), ld,
                     h->export_idx.as<uint32_t>(), h->export_d2.as<float>());
  GLOC_HIP(hipGetLastError());
  GLOC_HIP(hipMemcpyAsync(out_idx, h->export_idx.as<uint32_t>() + (size_t)job * ld, sizeof(uint32_t) * n_src,
                          hipMemcpyDeviceToHost, s));
  GLOC_HIP(hipMemcpyAsync(out_d2, h->export_d2.as<float>() + (size_t)job * ld, sizeof(float) * n_src,
                          hipMemcpyDeviceToHost, s));
  GLOC_HIP(hipStreamSynchronize(s));
  return GLOC_OK;
}

// Developer / test aid (not part of include/gloc3d.h): chained launches enqueued and chained launches that timed out.
int gloc_reg_debug_chain(gloc_reg* h, uint64_t* launches, uint64_t* timeouts) {
  GLOC_REQUIRE(h, GLOC_ERR_INVALID, "null handle");
  if (launches) *launches = h->chain_launches;
  if (timeouts) *timeouts = h->chain_timeouts;
  return GLOC_OK;
}

// Test aid (not part of include/gloc3d.h): the adaptive stop's iteration count as the DEVICE computes it, for `count`
// (inliers, points) pairs -- compared with the oracle's loop in tests/test_reg_gpu.py.
int gloc_reg_debug_needed_iters(gloc_reg* h, const uint32_t* inl, const uint32_t* n, uint32_t count, float conf, uint32_t max_iters,
                                uint32_t* out) {
  GLOC_REQUIRE(h && inl && n && out, GLOC_ERR_INVALID, "null argument");
  GLOC_HIP(hipSetDevice(h->device));
  GLOC_NOT_PENDING(h);
  hipStream_t s = h->stream;
  GLOC_TRY(h->export_idx.ensure(sizeof(uint32_t) * 3 * (size_t)count, s));
  uint32_t* d = h->export_idx.as<uint32_t>();
  GLOC_HIP(hipMemcpyAsync(d, inl, 4 * (size_t)count, hipMemcpyHostToDevice, s));
  GLOC_HIP(hipMemcpyAsync(d + count, n, 4 * (size_t)count, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(needed_iters_kernel, dim3((count + 255) / 256), dim3(256), 0, s, d, d + count, conf, max_iters, d + 2 * (size_t)count, count);
  GLOC_HIP(hipGetLastError());
  GLOC_HIP(hipMemcpyAsync(out, d + 2 * (size_t)count, 4 * (size_t)count, hipMemcpyDeviceToHost, s));
  GLOC_HIP(hipStreamSynchronize(s));
  return GLOC_OK;
}

// Test aid (not part of include/gloc3d.h): the next chained launches wait for a wave that never comes -- every wait runs
// out, the launch ends by itself, the batch is run again launch by launch (tests/test_reg_gpu.py: the bounded waits).
int gloc_reg_debug_chain_stall(gloc_reg* h, int on) {
  GLOC_REQUIRE(h, GLOC_ERR_INVALID, "null handle");
  h->chain_stall = on != 0;
  return GLOC_OK;
}

int gloc_reg_ndt_batch_ids(gloc_reg* h, uint32_t src_scan_id, const uint32_t* tgt_scan_ids, size_t n, const float* init_T,
                           const gloc_ndt_params* prm, float* out_T, double* out_prob, uint32_t* out_iters,
                           int* out_converged) {
  GLOC_REQUIRE(h && out_T && tgt_scan_ids, GLOC_ERR_INVALID, "null argument");
  GLOC_NOT_PENDING(h);
  GLOC_HIP(hipSetDevice(h->device));
  return gloc::ndt::run(ndt_ctx(h), src_scan_id, tgt_scan_ids, n, init_T, nullptr, prm, out_T, out_prob, out_iters, out_converged,
                        nullptr);
}

int gloc_reg_ndt_derivatives(gloc_reg* h, uint32_t src_scan_id, uint32_t tgt_scan_id, const double p6[6],
                             const gloc_ndt_params* prm, double* out_score, double* out_grad6, double* out_hess36) {
  GLOC_REQUIRE(h && p6 && out_score && out_grad6 && out_hess36, GLOC_ERR_INVALID, "null argument");
  GLOC_NOT_PENDING(h);
  GLOC_HIP(hipSetDevice(h->device));
  double s[43];
  GLOC_TRY(gloc::ndt::run(ndt_ctx(h), src_scan_id, &tgt_scan_id, 1, nullptr, p6, prm, nullptr, nullptr, nullptr, nullptr, s));
  *out_score = s[0];
  for (int i = 0; i < 6; ++i) out_grad6[i] = s[1 + i];
  for (int i = 0; i < 36; ++i) out_hess36[i] = s[7 + i];
  return GLOC_OK;
}

int gloc_reg_ndt_cells(gloc_reg* h, uint32_t scan_id, const gloc_ndt_params* prm, size_t capacity, int32_t* out_key3,
                       uint32_t* out_count, double* out_mean3, double* out_icov9, size_t* n_cells) {
  GLOC_REQUIRE(h && n_cells, GLOC_ERR_INVALID, "null argument");
  GLOC_NOT_PENDING(h);
  GLOC_HIP(hipSetDevice(h->device));
  return gloc::ndt::cells(ndt_ctx(h), scan_id, prm, capacity, out_key3, out_count, out_mean3, out_icov9, n_cells);
}

// The entries of the three Gauss-Newton refinements: each fills its call (batch_call / system_call, the robust half behind
// it) and hands it with the method's block to refine_entry.
int gloc_reg_p2l_batch_ids(gloc_reg* h, uint32_t src_scan_id, const uint32_t* tgt_scan_ids, size_t n, const float* init_T,
                           const gloc_p2l_params* prm, float* out_T, float* out_rmse, uint32_t* out_iters, int* out_status) {
  return refine_entry(h, batch_call(&src_scan_id, false, tgt_scan_ids, n, init_T, out_T, out_rmse, out_iters, out_status), prm,
                      gloc::p2l::check_params, run_p2l);
}

int gloc_reg_p2l_system(gloc_reg* h, uint32_t src_scan_id, uint32_t tgt_scan_id, const float* T16, const gloc_p2l_params* prm,
                        double* out_H36, double* out_g6, double* out_sum_r2, uint64_t* out_count) {
  return refine_entry(h, system_call(&src_scan_id, &tgt_scan_id, T16, out_H36, out_g6, out_sum_r2, out_count), prm,
                      gloc::p2l::check_params, run_p2l);
}

int gloc_reg_gicp_batch_ids(gloc_reg* h, uint32_t src_scan_id, const uint32_t* tgt_scan_ids, size_t n, const float* init_T,
                            const gloc_gicp_params* prm, float* out_T, float* out_rmse, uint32_t* out_iters, int* out_status) {
  return refine_entry(h, batch_call(&src_scan_id, false, tgt_scan_ids, n, init_T, out_T, out_rmse, out_iters, out_status), prm,
                      gloc::gicp::check_params, run_gicp);
}

int gloc_reg_gicp_system(gloc_reg* h, uint32_t src_scan_id, uint32_t tgt_scan_id, const float* T16, const gloc_gicp_params* prm,
                         double* out_H36, double* out_g6, double* out_sum, uint64_t* out_count) {
  return refine_entry(h, system_call(&src_scan_id, &tgt_scan_id, T16, out_H36, out_g6, out_sum, out_count), prm,
                      gloc::gicp::check_params, run_gicp);
}

int gloc_reg_vgicp_batch_ids(gloc_reg* h, uint32_t src_scan_id, const uint32_t* tgt_scan_ids, size_t n, const float* init_T,
                             const gloc_vgicp_params* prm, float* out_T, float* out_rmse, uint32_t* out_iters, int* out_status) {
  return refine_entry(h, batch_call(&src_scan_id, false, tgt_scan_ids, n, init_T, out_T, out_rmse, out_iters, out_status), prm,
                      gloc::vgicp::check_params, run_vgicp);
}

int gloc_reg_vgicp_system(gloc_reg* h, uint32_t src_scan_id, uint32_t tgt_scan_id, const float* T16, const gloc_vgicp_params* prm,
                          double* out_H36, double* out_g6, double* out_sum, uint64_t* out_count) {
  return refine_entry(h, system_call(&src_scan_id, &tgt_scan_id, T16, out_H36, out_g6, out_sum, out_count), prm,
                      gloc::vgicp::check_params, run_vgicp);
}

int gloc_reg_p2l_batch_ids_robust(gloc_reg* h, uint32_t src_scan_id, const uint32_t* tgt_scan_ids, size_t n, const float* init_T,
                                  const gloc_p2l_params* prm, const gloc_robust_params* robust, float* out_T, float* out_rmse,
                                  uint32_t* out_iters, int* out_status, float* out_weight) {
  const gloc::gn6::Call c = batch_call(&src_scan_id, false, tgt_scan_ids, n, init_T, out_T, out_rmse, out_iters, out_status);
  return refine_entry(h, robust_call(c, robust, 0, out_weight, nullptr), prm, gloc::p2l::check_params, run_p2l);
}

int gloc_reg_p2l_system_robust(gloc_reg* h, uint32_t src_scan_id, uint32_t tgt_scan_id, const float* T16, const gloc_p2l_params* prm,
                               const gloc_robust_params* robust, uint32_t pass, double* out_H36, double* out_g6, double* out_sum_r2,
                               uint64_t* out_count, double* out_wsum) {
  const gloc::gn6::Call c = system_call(&src_scan_id, &tgt_scan_id, T16, out_H36, out_g6, out_sum_r2, out_count);
  return refine_entry(h, robust_call(c, robust, pass, nullptr, out_wsum), prm, gloc::p2l::check_params, run_p2l);
}

int gloc_reg_gicp_batch_ids_robust(gloc_reg* h, uint32_t src_scan_id, const uint32_t* tgt_scan_ids, size_t n, const float* init_T,
                                   const gloc_gicp_params* prm, const gloc_robust_params* robust, float* out_T, float* out_rmse,
                                   uint32_t* out_iters, int* out_status, float* out_weight) {
  const gloc::gn6::Call c = batch_call(&src_scan_id, false, tgt_scan_ids, n, init_T, out_T, out_rmse, out_iters, out_status);
  return refine_entry(h, robust_call(c, robust, 0, out_weight, nullptr), prm, gloc::gicp::check_params, run_gicp);
}

int gloc_reg_gicp_system_robust(gloc_reg* h, uint32_t src_scan_id, uint32_t tgt_scan_id, const float* T16, const gloc_gicp_params* prm,
                                const gloc_robust_params* robust, uint32_t pass, double* out_H36, double* out_g6, double* out_sum,
                                uint64_t* out_count, double* out_wsum) {
  const gloc::gn6::Call c = system_call(&src_scan_id, &tgt_scan_id, T16, out_H36, out_g6, out_sum, out_count);
  return refine_entry(h, robust_call(c, robust, pass, nullptr, out_wsum), prm, gloc::gicp::check_params, run_gicp);
}

int gloc_reg_vgicp_batch_ids_robust(gloc_reg* h, uint32_t src_scan_id, const uint32_t* tgt_scan_ids, size_t n, const float* init_T,
                                    const gloc_vgicp_params* prm, const gloc_robust_params* robust, float* out_T, float* out_rmse,
                                    uint32_t* out_iters, int* out_status, float* out_weight) {
  const gloc::gn6::Call c = batch_call(&src_scan_id, false, tgt_scan_ids, n, init_T, out_T, out_rmse, out_iters, out_status);
  return refine_entry(h, robust_call(c, robust, 0, out_weight, nullptr), prm, gloc::vgicp::check_params, run_vgicp);
}

int gloc_reg_vgicp_system_robust(gloc_reg* h, uint32_t src_scan_id, uint32_t tgt_scan_id, const float* T16,
                                 const gloc_vgicp_params* prm, const gloc_robust_params* robust, uint32_t pass, double* out_H36,
                                 double* out_g6, double* out_sum, uint64_t* out_count, double* out_wsum) {
  const gloc::gn6::Call c = system_call(&src_scan_id, &tgt_scan_id, T16, out_H36, out_g6, out_sum, out_count);
  return refine_entry(h, robust_call(c, robust, pass, nullptr, out_wsum), prm, gloc::vgicp::check_params, run_vgicp);
}

// The pair-list entries: row c is (src_scan_ids[c], tgt_scan_ids[c]), every row the single-source entry's row.  The robust
// block may be null (the plain step, which has no weights to report).
int gloc_reg_p2l_pairs(gloc_reg* h, const uint32_t* src_scan_ids, const uint32_t* tgt_scan_ids, size_t n, const float* init_T,
                       const gloc_p2l_params* prm, const gloc_robust_params* robust, float* out_T, float* out_rmse, uint32_t* out_iters,
                       int* out_status, float* out_weight) {
  gloc::gn6::Call c = batch_call(src_scan_ids, true, tgt_scan_ids, n, init_T, out_T, out_rmse, out_iters, out_status);
  c.robust = robust;
  c.out_weight = robust ? out_weight : nullptr;
  return refine_entry(h, c, prm, gloc::p2l::check_params, run_p2l);
}

int gloc_reg_gicp_pairs(gloc_reg* h, const uint32_t* src_scan_ids, const uint32_t* tgt_scan_ids, size_t n, const float* init_T,
                        const gloc_gicp_params* prm, const gloc_robust_params* robust, float* out_T, float* out_rmse, uint32_t* out_iters,
                        int* out_status, float* out_weight) {
  gloc::gn6::Call c = batch_call(src_scan_ids, true, tgt_scan_ids, n, init_T, out_T, out_rmse, out_iters, out_status);
  c.robust = robust;
  c.out_weight = robust ? out_weight : nullptr;
  return refine_entry(h, c, prm, gloc::gicp::check_params, run_gicp);
}

int gloc_reg_vgicp_pairs(gloc_reg* h, const uint32_t* src_scan_ids, const uint32_t* tgt_scan_ids, size_t n, const float* init_T,
                         const gloc_vgicp_params* prm, const gloc_robust_params* robust, float* out_T, float* out_rmse, uint32_t* out_iters,
                         int* out_status, float* out_weight) {
  gloc::gn6::Call c = batch_call(src_scan_ids, true, tgt_scan_ids, n, init_T, out_T, out_rmse, out_iters, out_status);
  c.robust = robust;
  c.out_weight = robust ? out_weight : nullptr;
  return refine_entry(h, c, prm, gloc::vgicp::check_params, run_vgicp);
}

// The system form of the pair lists: row c is the single-pair _system (robust NULL) or _system_robust entry's result.
int gloc_reg_p2l_pairs_system(gloc_reg* h, const uint32_t* src_scan_ids, const uint32_t* tgt_scan_ids, size_t n, const float* T,
                              const gloc_p2l_params* prm, const gloc_robust_params* robust, uint32_t pass, double* out_H36, double* out_g6,
                              double* out_sum, uint64_t* out_count, double* out_wsum) {
  return refine_entry(h, pairs_system_call(src_scan_ids, tgt_scan_ids, n, T, robust, pass, out_H36, out_g6, out_sum, out_count, out_wsum), prm,
                      gloc::p2l::check_params, run_p2l);
}

int gloc_reg_gicp_pairs_system(gloc_reg* h, const uint32_t* src_scan_ids, const uint32_t* tgt_scan_ids, size_t n, const float* T,
                               const gloc_gicp_params* prm, const gloc_robust_params* robust, uint32_t pass, double* out_H36, double* out_g6,
                               double* out_sum, uint64_t* out_count, double* out_wsum) {
  return refine_entry(h, pairs_system_call(src_scan_ids, tgt_scan_ids, n, T, robust, pass, out_H36, out_g6, out_sum, out_count, out_wsum), prm,
                      gloc::gicp::check_params, run_gicp);
}

int gloc_reg_vgicp_pairs_system(gloc_reg* h, const uint32_t* src_scan_ids, const uint32_t* tgt_scan_ids, size_t n, const float* T,
                                const gloc_vgicp_params* prm, const gloc_robust_params* robust, uint32_t pass, double* out_H36, double* out_g6,
                                double* out_sum, uint64_t* out_count, double* out_wsum) {
  return refine_entry(h, pairs_system_call(src_scan_ids, tgt_scan_ids, n, T, robust, pass, out_H36, out_g6, out_sum, out_count, out_wsum), prm,
                      gloc::vgicp::check_params, run_vgicp);
}

// The point-to-point evaluation of a pair list (include/gloc3d.h: V1 - V6).  The block, the arrays and n, the handle, a
// batch in flight -- the order of refine_entry.
int gloc_reg_evaluate_pairs(gloc_reg* h, const uint32_t* src_scan_ids, const uint32_t* tgt_scan_ids, size_t n, const float* T,
                            const gloc_eval_params* prm, float* out_fitness, float* out_rmse, uint32_t* out_count, double* out_info36,
                            double* out_g6) {
  GLOC_TRY(gloc::eval::check_params(prm));
  GLOC_REQUIRE(src_scan_ids && tgt_scan_ids, GLOC_ERR_INVALID, "null scan ids");
  GLOC_REQUIRE(out_fitness || out_rmse || out_count || out_info36 || out_g6, GLOC_ERR_INVALID, "every output is null");
  GLOC_REQUIRE(n >= 1 && n <= 4096, GLOC_ERR_INVALID, "n = %zu outside [1, 4096]", n);
  GLOC_REQUIRE(h, GLOC_ERR_INVALID, "null argument");
  GLOC_NOT_PENDING(h);
  GLOC_HIP(hipSetDevice(h->device));
  gloc::gn6::Call c;
  c.src_ids = src_scan_ids;
  c.pairs = true;
  c.tgt_ids = tgt_scan_ids;
  c.n = n;
  c.init_T = T;
  c.system = true;
  return run_eval(h, c, prm, gloc::eval::Out{out_fitness, out_rmse, out_count, out_info36, out_g6});
}

int gloc_reg_vgicp_voxels(gloc_reg* h, uint32_t scan_id, const gloc_vgicp_params* prm, size_t capacity, int32_t* out_key3,
                          uint32_t* out_count, double* out_mean3, double* out_nn6, size_t* n_voxels) {
  GLOC_TRY(gloc::vgicp::check_params(prm));
  GLOC_REQUIRE(h && n_voxels, GLOC_ERR_INVALID, "null argument");
  GLOC_NOT_PENDING(h);
  GLOC_HIP(hipSetDevice(h->device));
  return gloc::vgicp::voxels(vgicp_ctx(h), scan_id, prm, capacity, out_key3, out_count, out_mean3, out_nn6, n_voxels);
}

// Resident voxel maps (include/gloc3d.h: M1 - M8; vmap.hip).  The parameters and the arguments, the handle, a batch in
// flight, the map's id -- the order of refine_entry -- and all of it before any device work.
int gloc_reg_vmap_create(gloc_reg* h, const gloc_vmap_params* prm, uint32_t* out_map_id) {
  GLOC_TRY(gloc::vmap::check_params(prm));
  GLOC_REQUIRE(h && out_map_id, GLOC_ERR_INVALID, "null argument");
  GLOC_NOT_PENDING(h);
  GLOC_HIP(hipSetDevice(h->device));
  return gloc::vmap::create(vmap_ctx(h), prm, out_map_id);
}

int gloc_reg_vmap_destroy(gloc_reg* h, uint32_t map_id) {
  GLOC_TRY(vmap_entry(h, map_id));
  return gloc::vmap::destroy(vmap_ctx(h), map_id);
}

int gloc_reg_vmap_insert(gloc_reg* h, uint32_t map_id, const uint32_t* scan_ids, size_t n, const float* T) {
  GLOC_REQUIRE(scan_ids, GLOC_ERR_INVALID, "null scan ids");
  GLOC_REQUIRE(n >= 1 && n <= 4096, GLOC_ERR_INVALID, "n = %zu outside [1, 4096]", n);
  GLOC_TRY(vmap_entry(h, map_id));
  return gloc::vmap::insert(vmap_ctx(h), map_id, scan_ids, n, T);
}

int gloc_reg_vmap_prune(gloc_reg* h, uint32_t map_id, const float* center3, float max_dist, uint32_t max_age, uint32_t* out_removed) {
  GLOC_REQUIRE(!center3 || (max_dist >= 0.f && max_dist <= 3.0e38f), GLOC_ERR_INVALID, "max_dist = %g must be >= 0 and finite", (double)max_dist);
  GLOC_TRY(vmap_entry(h, map_id));
  return gloc::vmap::prune(vmap_ctx(h), map_id, center3, max_dist, max_age, out_removed);
}

int gloc_reg_vmap_info(gloc_reg* h, uint32_t map_id, gloc_vmap_info* out) {
  GLOC_REQUIRE(out, GLOC_ERR_INVALID, "null argument");
  GLOC_TRY(vmap_entry(h, map_id));
  return gloc::vmap::info(vmap_ctx(h), map_id, out);
}

int gloc_reg_vmap_voxels(gloc_reg* h, uint32_t map_id, size_t capacity, int32_t* out_key3, uint32_t* out_count, double* out_mean3,
                         double* out_nn6, uint32_t* out_stamp, size_t* n_voxels) {
  GLOC_REQUIRE(n_voxels, GLOC_ERR_INVALID, "null argument");
  GLOC_TRY(vmap_entry(h, map_id));
  return gloc::vmap::voxels(vmap_ctx(h), map_id, capacity, out_key3, out_count, out_mean3, out_nn6, out_stamp, n_voxels);
}

// The pair-list entries with maps for targets: row c is (src_scan_ids[c], map_ids[c]).
int gloc_reg_vgicp_vmap(gloc_reg* h, const uint32_t* src_scan_ids, const uint32_t* map_ids, size_t n, const float* init_T,
                        const gloc_vgicp_params* prm, const gloc_robust_params* robust, float* out_T, float* out_rmse, uint32_t* out_iters,
                        int* out_status, float* out_weight) {
  gloc::gn6::Call c = batch_call(src_scan_ids, true, map_ids, n, init_T, out_T, out_rmse, out_iters, out_status);
  c.robust = robust;
  c.out_weight = robust ? out_weight : nullptr;
  return refine_entry(h, c, prm, gloc::vgicp::check_params, run_vgicp_vmap);
}

int gloc_reg_vgicp_vmap_system(gloc_reg* h, const uint32_t* src_scan_ids, const uint32_t* map_ids, size_t n, const float* T,
                               const gloc_vgicp_params* prm, const gloc_robust_params* robust, uint32_t pass, double* out_H36, double* out_g6,
                               double* out_sum, uint64_t* out_count, double* out_wsum) {
  return refine_entry(h, pairs_system_call(src_scan_ids, map_ids, n, T, robust, pass, out_H36, out_g6, out_sum, out_count, out_wsum), prm,
                      gloc::vgicp::check_params, run_vgicp_vmap);
}

// (the parameters are looked at before the handle, as generalized ICP's are)
int gloc_reg_fpfh_batch_ids(gloc_reg* h, uint32_t src_scan_id, const uint32_t* tgt_scan_ids, size_t n, const uint32_t* stream_ids,
                            const gloc_fpfh_params* prm, float* out_T, uint32_t* out_inliers, uint32_t* out_n_pairs, int* out_ok) {
  GLOC_TRY(gloc::fpfh::check_params(prm));
  GLOC_REQUIRE(h && out_T && tgt_scan_ids, GLOC_ERR_INVALID, "null argument");
  GLOC_NOT_PENDING(h);
  GLOC_HIP(hipSetDevice(h->device));
  return run_fpfh(h, src_scan_id, tgt_scan_ids, n, stream_ids, prm, Support::nearest(prm->normal_k), Support::nearest(prm->feature_k), out_T,
                  out_inliers, out_n_pairs, out_ok);
}

int gloc_reg_fpfh_batch_ids_radius(gloc_reg* h, uint32_t src_scan_id, const uint32_t* tgt_scan_ids, size_t n, const uint32_t* stream_ids,
                                   const gloc_fpfh_params* prm, const gloc_fpfh_radius_params* support, float* out_T, uint32_t* out_inliers,
                                   uint32_t* out_n_pairs, int* out_ok) {
  GLOC_TRY(gloc::fpfh::check_params(prm));
  GLOC_TRY(gloc::fpfh::check_radius_params(support));
  GLOC_REQUIRE(h && out_T && tgt_scan_ids, GLOC_ERR_INVALID, "null argument");
  GLOC_NOT_PENDING(h);
  GLOC_HIP(hipSetDevice(h->device));
  return run_fpfh(h, src_scan_id, tgt_scan_ids, n, stream_ids, prm, Support::normals_of(*support), Support::features_of(*support), out_T,
                  out_inliers, out_n_pairs, out_ok);
}

int gloc_reg_fpfh_graph_batch_ids(gloc_reg* h, uint32_t src_scan_id, const uint32_t* tgt_scan_ids, size_t n,
                                  const gloc_fpfh_graph_params* prm, float* out_T, uint32_t* out_inliers, uint32_t* out_n_pairs,
                                  int* out_ok) {
  GLOC_TRY(gloc::pairgraph::check_params(prm));
  GLOC_REQUIRE(h && out_T && tgt_scan_ids, GLOC_ERR_INVALID, "null argument");
  GLOC_NOT_PENDING(h);
  GLOC_HIP(hipSetDevice(h->device));
  return run_fpfh_graph(h, src_scan_id, tgt_scan_ids, n, prm, Support::nearest(prm->normal_k), Support::nearest(prm->feature_k), out_T,
                        out_inliers, out_n_pairs, out_ok);
}

int gloc_reg_fpfh_graph_batch_ids_radius(gloc_reg* h, uint32_t src_scan_id, const uint32_t* tgt_scan_ids, size_t n,
                                         const gloc_fpfh_graph_params* prm, const gloc_fpfh_radius_params* support, float* out_T,
                                         uint32_t* out_inliers, uint32_t* out_n_pairs, int* out_ok) {
  GLOC_TRY(gloc::pairgraph::check_params(prm));
  GLOC_TRY(gloc::fpfh::check_radius_params(support));
  GLOC_REQUIRE(h && out_T && tgt_scan_ids, GLOC_ERR_INVALID, "null argument");
  GLOC_NOT_PENDING(h);
  GLOC_HIP(hipSetDevice(h->device));
  return run_fpfh_graph(h, src_scan_id, tgt_scan_ids, n, prm, Support::normals_of(*support), Support::features_of(*support), out_T,
                        out_inliers, out_n_pairs, out_ok);
}

// (support == NULL: the k-mode features of prm)
int gloc_reg_fpfh_batch_ids_keypoints(gloc_reg* h, uint32_t src_scan_id, const uint32_t* tgt_scan_ids, size_t n, const uint32_t* stream_ids,
                                      const gloc_fpfh_params* prm, const gloc_fpfh_radius_params* support, const gloc_iss_params* iss,
                                      float* out_T, uint32_t* out_inliers, uint32_t* out_n_pairs, int* out_ok) {
  GLOC_TRY(gloc::fpfh::check_params(prm));
  if (support) GLOC_TRY(gloc::fpfh::check_radius_params(support));
  GLOC_TRY(check_iss_params(iss));
  GLOC_REQUIRE(h && out_T && tgt_scan_ids, GLOC_ERR_INVALID, "null argument");
  GLOC_NOT_PENDING(h);
  GLOC_HIP(hipSetDevice(h->device));
  return run_fpfh(h, src_scan_id, tgt_scan_ids, n, stream_ids, prm, support ? Support::normals_of(*support) : Support::nearest(prm->normal_k),
                  support ? Support::features_of(*support) : Support::nearest(prm->feature_k), out_T, out_inliers, out_n_pairs, out_ok, iss);
}

int gloc_reg_fpfh_graph_batch_ids_keypoints(gloc_reg* h, uint32_t src_scan_id, const uint32_t* tgt_scan_ids, size_t n,
                                            const gloc_fpfh_graph_params* prm, const gloc_fpfh_radius_params* support,
                                            const gloc_iss_params* iss, float* out_T, uint32_t* out_inliers, uint32_t* out_n_pairs,
                                            int* out_ok) {
  GLOC_TRY(gloc::pairgraph::check_params(prm));
  if (support) GLOC_TRY(gloc::fpfh::check_radius_params(support));
  GLOC_TRY(check_iss_params(iss));
  GLOC_REQUIRE(h && out_T && tgt_scan_ids, GLOC_ERR_INVALID, "null argument");
  GLOC_NOT_PENDING(h);
  GLOC_HIP(hipSetDevice(h->device));
  return run_fpfh_graph(h, src_scan_id, tgt_scan_ids, n, prm, support ? Support::normals_of(*support) : Support::nearest(prm->normal_k),
                        support ? Support::features_of(*support) : Support::nearest(prm->feature_k), out_T, out_inliers, out_n_pairs, out_ok,
                        iss);
}

int gloc_reg_pair_graph(gloc_reg* h, const float* P, const float* Q, size_t m, const gloc_fpfh_graph_params* prm,
                        uint32_t* out_degree, uint64_t* out_score, uint32_t* out_seeds, uint32_t* out_set_sizes,
                        uint32_t* out_seed_inliers, float* out_T, uint32_t* out_inliers, uint32_t* out_winner_rank, int* out_ok) {
  GLOC_TRY(gloc::pairgraph::check_params(prm));
  GLOC_REQUIRE(h && ((P && Q) || m == 0), GLOC_ERR_INVALID, "null argument");
  GLOC_REQUIRE(m < (1ull << 31), GLOC_ERR_INVALID, "too many pairs");
  GLOC_NOT_PENDING(h);
  GLOC_HIP(hipSetDevice(h->device));
  return run_pair_graph(h, P, Q, m, prm, out_degree, out_score, out_seeds, out_set_sizes, out_seed_inliers, out_T, out_inliers,
                        out_winner_rank, out_ok);
}

int gloc_reg_fpfh_fgr_batch_ids(gloc_reg* h, uint32_t src_scan_id, const uint32_t* tgt_scan_ids, size_t n, const uint32_t* stream_ids,
                                const gloc_fgr_params* prm, float* out_T, uint32_t* out_inliers, uint32_t* out_n_pairs, int* out_ok) {
  GLOC_TRY(gloc::fgr::check_params(prm));
  GLOC_REQUIRE(h && out_T && tgt_scan_ids, GLOC_ERR_INVALID, "null argument");
  GLOC_NOT_PENDING(h);
  GLOC_HIP(hipSetDevice(h->device));
  return run_fpfh_fgr(h, src_scan_id, tgt_scan_ids, n, stream_ids, prm, Support::nearest(prm->normal_k), Support::nearest(prm->feature_k),
                      out_T, out_inliers, out_n_pairs, out_ok);
}

int gloc_reg_fpfh_fgr_batch_ids_radius(gloc_reg* h, uint32_t src_scan_id, const uint32_t* tgt_scan_ids, size_t n, const uint32_t* stream_ids,
                                       const gloc_fgr_params* prm, const gloc_fpfh_radius_params* support, float* out_T,
                                       uint32_t* out_inliers, uint32_t* out_n_pairs, int* out_ok) {
  GLOC_TRY(gloc::fgr::check_params(prm));
  GLOC_TRY(gloc::fpfh::check_radius_params(support));
  GLOC_REQUIRE(h && out_T && tgt_scan_ids, GLOC_ERR_INVALID, "null argument");
  GLOC_NOT_PENDING(h);
  GLOC_HIP(hipSetDevice(h->device));
  return run_fpfh_fgr(h, src_scan_id, tgt_scan_ids, n, stream_ids, prm, Support::normals_of(*support), Support::features_of(*support), out_T,
                      out_inliers, out_n_pairs, out_ok);
}

// (support == NULL: the k-mode features of prm)
int gloc_reg_fpfh_fgr_batch_ids_keypoints(gloc_reg* h, uint32_t src_scan_id, const uint32_t* tgt_scan_ids, size_t n,
                                          const uint32_t* stream_ids, const gloc_fgr_params* prm, const gloc_fpfh_radius_params* support,
                                          const gloc_iss_params* iss, float* out_T, uint32_t* out_inliers, uint32_t* out_n_pairs,
                                          int* out_ok) {
  GLOC_TRY(gloc::fgr::check_params(prm));
  if (support) GLOC_TRY(gloc::fpfh::check_radius_params(support));
  GLOC_TRY(check_iss_params(iss));
  GLOC_REQUIRE(h && out_T && tgt_scan_ids, GLOC_ERR_INVALID, "null argument");
  GLOC_NOT_PENDING(h);
  GLOC_HIP(hipSetDevice(h->device));
  return run_fpfh_fgr(h, src_scan_id, tgt_scan_ids, n, stream_ids, prm, support ? Support::normals_of(*support) : Support::nearest(prm->normal_k),
                      support ? Support::features_of(*support) : Support::nearest(prm->feature_k), out_T, out_inliers, out_n_pairs, out_ok,
                      iss);
}

int gloc_reg_fgr_pairs(gloc_reg* h, const float* P, const float* Q, size_t m, uint32_t stream_id, const gloc_fgr_params* prm,
                       uint32_t* out_mult, uint32_t* out_n_tuples, double* out_d2, double* out_system, float* out_T,
                       uint32_t* out_inliers, int* out_status, int* out_ok) {
  GLOC_TRY(gloc::fgr::check_params(prm));
  GLOC_REQUIRE(h && out_T && ((P && Q) || m == 0), GLOC_ERR_INVALID, "null argument");
  GLOC_REQUIRE(m < (1ull << 31), GLOC_ERR_INVALID, "too many pairs");
  GLOC_NOT_PENDING(h);
  GLOC_HIP(hipSetDevice(h->device));
  return run_fgr_pairs(h, P, Q, m, stream_id, prm, out_mult, out_n_tuples, out_d2, out_system, out_T, out_inliers, out_status, out_ok);
}

int gloc_reg_fpfh_match(gloc_reg* h, const float* src_feat, size_t n_src, const float* tgt_feat, size_t n_tgt, uint32_t mutual,
                        uint32_t* out_idx, float* out_d2) {
  GLOC_REQUIRE(h && out_idx && (src_feat || n_src == 0) && (tgt_feat || n_tgt == 0), GLOC_ERR_INVALID, "null argument");
  GLOC_REQUIRE(n_src < (1ull << 31) && n_tgt < (1ull << 31), GLOC_ERR_INVALID, "too many rows");
  GLOC_NOT_PENDING(h);
  GLOC_HIP(hipSetDevice(h->device));
  for (size_t i = 0; i < n_src; ++i) {
    out_idx[i] = 0xFFFFFFFFu;
    if (out_d2) out_d2[i] = INFINITY;
  }
  if (n_src == 0 || n_tgt == 0) return GLOC_OK;
  GLOC_TRY(ensure_ws(&h->fpfh));
  gloc::fpfh::Ws& w = *h->fpfh;
  hipStream_t s = h->stream;
  const size_t row = sizeof(float) * gloc::fpfh::FEAT_DIM, n_keys = n_src + (mutual ? n_tgt : 0);
  GLOC_TRY(w.feat_a.ensure(row * n_src, s));
  GLOC_TRY(w.feat_b.ensure(row * n_tgt, s));
  GLOC_TRY(w.keys.ensure(sizeof(unsigned long long) * n_keys, s));
  GLOC_HIP(hipMemcpyAsync(w.feat_a.p, src_feat, row * n_src, hipMemcpyHostToDevice, s));
  GLOC_HIP(hipMemcpyAsync(w.feat_b.p, tgt_feat, row * n_tgt, hipMemcpyHostToDevice, s));
  GLOC_HIP(hipMemsetAsync(w.keys.p, 0xFF, sizeof(unsigned long long) * n_keys, s));
  unsigned long long* keys = w.keys.as<unsigned long long>();
  std::vector<gloc::fpfh::MatchTask> tasks;
  tasks.push_back(gloc::fpfh::MatchTask{w.feat_a.as<float>(), nullptr, w.feat_b.as<float>(), nullptr, keys, (uint32_t)n_src, (uint32_t)n_tgt});
  if (mutual)
    tasks.push_back(gloc::fpfh::MatchTask{w.feat_b.as<float>(), nullptr, w.feat_a.as<float>(), nullptr, keys + n_src, (uint32_t)n_tgt, (uint32_t)n_src});
  {
    ProfScope ps(h->prof, "fpfh_match", s);
    GLOC_TRY(gloc::fpfh::match(s, w, tasks));
  }
  std::vector<unsigned long long> hk(n_keys);
  GLOC_HIP(hipMemcpyAsync(hk.data(), w.keys.p, sizeof(unsigned long long) * n_keys, hipMemcpyDeviceToHost, s));
  GLOC_HIP(hipStreamSynchronize(s));
  for (size_t i = 0; i < n_src; ++i) {
    if (hk[i] == ~0ull) continue;
    const uint32_t j = (uint32_t)(hk[i] & 0xFFFFFFFFull), bits = (uint32_t)(hk[i] >> 32);
    if (j >= n_tgt) continue;
    if (mutual && (hk[n_src + j] == ~0ull || (uint32_t)(hk[n_src + j] & 0xFFFFFFFFull) != (uint32_t)i)) continue;
    out_idx[i] = j;
    if (out_d2) memcpy(&out_d2[i], &bits, 4);
  }
  return GLOC_OK;
}

int gloc_reg_profile(gloc_reg* h, const char* kernel, double* total_ms, uint64_t* launches) {
  return handle_profile(h, kernel, total_ms, launches);
}

int gloc_reg_profile_reset(gloc_reg* h) {
  GLOC_TRY(handle_profile_reset(h));
  h->nn_launches = 0;
  if (h->counters.p) GLOC_HIP(hipMemsetAsync(h->counters.p, 0, 8 * NN_STAT_SLOTS, h->stream));
  return GLOC_OK;
}

}  // extern "C"
