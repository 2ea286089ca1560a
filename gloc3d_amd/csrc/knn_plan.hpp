// knn_plan.hpp -- every decision of a coarse (matrix-core) descriptor kNN search, made before anything is launched:
// plan_search() turns the shape of one block of queries into a SearchPlan, and knn.hip's run_mfma() executes it step by
// step.  Host arithmetic on plain integers only -- nothing from HIP is included, so the planner compiles and is tested
// without a GPU (tests/test_knn_plan_cpu.py).  The constants are the kernels' (knn_kernels.hpp includes this header).
#pragma once
#include <stddef.h>

#include <algorithm>

namespace gloc {
namespace knn {

constexpr int MIR_ROWS = 64;  // rows per tile
constexpr int SEL_LIST = 2048;
constexpr int SELQ_THREADS = 1024;
constexpr int SELQ_EPT = 16;                             // keys per thread
constexpr int SELQ_MAX_ROWS = SELQ_THREADS * SELQ_EPT;   // 16 384
constexpr int SELB_MAX_BLOCKS = 64;
constexpr int SELB_LIST = 32 * SELB_MAX_BLOCKS;
constexpr int SRR_KC = 32;
constexpr int SRR_G = 1024;          // groups of 4 dims held per candidate
constexpr int SELECT_ONE_BLOCK_MAX = 16384;  // rows one work-group per query selects from in one launch

// (in 64 bits: a window may hold 2^31 - 1 rows, and rows + tile - 1 does not fit an int there)
inline long long ceil_div(long long a, long long b) { return (a + b - 1) / b; }

// Windows above 16 384 rows: S slices of L rows (a multiple of 64, <= 16 384), one work-group per (slice, query);
// more slices than the window needs while the launch would leave CUs idle.
struct SlicePlan {
  int S, L;
};
inline bool plan_slices(int n_range, int nq, int K, SlicePlan* out) {
  long long s = ceil_div(n_range, SELQ_MAX_ROWS);
  while (s * nq < 512 && n_range / (s * 2) >= 4096 && s * 2 * K <= SELQ_MAX_ROWS) s *= 2;
  const int L = (int)((ceil_div(n_range, s) + 63) & ~63ll);
  const long long S = ceil_div(n_range, L);  // (no empty slice)
  if (S * K > SELQ_MAX_ROWS || S > 65535) return false;  // the lists no longer fit one work-group's registers
  *out = SlicePlan{(int)S, L};
  return true;
}

// Per-query top-K of a window of distances (knn.hip: run_select): over the window itself by one work-group per query,
// over slices and then their lists, or by chunked threshold selection + merge(s).  BlockMinima: only inside the fused
// selection + re-rank of a coarse search (SearchPlan below).
enum class Selection { Window, BlockMinima, Slices, Chunks };
struct SelectPlan {
  Selection form;
  SlicePlan sl;  // Slices only
};
inline SelectPlan plan_select(int n_range, int nq, int K) {
  SelectPlan s{Selection::Chunks, {1, 0}};
  if (n_range <= SELQ_MAX_ROWS && K <= 64) s.form = Selection::Window;  // one launch, one work-group per query
  else if (K <= 64 && plan_slices(n_range, nq, K, &s.sl)) s.form = Selection::Slices;  // two launches: slices, then their lists
  return s;
}

struct MfmaPlan {
  int WQ, NT, KS, BQ, BN;
  int t32 = 0;  // 1: the 32 x 32 x 2 tiles (dist_mfma32_kernel: BQ = 64, BN = 128, one plan)
  int b3 = 0;   // 1: the split-bf16 form (dist_bf16x3_tiled_kernel: BQ = 64, BN = 64 * NT)
};

inline MfmaPlan plan_mfma(int nq, int n_range, int dim, bool fp32_only) {
  // The split-bf16 coarse pass (round 4): the matrix cores stop being the bound, the rows' stream from HBM is.  Tiles of
  // 64 queries x 128 rows when those alone fill the CUs twice, 64 rows otherwise; K split until ~512 work-groups.
  if (!fp32_only && dim % 8 == 0 && dim >= 8) {
    const int qblocks = (nq + 63) / 64;
    const int nt = (ceil_div(n_range, 128) * qblocks >= 512) ? 2 : 1;
    const long long tiles = ceil_div(n_range, 64 * nt) * qblocks;
    int ks = 1;
    while (tiles * ks < 512 && ks < 16 && (dim % (64 * ks * 2)) == 0 && dim / (ks * 2) >= 128) ks *= 2;
    MfmaPlan b{4, nt, ks, 64, 64 * nt};
    b.b3 = 1;
    return b;
  }
  MfmaPlan best{};
  double best_cost = 1e300;
  const int WQ = nq <= 16 ? 1 : (nq <= 32 ? 2 : 4);
  static const int NT4[] = {2, 3, 4, 5, 6, 8}, NT2[] = {2, 4}, NT1[] = {1, 2};
  const int* nts = WQ == 4 ? NT4 : (WQ == 2 ? NT2 : NT1);
  const int n_nts = WQ == 4 ? 6 : 2;
  const int BQ = 16 * WQ;
  const int qblocks = (nq + BQ - 1) / BQ;
  for (int i = 0; i < n_nts; ++i) {
    const int NT = nts[i], BN = 16 * NT * (4 / WQ);
    const long long tiles = ceil_div(n_range, BN) * qblocks;
    // split K only when the tiles alone cannot give every CU a work-group (the partial sums cost
    // KS x Q x N x 8 B of extra traffic and a longer rounding chain)
    int KS = 1;
    // (one block of queries over >= 64 row tiles: two work-groups per CU overlap each other's LDS hand-offs;
    // measured at 64 x 10 000 and 25 x 4541 x 4096: -4 / -3 us; 128 x 16 000 and 32 x 2000: +4 us, so not there)
    const long long want_wgs = (qblocks == 1 && tiles >= 64) ? 400 : 200;
    while (tiles * KS < want_wgs && KS < 16 && (dim % (64 * KS * 2)) == 0 && dim / (KS * 2) >= 128) KS *= 2;
    const int klen = (dim + KS - 1) / KS;
    const long long wgs = tiles * KS;
    const long long rounds = (wgs + 255) / 256;
    // per-WG time ~ klen * (MFMA issue for BN rows + staging of BQ+BN rows)
    const double per_wg = (double)klen * ((double)BN * 1.0 + (double)(BQ + BN) * 0.35);
    const double cost = (double)rounds * per_wg * (1.0 + 0.03 * (KS - 1)) + (wgs < 128 ? 1e7 : 0);
    if (cost < best_cost) {
      best_cost = cost;
      best = MfmaPlan{WQ, NT, KS, BQ, BN};
    }
  }
  // Many rounds of work-groups per CU (a shard of a large database): the 32 x 32 x 2 tiles -- half the LDS operand reads
  // per flop.  Measured at 64 x 125 000 x 4096: 794 us against 922 with the 16 x 16 x 4 tiles (BN = 128, K-step 32, three
  // work-groups per CU).  At 64 x 10 000 the launch is ONE round of work-groups and the tile that divides 10 000 rows
  // into 500 of them (BN = 80, split-K 4) wins: 82 us against 92 - 116 for every 32-wide plan.
  if (nq > 32 && ceil_div(n_range, 128) * ((nq + 63) / 64) >= 3 * 256) {
    best = MfmaPlan{4, 2, 1, 64, 128};
    best.t32 = 1;
  }
  return best;
}

// How the queries whose candidate set could not be proven complete are redone exactly:
//   InLaunch      by their own work-group inside the fused selection + re-rank launch (windows of <= 16 384 rows): no
//                 read-back, no host synchronisation, no further launch
//   OneLaunch     flagged_redo_kernel over redo.sl: every work-group walks the flags and leaves when none is set
//   FlaggedExact  the exact distance pass and run_select(redo), both launched always and leaving at once unless the
//                 query's flag is set
//   HostReadBack  the flags are copied to the host, which runs the exact path per flagged query
enum class Redo { InLaunch, OneLaunch, FlaggedExact, HostReadBack };

// One block of queries (nq <= 1024) against a window of n_range rows.
struct SearchPlan {
  MfmaPlan tile;             // the coarse kernel (b3 / t32 / neither: the fp32 tiles <WQ, NT>) and its tile
  int kps;                   // k per split: whole 64-float steps
  unsigned gx, gy, gz;       // its grid: row tiles (the split-bf16 form: from the head of the window's first mirror tile), query blocks, K splits
  size_t ld, qpad, strideP;  // partial dots [gz][qpad][ld]
  int KC;                    // coarse candidates per query
  bool qraw;                 // split-bf16 form: the work-groups split their queries themselves (else split_queries_kernel, ahead)
  bool use_bmin;             // split-bf16 form: the epilogue leaves block minima ...
  int n_blocks;              // ... of that many blocks of 32 rows
  bool large;                // a window above SELQ_MAX_ROWS rows
  bool fused;                // selection + re-rank + completeness check in ONE launch (select_rerank_kernel), which writes
                             // the result itself; else run_select(sel) and the re-rank kernels
  SelectPlan sel;
  Redo how_redo;
  SelectPlan redo;           // OneLaunch: Slices, the kernel's own; FlaggedExact: run_select's form
  float eps_rel_d, eps_rel_n;
};

// first_in_tile: the window's first row % MIR_ROWS
inline SearchPlan plan_search(int nq, int n_range, int first_in_tile, int dim, int k, int candidates, bool fp32_only) {
  SearchPlan p{};
  const MfmaPlan t = p.tile = plan_mfma(nq, n_range, dim, fp32_only);
  p.KC = std::max(candidates, std::min(64, k + 12));
  p.ld = ((size_t)n_range + 63) & ~(size_t)63;
  p.qpad = (size_t)((nq + t.BQ - 1) / t.BQ) * t.BQ;
  p.strideP = p.qpad * p.ld;
  p.kps = ((dim + t.KS - 1) / t.KS + 63) & ~63;
  p.gx = (unsigned)ceil_div(n_range, t.BN), p.gy = (unsigned)((nq + t.BQ - 1) / t.BQ), p.gz = (unsigned)t.KS;
  if (t.b3) {
    // few work-groups: each splits its queries itself; many: once, ahead of the launch
    p.qraw = (long long)p.gx * p.gy * p.gz <= 768;  // (64 x 125 000, 977 work-groups: 456 us split ahead, 461 in-kernel)
    // (the mirror's tiles are aligned to absolute row numbers: a window that starts inside one computes its leading rows too)
    p.gx = (unsigned)ceil_div((long long)first_in_tile + n_range, t.BN);
    // a large window in one K-split: the epilogue leaves block minima for the selection (select_blocks_body)
    p.n_blocks = (int)p.gx * (t.BN / 32);
    p.use_bmin = n_range > SELQ_MAX_ROWS && t.KS == 1 && p.n_blocks <= SELQ_MAX_ROWS && p.KC <= SRR_KC && dim <= 4 * SRR_G;
  }
  // rounding bound of the coarse distance against the reference-order distance:
  //   reference chain          (D/4 + 4) u d2
  //   MFMA chains of <= 64 fma, nch partial sums, KS split sums, norms (D/64 + 6), 3 final ops
  const float u = 5.9604645e-8f;
  p.eps_rel_d = 1.05f * u * (float)(dim / 4 + 4);
  //   split-bf16 form: the dropped product terms 3.03 * 2^-16 = 776 u (knn_kernels.hpp), and its chains are 3 x 64
  //   products long with the accumulation inside an MFMA priced as truncating adds (2 u each): 384 for the 64
  const float chain_u = t.b3 ? 776.f + 384.f : 64.f;
  p.eps_rel_n = 1.05f * u * (chain_u + (float)((p.kps + 63) / 64 + t.KS + dim / 64 + 6 + 3 + 4));

  // The selection.  Fused: a small window by the launch itself; a large one from the block minima (round 6: 32 x KC partial
  // dots per query, not the window's -- select_blocks_body) or from the lists of slices launched ahead of it.
  p.large = n_range > SELQ_MAX_ROWS;
  SlicePlan sl{1, 0};
  p.fused = (!p.large || p.use_bmin || plan_slices(n_range, nq, p.KC, &sl)) && p.KC <= SRR_KC && dim <= 4 * SRR_G;
  if (p.fused) p.sel = SelectPlan{!p.large ? Selection::Window : (p.use_bmin ? Selection::BlockMinima : Selection::Slices), sl};
  else p.sel = plan_select(n_range, nq, p.KC);

  // The redo.  (A large window goes on to a pass of its own: a work-group per query cannot redo a window of that size.)
  p.redo = SelectPlan{Selection::Window, {1, 0}};
  if (p.fused && !p.large) {
    p.how_redo = Redo::InLaunch;
    return p;
  }
  SlicePlan fb_sl;
  if (!((n_range <= SELECT_ONE_BLOCK_MAX && k <= 2048 / std::max(1, (n_range + 255) / 256)) ||
        (k <= 64 && plan_slices(n_range, nq, k, &fb_sl)))) {
    // windows too large for the device forms (the slices' lists no longer fit one work-group)
    p.how_redo = Redo::HostReadBack;
    return p;
  }
  // Incomplete queries are redone on the exact path ON THE DEVICE: the kernels are always
  // launched and leave at once unless the query's flag is set -- no read-back, no host synchronisation
  // (windows above 16 384 rows too since round 4: the read-back of the flags stalled the launches of a run of searches
  // behind a host synchronisation, ~35 us of a 460-us search over a 125 000-row shard).
  p.how_redo = Redo::FlaggedExact;
  p.redo = plan_select(n_range, nq, k);
  if (p.fused && p.large && k <= 64) {
    // ONE launch (round 6): every work-group walks the flags and leaves when none is set; a flagged query's exact
    // distances, slice selections and final selection happen inside it (flagged_redo_kernel)
    long long S = std::max(1ll, ceil_div(n_range, 2048));
    while (S * k > SELQ_MAX_ROWS) S = (S + 1) / 2;
    const long long L = (ceil_div(n_range, S) + 63) & ~63ll;
    S = ceil_div(n_range, L);  // (no empty slice)
    if (L <= SELQ_MAX_ROWS) {
      p.how_redo = Redo::OneLaunch;
      p.redo = SelectPlan{Selection::Slices, {(int)S, (int)L}};
    }
  }
  return p;
}

}  // namespace knn
}  // namespace gloc
