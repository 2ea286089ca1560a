// pgo.hip -- C ABI of the pose-graph optimisation (include/gloc3d.h, gloc_pgo_*): the checks, the upload of a graph, the
// CSR, and the Levenberg-Marquardt loop around the kernels of pgo_kernels.hpp.  tests/pgo_ref.py is the contract.
//
// Launches.  Per call: fill, the radix sort of the 2 m (node, entry) pairs (3 launches per 8 bits of n - 1), rowstart.
// Per linearisation: linearize, gather, finalize, and one read-back of the Scalars.  Per Levenberg-Marquardt attempt:
// pcg_init, TWO launches per PCG iteration (matvec, update: alpha, beta and the stop test stay on the device), the stop
// flag read back every PCG_CHUNK iterations -- the launches behind a stop inside a chunk leave at once --, retract and a
// linearisation.  Every host loop is bounded by max_iters x (pcg_max_iters + PCG_CHUNK + const).
//
// Memory: both the current and the trial linearisation are resident (36 doubles per edge, 48 per node, each), so a
// rejected step costs nothing to undo.
//
// The closure selection (gloc_pgo_consistency, C1 - C6; pgo_consistency_kernels.hpp, tests/pcm_ref.py) is the second half
// of this file.  Launches per call: pc_setup, pc_pair, pg_score, pc_key, pg_seeds, pc_clique, pc_choose -- seven, ordered by
// the stream alone.  It borrows the optimiser's upload buffers (every optimiser call uploads its own graph again).
#include <algorithm>
#include <cmath>
#include <vector>

#include "common.hpp"
#include "pairgraph.hpp"
#include "pgo.hpp"
#include "pgo_consistency_kernels.hpp"
#include "pgo_kernels.hpp"
#include "seg_sort.hpp"

using namespace gloc;
using namespace gloc::pgo;

namespace {
constexpr uint32_t PCG_CHUNK = 16;
enum { PART_F, PART_GINF, PART_DEN, PART_W, PART_V, PART_RR0, PART_RR1, PART_RZ0, PART_RZ1, PART_G2, PART_PAP, N_PARTS };
}  // namespace

struct gloc_pgo : Handle {
  DevBuf P[2], fixed, free_, src, tgt, Zf, Om, mask, key[2], val[2], seg, hist, row;
  DevBuf lin_e[2], lin_n[2], bad, vec, parts, sc;
  std::vector<double> hP, hOm, hd;
  std::vector<float> hZ;
  std::vector<uint8_t> hmask;
  // the closure selection's
  DevBuf c_ops, c_status, c_path, c_count, c_bits, c_s2, c_score, c_degree, c_key, c_seeds, c_sizes, c_members, c_counts, c_res, c_mask;
  // of the call in progress
  uint32_t n = 0, m = 0, ge = 0, gm = 0, gu = 0, kind = 0;
  double c2 = 1.0, origin[3] = {0, 0, 0};
  bool any_free = false;
  const uint32_t* csr = nullptr;
  Lin lin(int s) const {
    Lin L;
    double* e = lin_e[s].as<double>();
    double* v = lin_n[s].as<double>();
    const size_t mm = m, nn = n;
    L.r = e, L.s2 = e + 6 * mm, L.w = e + 7 * mm, L.rho = e + 8 * mm, L.W = e + 9 * mm, L.b = e + 30 * mm;
    L.g = v, L.Hd = v + 6 * nn, L.Lf = v + 27 * nn;
    L.bad = bad.as<uint32_t>() + s;
    return L;
  }
  double* part(int which) const { return parts.as<double>() + (size_t)which * MAX_GRID; }
};

namespace gloc {
namespace pgo {

int check_params(const gloc_pgo_params* p) {
  GLOC_REQUIRE(p, GLOC_ERR_INVALID, "params is null");
  GLOC_REQUIRE(p->max_iters >= 1, GLOC_ERR_INVALID, "max_iters = 0");
  GLOC_REQUIRE(p->pcg_max_iters >= 1, GLOC_ERR_INVALID, "pcg_max_iters = 0");
  GLOC_REQUIRE(std::isfinite(p->lambda_init) && p->lambda_init > 0.0, GLOC_ERR_INVALID, "lambda_init = %g must be > 0 and finite", p->lambda_init);
  GLOC_REQUIRE(std::isfinite(p->pcg_tol) && p->pcg_tol > 0.0, GLOC_ERR_INVALID, "pcg_tol = %g must be > 0 and finite", p->pcg_tol);
  GLOC_REQUIRE(std::isfinite(p->rot_eps) && p->rot_eps >= 0.0, GLOC_ERR_INVALID, "rot_eps = %g must be >= 0 and finite", p->rot_eps);
  GLOC_REQUIRE(std::isfinite(p->trans_eps) && p->trans_eps >= 0.0, GLOC_ERR_INVALID, "trans_eps = %g must be >= 0 and finite", p->trans_eps);
  GLOC_REQUIRE(std::isfinite(p->grad_eps) && p->grad_eps >= 0.0, GLOC_ERR_INVALID, "grad_eps = %g must be >= 0 and finite", p->grad_eps);
  GLOC_REQUIRE(p->reserved_[0] == 0 && p->reserved_[1] == 0, GLOC_ERR_INVALID, "reserved_ must be 0");
  return GLOC_OK;
}

int check_robust(const gloc_robust_params* r) {
  if (!r) return GLOC_OK;
  GLOC_TRY(robust::check_params(r));
  GLOC_REQUIRE(r->kind == GLOC_ROBUST_NONE || r->scale_start == 0.f, GLOC_ERR_INVALID,
               "a robust schedule (scale_start = %g) has no single objective to accept steps against", (double)r->scale_start);
  return GLOC_OK;
}

int check_graph(const Graph& g) {
  GLOC_REQUIRE(g.n >= 2 && g.n <= MAX_NODES, GLOC_ERR_INVALID, "n = %zu nodes outside [2, 2^20]", g.n);
  GLOC_REQUIRE(g.m >= 1 && g.m <= MAX_EDGES, GLOC_ERR_INVALID, "m = %zu edges outside [1, 2^22]", g.m);
  for (size_t e = 0; e < g.m; ++e)
    GLOC_REQUIRE(g.src[e] < g.n && g.tgt[e] < g.n, GLOC_ERR_INVALID, "edge %zu has an end (%u, %u) beyond the %zu nodes", e, g.src[e], g.tgt[e], g.n);
  for (size_t e = 0; e < g.m; ++e) GLOC_REQUIRE(g.src[e] != g.tgt[e], GLOC_ERR_INVALID, "edge %zu joins node %u to itself", e, g.src[e]);
  bool any = false;
  for (size_t k = 0; k < g.n && !any; ++k) any = g.fixed[k] != 0;
  GLOC_REQUIRE(any, GLOC_ERR_INVALID, "no fixed node");
  for (size_t i = 0; i < 16 * g.n; ++i) GLOC_REQUIRE(std::isfinite(g.poses[i]), GLOC_ERR_INVALID, "pose %zu is not finite", i / 16);
  for (size_t i = 0; i < 16 * g.m; ++i) GLOC_REQUIRE(std::isfinite(g.Z[i]), GLOC_ERR_INVALID, "Z of edge %zu is not finite", i / 16);
  for (size_t i = 0; i < 36 * g.m; ++i) GLOC_REQUIRE(std::isfinite(g.info[i]), GLOC_ERR_INVALID, "info of edge %zu is not finite", i / 36);
  return GLOC_OK;
}

}  // namespace pgo
}  // namespace gloc

namespace {

int check_all(const gloc_pgo* h, const Graph& g, const gloc_pgo_params* prm, const gloc_robust_params* rob, bool outputs) {
  GLOC_TRY(check_params(prm));
  GLOC_TRY(check_robust(rob));
  GLOC_REQUIRE(g.poses && g.fixed && g.src && g.tgt && g.Z && g.info && outputs, GLOC_ERR_INVALID, "null argument");
  GLOC_TRY(check_graph(g));
  GLOC_REQUIRE(h, GLOC_ERR_INVALID, "null handle");
  return GLOC_OK;
}

#define PGO_LAUNCH(name, kernel, grid, ...)                                              \
  do {                                                                                   \
    ProfScope ps_(h->prof, name, s);                                                     \
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(THREADS), 0, s, __VA_ARGS__);            \
    GLOC_HIP(hipGetLastError());                                                         \
  } while (0)

// the graph onto the device (poses into P[0], relative to the first fixed node), the CSR, the free flags
int prepare(gloc_pgo* h, const Graph& g, const gloc_robust_params* rob) {
  hipStream_t s = h->stream;
  const size_t n = g.n, m = g.m;
  h->n = (uint32_t)n, h->m = (uint32_t)m;
  h->ge = (uint32_t)std::min<size_t>((m + THREADS - 1) / THREADS, MAX_GRID);
  h->gm = (uint32_t)std::min<size_t>((n + WAVES - 1) / WAVES, MAX_GRID);
  h->gu = (uint32_t)std::min<size_t>((n + THREADS - 1) / THREADS, MAX_GRID);
  h->kind = rob ? rob->kind : (uint32_t)GLOC_ROBUST_NONE;
  h->c2 = h->kind ? (double)rob->scale * (double)rob->scale : 1.0;
  size_t f0 = 0;
  while (!g.fixed[f0]) ++f0;
  for (int a = 0; a < 3; ++a) h->origin[a] = g.poses[16 * f0 + 4 * a + 3];
  std::vector<uint32_t> deg(n, 0);
  for (size_t e = 0; e < m; ++e) ++deg[g.src[e]], ++deg[g.tgt[e]];
  h->any_free = false;
  for (size_t k = 0; k < n; ++k) h->any_free = h->any_free || (!g.fixed[k] && deg[k]);
  h->hP.resize(12 * n), h->hZ.resize(12 * m), h->hOm.resize(21 * m), h->hmask.assign(m, 1);
  for (size_t k = 0; k < n; ++k)
    for (int a = 0; a < 3; ++a) {
      for (int b = 0; b < 3; ++b) h->hP[12 * k + 3 * a + b] = g.poses[16 * k + 4 * a + b];
      h->hP[12 * k + 9 + a] = g.poses[16 * k + 4 * a + 3] - h->origin[a];
    }
  for (size_t e = 0; e < m; ++e) {
    for (int a = 0; a < 3; ++a) {
      for (int b = 0; b < 3; ++b) h->hZ[(size_t)(3 * a + b) * m + e] = g.Z[16 * e + 4 * a + b];
      h->hZ[(size_t)(9 + a) * m + e] = g.Z[16 * e + 4 * a + 3];
    }
    for (int a = 0; a < 6; ++a)
      for (int b = a; b < 6; ++b) h->hOm[(size_t)ut(a, b) * m + e] = g.info[36 * e + 6 * a + b];
    if (g.mask) h->hmask[e] = g.mask[e] ? 1 : 0;
  }
  GLOC_TRY(h->P[0].ensure(sizeof(double) * 12 * n, s));
  GLOC_TRY(h->P[1].ensure(sizeof(double) * 12 * n, s));
  GLOC_TRY(h->fixed.ensure(n, s));
  GLOC_TRY(h->free_.ensure(n, s));
  GLOC_TRY(h->src.ensure(sizeof(uint32_t) * m, s));
  GLOC_TRY(h->tgt.ensure(sizeof(uint32_t) * m, s));
  GLOC_TRY(h->Zf.ensure(sizeof(float) * 12 * m, s));
  GLOC_TRY(h->Om.ensure(sizeof(double) * 21 * m, s));
  GLOC_TRY(h->mask.ensure(m, s));
  for (int i = 0; i < 2; ++i) {
    GLOC_TRY(h->key[i].ensure(sizeof(uint32_t) * 2 * m, s));
    GLOC_TRY(h->val[i].ensure(sizeof(uint32_t) * 2 * m, s));
    GLOC_TRY(h->lin_e[i].ensure(sizeof(double) * 36 * m, s));
    GLOC_TRY(h->lin_n[i].ensure(sizeof(double) * 48 * n, s));
  }
  GLOC_TRY(h->seg.ensure(sizeof(segsort::Seg), s));
  GLOC_TRY(h->hist.ensure(segsort::scratch_bytes(1, (uint32_t)(2 * m)), s));
  GLOC_TRY(h->row.ensure(sizeof(uint32_t) * (n + 1), s));
  GLOC_TRY(h->bad.ensure(sizeof(uint32_t) * 2, s));
  GLOC_TRY(h->vec.ensure(sizeof(double) * 6 * 6 * n, s));  // x, r, z, Ap, p[2]
  GLOC_TRY(h->parts.ensure(sizeof(double) * N_PARTS * MAX_GRID, s));
  GLOC_TRY(h->sc.ensure(sizeof(Scalars), s));
  GLOC_HIP(hipMemcpyAsync(h->P[0].p, h->hP.data(), sizeof(double) * 12 * n, hipMemcpyHostToDevice, s));
  GLOC_HIP(hipMemcpyAsync(h->fixed.p, g.fixed, n, hipMemcpyHostToDevice, s));
  GLOC_HIP(hipMemcpyAsync(h->src.p, g.src, sizeof(uint32_t) * m, hipMemcpyHostToDevice, s));
  GLOC_HIP(hipMemcpyAsync(h->tgt.p, g.tgt, sizeof(uint32_t) * m, hipMemcpyHostToDevice, s));
  GLOC_HIP(hipMemcpyAsync(h->Zf.p, h->hZ.data(), sizeof(float) * 12 * m, hipMemcpyHostToDevice, s));
  GLOC_HIP(hipMemcpyAsync(h->Om.p, h->hOm.data(), sizeof(double) * 21 * m, hipMemcpyHostToDevice, s));
  GLOC_HIP(hipMemcpyAsync(h->mask.p, h->hmask.data(), m, hipMemcpyHostToDevice, s));
  const segsort::Seg seg{0u, (uint32_t)(2 * m)};
  GLOC_HIP(hipMemcpyAsync(h->seg.p, &seg, sizeof(seg), hipMemcpyHostToDevice, s));
  GLOC_HIP(hipMemsetAsync(h->parts.p, 0, sizeof(double) * N_PARTS * MAX_GRID, s));
  GLOC_HIP(hipMemsetAsync(h->sc.p, 0, sizeof(Scalars), s));
  GLOC_HIP(hipMemsetAsync(h->bad.p, 0, sizeof(uint32_t) * 2, s));
  GLOC_HIP(hipStreamSynchronize(s));  // (`seg` is on this frame)
  {
    ProfScope ps(h->prof, "pgo_setup", s);
    const uint32_t cnt = (uint32_t)(2 * m);
    hipLaunchKernelGGL(fill_kernel, dim3((cnt + THREADS - 1) / THREADS), dim3(THREADS), 0, s, h->src.as<uint32_t>(), h->tgt.as<uint32_t>(), (uint32_t)m,
                       h->key[0].as<uint32_t>(), h->val[0].as<uint32_t>());
    int bits = 1;
    while (bits < 32 && ((n - 1) >> bits)) ++bits;
    const int at = segsort::sort_pairs<uint32_t, 8>(s, h->key[0].as<uint32_t>(), h->key[1].as<uint32_t>(), h->val[0].as<uint32_t>(), h->val[1].as<uint32_t>(),
                                                    h->seg.as<segsort::Seg>(), 1, cnt, 0, bits, h->hist.as<uint32_t>());
    h->csr = h->val[at].as<uint32_t>();
    hipLaunchKernelGGL(rowstart_kernel, dim3((uint32_t)((n + 1 + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, h->key[at].as<uint32_t>(), cnt, (uint32_t)n,
                       h->fixed.as<uint8_t>(), h->row.as<uint32_t>(), h->free_.as<uint8_t>());
    GLOC_HIP(hipGetLastError());
  }
  return GLOC_OK;
}

// the linearisation `set` at the poses P, and its scalars on the host
int linearize(gloc_pgo* h, int set, const double* P, Scalars* out) {
  hipStream_t s = h->stream;
  const Lin L = h->lin(set);
  GLOC_HIP(hipMemsetAsync(L.bad, 0, sizeof(uint32_t), s));
  PGO_LAUNCH("pgo_linearize", linearize_kernel, h->ge, h->m, h->src.as<uint32_t>(), h->tgt.as<uint32_t>(), h->Zf.as<float>(), h->Om.as<double>(),
             h->mask.as<uint8_t>(), h->kind, h->c2, P, L, h->part(PART_F));
  PGO_LAUNCH("pgo_gather", gather_kernel, h->gm, h->n, h->m, h->row.as<uint32_t>(), h->csr, h->free_.as<uint8_t>(), L, h->part(PART_GINF));
  PGO_LAUNCH("pgo_step", finalize_kernel, 1, L, h->part(PART_F), h->ge, h->part(PART_GINF), h->gm, h->part(PART_DEN), h->part(PART_W), h->part(PART_V),
             h->gu, h->sc.as<Scalars>());
  GLOC_HIP(hipMemcpyAsync(out, h->sc.p, sizeof(Scalars), hipMemcpyDeviceToHost, s));
  GLOC_HIP(hipStreamSynchronize(s));
  return GLOC_OK;
}

Pcg pcg_of(const gloc_pgo* h) {
  Pcg c;
  double* v = h->vec.as<double>();
  const size_t n6 = 6 * (size_t)h->n;
  c.x = v, c.r = v + n6, c.z = v + 2 * n6, c.Ap = v + 3 * n6, c.p[0] = v + 4 * n6, c.p[1] = v + 5 * n6;
  c.part_rr[0] = h->part(PART_RR0), c.part_rr[1] = h->part(PART_RR1), c.part_rz[0] = h->part(PART_RZ0), c.part_rz[1] = h->part(PART_RZ1);
  c.part_g2 = h->part(PART_G2), c.part_pAp = h->part(PART_PAP);
  c.sc = h->sc.as<Scalars>();
  c.gu = h->gu, c.gm = h->gm;
  return c;
}

// (H + lambda D) x = -g of the linearisation `set`: x in the PCG's vectors
int solve(gloc_pgo* h, int set, double lambda, const gloc_pgo_params* prm) {
  hipStream_t s = h->stream;
  const Lin L = h->lin(set);
  const Pcg c = pcg_of(h);
  const double tol2 = prm->pcg_tol * prm->pcg_tol;
  const uint8_t* fr = h->free_.as<uint8_t>();
  PGO_LAUNCH("pgo_pcg", pcg_init_kernel, h->gu, h->n, fr, L, lambda, c);
  for (uint32_t it = 0; it < prm->pcg_max_iters;) {
    const uint32_t end = std::min(prm->pcg_max_iters, it + PCG_CHUNK);
    for (; it < end; ++it) {
      PGO_LAUNCH("pgo_pcg", pcg_matvec_kernel, h->gm, h->n, h->m, it, lambda, tol2, h->row.as<uint32_t>(), h->csr, h->src.as<uint32_t>(),
                 h->tgt.as<uint32_t>(), fr, L, c);
      PGO_LAUNCH("pgo_pcg", pcg_update_kernel, h->gu, h->n, it, lambda, tol2, fr, L, c);
    }
    uint32_t stop = 0;
    GLOC_HIP(hipMemcpyAsync(&stop, &c.sc->pcg_stop, sizeof(stop), hipMemcpyDeviceToHost, s));
    GLOC_HIP(hipStreamSynchronize(s));
    if (stop) break;
  }
  return GLOC_OK;
}

int download(gloc_pgo* h, const void* d, std::vector<double>& to, size_t count) {
  to.resize(count);
  GLOC_HIP(hipMemcpyAsync(to.data(), d, sizeof(double) * count, hipMemcpyDeviceToHost, h->stream));
  GLOC_HIP(hipStreamSynchronize(h->stream));
  return GLOC_OK;
}

// s2 and the weights of the linearisation `set`
int edge_outputs(gloc_pgo* h, int set, double* out_s2, double* out_weight) {
  const Lin L = h->lin(set);
  if (out_s2) {
    GLOC_TRY(download(h, L.s2, h->hd, h->m));
    std::copy(h->hd.begin(), h->hd.end(), out_s2);
  }
  if (out_weight) {
    GLOC_TRY(download(h, L.w, h->hd, h->m));
    std::copy(h->hd.begin(), h->hd.end(), out_weight);
  }
  return GLOC_OK;
}

}  // namespace

extern "C" {

void gloc_pgo_default_params(gloc_pgo_params* p) {
  if (!p) return;
  p->max_iters = 50;
  p->pcg_max_iters = 200;
  p->lambda_init = 1e-4;  // Ceres' initial trust radius, inverted
  p->pcg_tol = 1e-8;
  p->rot_eps = 1e-6;
  p->trans_eps = 1e-6;
  p->grad_eps = 1e-6;
  p->reserved_[0] = p->reserved_[1] = 0;
}

int gloc_pgo_create(int device, gloc_pgo** out) { return create_handle(device, out); }
int gloc_pgo_destroy(gloc_pgo* h) { return destroy_handle(h); }
int gloc_pgo_set_stream(gloc_pgo* h, void* hip_stream) { return handle_set_stream(h, hip_stream); }
int gloc_pgo_synchronize(gloc_pgo* h) { return handle_synchronize(h); }
int gloc_pgo_set_profile(gloc_pgo* h, int enable) { return handle_set_profile(h, enable); }
int gloc_pgo_profile(gloc_pgo* h, const char* kernel, double* total_ms, uint64_t* launches) { return handle_profile(h, kernel, total_ms, launches); }
int gloc_pgo_profile_reset(gloc_pgo* h) { return handle_profile_reset(h); }

int gloc_pgo_linearize(gloc_pgo* h, const double* poses, const uint8_t* fixed, size_t n, const uint32_t* edge_src, const uint32_t* edge_tgt, const float* Z,
                       const double* info, const uint8_t* robust_mask, size_t m, const gloc_pgo_params* prm, const gloc_robust_params* robust,
                       double* out_r6, double* out_s2, double* out_weight, double* out_g6, double* out_Hdiag36, double* out_cost) {
  const Graph g{poses, fixed, n, edge_src, edge_tgt, Z, info, robust_mask, m};
  GLOC_TRY(check_all(h, g, prm, robust, out_r6 || out_s2 || out_weight || out_g6 || out_Hdiag36 || out_cost));
  GLOC_HIP(hipSetDevice(h->device));
  GLOC_TRY(prepare(h, g, robust));
  Scalars sc;
  GLOC_TRY(linearize(h, 0, h->P[0].as<double>(), &sc));
  const Lin L = h->lin(0);
  if (out_r6) {
    GLOC_TRY(download(h, L.r, h->hd, 6 * m));
    for (size_t e = 0; e < m; ++e)
      for (int a = 0; a < 6; ++a) out_r6[6 * e + a] = h->hd[(size_t)a * m + e];
  }
  GLOC_TRY(edge_outputs(h, 0, out_s2, out_weight));
  if (out_g6) {
    GLOC_TRY(download(h, L.g, h->hd, 6 * n));
    std::copy(h->hd.begin(), h->hd.end(), out_g6);
  }
  if (out_Hdiag36) {
    GLOC_TRY(download(h, L.Hd, h->hd, 21 * n));
    for (size_t k = 0; k < n; ++k)
      for (int a = 0; a < 6; ++a)
        for (int b = 0; b < 6; ++b) out_Hdiag36[36 * k + 6 * a + b] = h->hd[21 * k + (a <= b ? ut(a, b) : ut(b, a))];
  }
  if (out_cost) *out_cost = sc.F;
  return GLOC_OK;
}

int gloc_pgo_optimize(gloc_pgo* h, const double* poses, const uint8_t* fixed, size_t n, const uint32_t* edge_src, const uint32_t* edge_tgt, const float* Z,
                      const double* info, const uint8_t* robust_mask, size_t m, const gloc_pgo_params* prm, const gloc_robust_params* robust,
                      double* out_poses, double* out_s2, double* out_weight, gloc_pgo_result* out) {
  const Graph g{poses, fixed, n, edge_src, edge_tgt, Z, info, robust_mask, m};
  GLOC_TRY(check_all(h, g, prm, robust, out_poses && out));
  GLOC_HIP(hipSetDevice(h->device));
  GLOC_TRY(prepare(h, g, robust));
  hipStream_t s = h->stream;
  int cur = 0;
  Scalars sc;
  GLOC_TRY(linearize(h, cur, h->P[cur].as<double>(), &sc));
  double F = sc.F, ginf = sc.ginf, lambda = prm->lambda_init, nu = 2.0;
  bool bad = sc.bad != 0;
  gloc_pgo_result res{};
  res.cost_initial = F;
  uint32_t pcg_iters = 0;
  if (!h->any_free) {
    res.status = 2;
  } else if (prm->grad_eps > 0.0 && ginf <= prm->grad_eps) {
    res.status = 3;
  } else {
    for (uint32_t it = 0; it < prm->max_iters; ++it) {
      ++res.iters;
      if (bad) {
        res.status = 2;
        break;
      }
      GLOC_TRY(solve(h, cur, lambda, prm));
      const Pcg c = pcg_of(h);
      PGO_LAUNCH("pgo_step", retract_kernel, h->gu, h->n, h->free_.as<uint8_t>(), c.x, h->lin(cur), lambda, h->P[cur].as<double>(), h->P[cur ^ 1].as<double>(),
                 h->part(PART_DEN), h->part(PART_W), h->part(PART_V));
      GLOC_TRY(linearize(h, cur ^ 1, h->P[cur ^ 1].as<double>(), &sc));
      pcg_iters = sc.pcg_iters;
      const double gain = sc.denom != 0.0 ? (F - sc.F) / sc.denom : -1.0;
      if (gain > 0.0 && std::isfinite(sc.F)) {
        cur ^= 1;
        F = sc.F, ginf = sc.ginf, bad = sc.bad != 0;
        ++res.accepted;
        const double q = 2.0 * gain - 1.0;
        lambda *= std::max(1.0 / 3.0, 1.0 - q * q * q);
        nu = 2.0;
        if (prm->rot_eps > 0.0 && prm->trans_eps > 0.0 && sc.max_w <= prm->rot_eps && sc.max_v <= prm->trans_eps) {
          res.status = 1;
          break;
        }
        if (prm->grad_eps > 0.0 && ginf <= prm->grad_eps) {
          res.status = 3;
          break;
        }
      } else {
        lambda *= nu;
        nu *= 2.0;
      }
    }
  }
  res.pcg_iters = pcg_iters;
  res.cost_final = F, res.lambda = lambda, res.grad_inf = ginf;
  GLOC_TRY(download(h, h->P[cur].p, h->hd, 12 * n));
  std::vector<uint32_t> deg(n, 0);
  for (size_t e = 0; e < m; ++e) ++deg[edge_src[e]], ++deg[edge_tgt[e]];
  for (size_t k = 0; k < n; ++k) {
    if (fixed[k] || !deg[k]) {  // bit for bit
      std::copy(poses + 16 * k, poses + 16 * (k + 1), out_poses + 16 * k);
      continue;
    }
    for (int a = 0; a < 3; ++a) {
      for (int b = 0; b < 3; ++b) out_poses[16 * k + 4 * a + b] = h->hd[12 * k + 3 * a + b];
      out_poses[16 * k + 4 * a + 3] = h->hd[12 * k + 9 + a] + h->origin[a];
    }
    out_poses[16 * k + 12] = out_poses[16 * k + 13] = out_poses[16 * k + 14] = 0.0;
    out_poses[16 * k + 15] = 1.0;
  }
  GLOC_TRY(edge_outputs(h, cur, out_s2, out_weight));
  *out = res;
  return GLOC_OK;
}

}  // extern "C"

// ---- the closure selection ------------------------------------------------------------------------------------------------
namespace {

struct Closures {
  const double* poses;
  size_t n;
  const uint32_t *src, *tgt;
  const float* Z;
  const double *info, *path;
  size_t L;
};

int check_consistency(const gloc_pgo* h, const Closures& c, const gloc_pgo_consistency_params* p, bool outputs, bool want_s2) {
  GLOC_REQUIRE(p, GLOC_ERR_INVALID, "params is null");
  GLOC_REQUIRE(std::isfinite(p->chi2) && p->chi2 > 0.0, GLOC_ERR_INVALID, "chi2 = %g must be > 0 and finite", p->chi2);
  GLOC_REQUIRE(std::isfinite(p->drift_rot) && p->drift_rot >= 0.0, GLOC_ERR_INVALID, "drift_rot = %g must be >= 0 and finite", p->drift_rot);
  GLOC_REQUIRE(std::isfinite(p->drift_trans) && p->drift_trans >= 0.0, GLOC_ERR_INVALID, "drift_trans = %g must be >= 0 and finite", p->drift_trans);
  GLOC_REQUIRE(p->n_seeds >= 1 && p->n_seeds <= 1024, GLOC_ERR_INVALID, "n_seeds = %u outside [1, 1024]", p->n_seeds);
  GLOC_REQUIRE(p->reserved_[0] == 0 && p->reserved_[1] == 0, GLOC_ERR_INVALID, "reserved_ must be 0");
  GLOC_REQUIRE(c.poses && c.src && c.tgt && c.Z && c.info && outputs, GLOC_ERR_INVALID, "null argument");
  GLOC_REQUIRE(c.n >= 2 && c.n <= MAX_NODES, GLOC_ERR_INVALID, "n = %zu nodes outside [2, 2^20]", c.n);
  GLOC_REQUIRE(c.L >= 1 && c.L <= PC_MAX_L, GLOC_ERR_INVALID, "L = %zu closures outside [1, 16384]", c.L);
  GLOC_REQUIRE(!want_s2 || c.L <= PC_MAX_S2_L, GLOC_ERR_INVALID, "out_s2 is refused for L = %zu > 4096 closures", c.L);
  for (size_t a = 0; a < c.L; ++a)
    GLOC_REQUIRE(c.src[a] < c.n && c.tgt[a] < c.n, GLOC_ERR_INVALID, "closure %zu has an end (%u, %u) beyond the %zu nodes", a, c.src[a], c.tgt[a], c.n);
  for (size_t a = 0; a < c.L; ++a) GLOC_REQUIRE(c.src[a] != c.tgt[a], GLOC_ERR_INVALID, "closure %zu joins node %u to itself", a, c.src[a]);
  for (size_t i = 0; i < 16 * c.n; ++i) GLOC_REQUIRE(std::isfinite(c.poses[i]), GLOC_ERR_INVALID, "pose %zu is not finite", i / 16);
  for (size_t i = 0; i < 16 * c.L; ++i) GLOC_REQUIRE(std::isfinite(c.Z[i]), GLOC_ERR_INVALID, "Z of closure %zu is not finite", i / 16);
  for (size_t i = 0; i < 36 * c.L; ++i) GLOC_REQUIRE(std::isfinite(c.info[i]), GLOC_ERR_INVALID, "info of closure %zu is not finite", i / 36);
  if (c.path)
    for (size_t k = 0; k < c.n; ++k) GLOC_REQUIRE(std::isfinite(c.path[k]), GLOC_ERR_INVALID, "path of node %zu is not finite", k);
  GLOC_REQUIRE(h, GLOC_ERR_INVALID, "null handle");
  return GLOC_OK;
}

template <class T>
int fetch(gloc_pgo* h, const DevBuf& d, T* to, size_t count) {
  if (!to) return GLOC_OK;
  GLOC_HIP(hipMemcpyAsync(to, d.p, sizeof(T) * count, hipMemcpyDeviceToHost, h->stream));
  return GLOC_OK;
}

}  // namespace

extern "C" {

void gloc_pgo_consistency_default_params(gloc_pgo_consistency_params* p) {
  if (!p) return;
  p->chi2 = 16.8119;  // the 99 % quantile of chi-squared with 6 degrees of freedom
  p->drift_rot = 0.0;
  p->drift_trans = 0.0;
  p->n_seeds = 64;
  p->min_clique = 2;
  p->reserved_[0] = p->reserved_[1] = 0;
}

int gloc_pgo_consistency(gloc_pgo* h, const double* poses, size_t n, const uint32_t* src, const uint32_t* tgt, const float* Z, const double* info,
                         const double* path, size_t L, const gloc_pgo_consistency_params* prm, uint8_t* out_mask, uint32_t* out_clique_size,
                         uint32_t* out_winner_rank, uint32_t* out_ok, uint8_t* out_status, uint32_t* out_degree, uint64_t* out_score,
                         uint32_t* out_seeds, uint32_t* out_clique_sizes, double* out_s2) {
  const Closures c{poses, n, src, tgt, Z, info, path, L};
  GLOC_TRY(check_consistency(h, c, prm,
                             out_mask || out_clique_size || out_winner_rank || out_ok || out_status || out_degree || out_score || out_seeds ||
                                 out_clique_sizes || out_s2,
                             out_s2 != nullptr));
  GLOC_HIP(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  const uint32_t Lu = (uint32_t)L, words = (Lu + 63u) / 64u, S = prm->n_seeds;
  // the upload: the optimiser's layouts (prepare) for poses, Z and Omega; a closure's two path coordinates
  h->hP.resize(12 * n), h->hZ.resize(12 * L), h->hOm.resize(21 * L), h->hd.assign(2 * L, 0.0);
  for (size_t k = 0; k < n; ++k)
    for (int a = 0; a < 3; ++a) {
      for (int b = 0; b < 3; ++b) h->hP[12 * k + 3 * a + b] = poses[16 * k + 4 * a + b];
      h->hP[12 * k + 9 + a] = poses[16 * k + 4 * a + 3] - poses[4 * a + 3];
    }
  for (size_t e = 0; e < L; ++e) {
    for (int a = 0; a < 3; ++a) {
      for (int b = 0; b < 3; ++b) h->hZ[(size_t)(3 * a + b) * L + e] = Z[16 * e + 4 * a + b];
      h->hZ[(size_t)(9 + a) * L + e] = Z[16 * e + 4 * a + 3];
    }
    for (int a = 0; a < 6; ++a)
      for (int b = a; b < 6; ++b) h->hOm[(size_t)ut(a, b) * L + e] = info[36 * e + 6 * a + b];
    if (path) h->hd[e] = path[src[e]], h->hd[L + e] = path[tgt[e]];
  }
  GLOC_TRY(h->P[0].ensure(sizeof(double) * 12 * n, s));
  GLOC_TRY(h->src.ensure(sizeof(uint32_t) * L, s));
  GLOC_TRY(h->tgt.ensure(sizeof(uint32_t) * L, s));
  GLOC_TRY(h->Zf.ensure(sizeof(float) * 12 * L, s));
  GLOC_TRY(h->Om.ensure(sizeof(double) * 21 * L, s));
  GLOC_TRY(h->c_path.ensure(sizeof(double) * 2 * L, s));
  GLOC_TRY(h->c_ops.ensure(sizeof(double) * PC_OPS * L, s));
  GLOC_TRY(h->c_status.ensure(L, s));
  GLOC_TRY(h->c_count.ensure(sizeof(uint32_t), s));
  GLOC_TRY(h->c_bits.ensure(sizeof(unsigned long long) * L * words, s));
  if (out_s2) GLOC_TRY(h->c_s2.ensure(sizeof(double) * L * L, s));
  GLOC_TRY(h->c_score.ensure(sizeof(unsigned long long) * L, s));
  GLOC_TRY(h->c_degree.ensure(sizeof(uint32_t) * L, s));
  GLOC_TRY(h->c_key.ensure(sizeof(unsigned long long) * L, s));
  GLOC_TRY(h->c_seeds.ensure(sizeof(uint32_t) * S, s));
  GLOC_TRY(h->c_sizes.ensure(sizeof(uint32_t) * S, s));
  GLOC_TRY(h->c_members.ensure(sizeof(unsigned long long) * S * words, s));
  GLOC_TRY(h->c_counts.ensure(sizeof(uint32_t) * S * L, s));
  GLOC_TRY(h->c_res.ensure(sizeof(uint32_t) * 4, s));
  GLOC_TRY(h->c_mask.ensure(L, s));
  GLOC_HIP(hipMemcpyAsync(h->P[0].p, h->hP.data(), sizeof(double) * 12 * n, hipMemcpyHostToDevice, s));
  GLOC_HIP(hipMemcpyAsync(h->src.p, src, sizeof(uint32_t) * L, hipMemcpyHostToDevice, s));
  GLOC_HIP(hipMemcpyAsync(h->tgt.p, tgt, sizeof(uint32_t) * L, hipMemcpyHostToDevice, s));
  GLOC_HIP(hipMemcpyAsync(h->Zf.p, h->hZ.data(), sizeof(float) * 12 * L, hipMemcpyHostToDevice, s));
  GLOC_HIP(hipMemcpyAsync(h->Om.p, h->hOm.data(), sizeof(double) * 21 * L, hipMemcpyHostToDevice, s));
  GLOC_HIP(hipMemcpyAsync(h->c_path.p, h->hd.data(), sizeof(double) * 2 * L, hipMemcpyHostToDevice, s));
  GLOC_HIP(hipMemcpyAsync(h->c_count.p, &Lu, sizeof(uint32_t), hipMemcpyHostToDevice, s));
  GLOC_HIP(hipStreamSynchronize(s));  // (`Lu` is on this frame, the vectors are pageable)
  const uint32_t gl = (Lu + THREADS - 1) / THREADS;
  unsigned long long* bits = h->c_bits.as<unsigned long long>();
  {
    ProfScope ps(h->prof, "pgo_consistency", s, ProfScope::Apart, "pgo_consistency_pairs");
    hipLaunchKernelGGL(pc_setup_kernel, dim3(gl), dim3(THREADS), 0, s, Lu, h->src.as<uint32_t>(), h->tgt.as<uint32_t>(), h->Zf.as<float>(),
                       h->Om.as<double>(), h->P[0].as<double>(), h->c_path.as<double>(), h->c_ops.as<double>(), h->c_status.as<uint8_t>());
    GLOC_HIP(hipGetLastError());
    hipLaunchKernelGGL(pc_pair_kernel, dim3(words, words), dim3(THREADS), 0, s, Lu, words, h->c_ops.as<double>(), h->c_status.as<uint8_t>(), prm->chi2,
                       prm->drift_rot * prm->drift_rot, prm->drift_trans * prm->drift_trans, bits, out_s2 ? h->c_s2.as<double>() : nullptr);
    GLOC_HIP(hipGetLastError());
  }
  {
    ProfScope ps(h->prof, "pgo_consistency", s, ProfScope::Apart, "pgo_consistency_score");
    GLOC_TRY(pairgraph::score_matrix(s, h->c_count.as<uint32_t>(), Lu, words, bits, h->c_score.as<unsigned long long>(), h->c_degree.as<uint32_t>()));
    hipLaunchKernelGGL(pc_key_kernel, dim3(gl), dim3(THREADS), 0, s, Lu, h->c_score.as<unsigned long long>(), h->c_degree.as<uint32_t>(),
                       h->c_key.as<unsigned long long>());
    GLOC_HIP(hipGetLastError());
    GLOC_TRY(pairgraph::rank_seeds(s, h->c_count.as<uint32_t>(), Lu, h->c_key.as<unsigned long long>(), S, h->c_seeds.as<uint32_t>()));
  }
  {
    ProfScope ps(h->prof, "pgo_consistency", s, ProfScope::Apart, "pgo_consistency_clique");
    uint32_t lanes_per_row = 1;
    while (lanes_per_row < std::min(words, 64u)) lanes_per_row <<= 1;
    hipLaunchKernelGGL(pc_clique_kernel, dim3(S), dim3(THREADS), sizeof(unsigned long long) * 3 * words, s, Lu, words, lanes_per_row, bits,
                       h->c_seeds.as<uint32_t>(), h->c_sizes.as<uint32_t>(), h->c_members.as<unsigned long long>(), h->c_counts.as<uint32_t>());
    GLOC_HIP(hipGetLastError());
    hipLaunchKernelGGL(pc_choose_kernel, dim3(1), dim3(THREADS), 0, s, Lu, words, S, prm->min_clique, h->c_sizes.as<uint32_t>(),
                       h->c_members.as<unsigned long long>(), h->c_res.as<uint32_t>(), h->c_mask.as<uint8_t>());
    GLOC_HIP(hipGetLastError());
  }
  uint32_t res[3] = {0, 0, 0};
  GLOC_TRY(fetch(h, h->c_res, res, 3));
  GLOC_TRY(fetch(h, h->c_mask, out_mask, L));
  GLOC_TRY(fetch(h, h->c_status, out_status, L));
  GLOC_TRY(fetch(h, h->c_degree, out_degree, L));
  GLOC_TRY(fetch(h, h->c_score, out_score, L));
  GLOC_TRY(fetch(h, h->c_seeds, out_seeds, S));
  GLOC_TRY(fetch(h, h->c_sizes, out_clique_sizes, S));
  GLOC_TRY(fetch(h, h->c_s2, out_s2, L * L));
  GLOC_HIP(hipStreamSynchronize(s));
  if (out_clique_size) *out_clique_size = res[0];
  if (out_winner_rank) *out_winner_rank = res[1];
  if (out_ok) *out_ok = res[2];
  return GLOC_OK;
}

}  // extern "C"
