// vmap.hip -- resident voxel maps (include/gloc3d.h: M1 - M8): the voxel statistics of the voxelized generalized ICP as a
// target that lives across calls, grows by the scans inserted under poses and forgets by distance and age.  Host side of
// vmap_kernels.hpp; tests/vmap_ref.py is the contract.  The C entry points are in reg.hip, which owns the handle.
//
// A map is allocated whole when it is made -- voxels, their running sums and stamps, one hash table of >= 2 x capacity
// slots -- and nothing of it moves afterwards: the views the refinement takes (vgicp::Target) stay good for the call.
// An insert is the shared voxel-map builder over the moved scan (its contribution, one cell per voxel), a count of the
// keys the map lacks, ONE look of the host at that count -- what sizes the insert and what refuses it -- and the merge.
#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include "vgicp_kernels.hpp"
#include "vmap.hpp"
#include "vmap_kernels.hpp"
#include "voxel_map.hpp"

using namespace gloc;
using namespace gloc::vmap;

namespace gloc {
namespace vmap {

struct Map {
  float resolution = 0.f;
  uint32_t capacity = 0, normal_k = 0, mask = 0;
  uint32_t n_voxels = 0, n_inserts = 0;
  uint64_t n_points = 0;
  DevBuf vox, sums, stamps, hkey, hval;  // [capacity] x 3, [mask + 1] x 2
};

struct Set {
  std::vector<std::unique_ptr<Map>> maps;  // by id; null: destroyed (ids are not reused: a stale id stays unknown)
  voxmap::Ws build;                        // the contribution of an insert (voxmap::build), and the flag scans
  DevBuf aux, moved, is_new, at, rank, total, ctr;
  DevBuf tvox, tsums, tstamps, first, toff, tmask;  // a prune's compaction and the table rebuild's three words
};

void set_free(Set* s) { delete s; }

namespace {

Map* find(const Ctx& x, uint32_t id) {
  Set* s = *x.set;
  return s && id < s->maps.size() ? s->maps[id].get() : nullptr;
}

int get(const Ctx& x, uint32_t id, Map** out) {
  *out = find(x, id);
  GLOC_REQUIRE(*out, GLOC_ERR_INVALID, "unknown voxel map id %u", id);
  return GLOC_OK;
}

// the counters of an insert or a prune and the flag scan's total, read after the launches that wrote them: the ONE wait
int read_back(hipStream_t q, Set& s, Counters* c, uint32_t* total) {
  GLOC_HIP(hipMemcpyAsync(c, s.ctr.p, sizeof(Counters), hipMemcpyDeviceToHost, q));
  if (total) GLOC_HIP(hipMemcpyAsync(total, s.total.p, sizeof(uint32_t), hipMemcpyDeviceToHost, q));
  GLOC_HIP(hipStreamSynchronize(q));
  return GLOC_OK;
}

// M2 - M4 for one scan.  The scan is pinned by the caller and has its normals.
int insert_one(const Ctx& x, Set& s, Map& m, const DevScan& scan, const float* T16) {
  const hipStream_t q = x.stream;
  Pose P{};
  if (T16) {
    for (int i = 0; i < 3; ++i) {
      for (int k = 0; k < 3; ++k) P.T[3 * i + k] = T16[4 * i + k];
      P.T[9 + i] = T16[4 * i + 3];
    }
    P.on = 1u;
  }
  if (scan.n == 0) {  // (an insert all the same: the counter the stamps are taken from moves on)
    m.n_inserts++;
    return GLOC_OK;
  }
  GLOC_REQUIRE(scan.n < (1ull << 31), GLOC_ERR_INVALID, "the scan is too large");
  const uint32_t n = (uint32_t)scan.n;
  std::vector<DevScan> tg(1, scan);
  voxmap::Maps tm;
  {
    ProfScope ps(*x.prof, "vmap_contrib", q);
    if (P.on) {
      GLOC_TRY(s.moved.ensure(12 * (size_t)n, q));
      hipLaunchKernelGGL(move_kernel, dim3(voxmap::blocks(n, 256)), dim3(256), 0, q, scan.xyz, n, P, s.moved.as<float>());
      tg[0].xyz = s.moved.as<float>();
    }
    const TgtAux aux{scan.idx.inv, scan.nrm};
    GLOC_TRY(s.aux.ensure(sizeof(TgtAux), q));
    GLOC_HIP(hipMemcpyAsync(s.aux.p, &aux, sizeof(TgtAux), hipMemcpyHostToDevice, q));  // (build() synchronises)
    GLOC_TRY(voxmap::build<Contrib>(q, s.build, tg, m.resolution, [&](dim3 g, const voxmap::TgtDesc* d, const unsigned long long* key,
                                                                       const uint32_t* val, const uint32_t* flag, const uint32_t* pos) {
      hipLaunchKernelGGL(contrib_stats_kernel, g, dim3(256), 0, q, d, s.aux.as<TgtAux>(), key, val, flag, pos, (double)m.resolution, P,
                         s.build.cells.as<Contrib>());
    }, &tm));
  }
  const uint32_t nc = tm.first[1] - tm.first[0];
  if (nc == 0) {  // (no point of the scan is in a voxel)
    m.n_inserts++;
    return GLOC_OK;
  }
  const Contrib* con = s.build.cells.as<Contrib>() + tm.first[0];
  const dim3 g(voxmap::blocks(nc, 256));
  GLOC_TRY(s.is_new.ensure(4 * (size_t)nc, q));
  GLOC_TRY(s.at.ensure(4 * (size_t)nc, q));
  GLOC_TRY(s.rank.ensure(4 * (size_t)nc, q));
  GLOC_TRY(s.total.ensure(16, q));
  GLOC_TRY(s.ctr.ensure(sizeof(Counters), q));
  Counters ctr{};
  uint32_t n_new = 0;
  {
    ProfScope ps(*x.prof, "vmap_count", q);
    GLOC_HIP(hipMemsetAsync(s.ctr.p, 0, sizeof(Counters), q));
    hipLaunchKernelGGL(count_new_kernel, g, dim3(256), 0, q, con, nc, reinterpret_cast<const unsigned long long*>(m.hkey.p),
                       m.hval.as<uint32_t>(), m.mask, s.is_new.as<uint32_t>(), s.at.as<uint32_t>(), s.ctr.as<Counters>());
    GLOC_TRY(voxmap::scan_flags(q, s.build, s.is_new.as<uint32_t>(), nc, s.rank.as<uint32_t>(), s.total.as<uint32_t>()));
  }
  GLOC_TRY(read_back(q, s, &ctr, &n_new));  // the wait that sizes the insert
  GLOC_REQUIRE(!ctr.err, GLOC_ERR_STATE, "the voxel map's table is broken: a probe found no empty slot");
  GLOC_REQUIRE((uint64_t)m.n_voxels + n_new <= m.capacity, GLOC_ERR_NOMEM, "the scan adds %u voxels to %u, the map holds %u", n_new,
               m.n_voxels, m.capacity);
  {
    ProfScope ps(*x.prof, "vmap_merge", q);
    hipLaunchKernelGGL(merge_kernel, g, dim3(256), 0, q, con, nc, s.is_new.as<uint32_t>(), s.rank.as<uint32_t>(), s.at.as<uint32_t>(),
                       m.n_voxels, m.capacity, m.n_inserts + 1, (double)m.resolution, reinterpret_cast<unsigned long long*>(m.hkey.p),
                       m.hval.as<uint32_t>(), m.mask, m.vox.as<Voxel>(), m.sums.as<Sums>(), m.stamps.as<uint32_t>(), s.ctr.as<Counters>());
    GLOC_HIP(hipGetLastError());
  }
  m.n_voxels += n_new;
  m.n_inserts++;
  m.n_points += ctr.points;
  GLOC_TRY(read_back(q, s, &ctr, nullptr));  // (the contribution is the Set's: the next insert builds over it)
  GLOC_REQUIRE(!ctr.err, GLOC_ERR_STATE, "the voxel map's table is broken: a new key found no empty slot");
  return GLOC_OK;
}

}  // namespace

int check_params(const gloc_vmap_params* p) {
  GLOC_REQUIRE(p, GLOC_ERR_INVALID, "params is null");
  GLOC_REQUIRE(p->resolution > 0.f && p->resolution <= 3.0e38f, GLOC_ERR_INVALID, "resolution = %g must be > 0 and finite", (double)p->resolution);
  GLOC_REQUIRE(p->capacity >= 1 && p->capacity <= (1u << 24), GLOC_ERR_INVALID, "capacity = %u outside [1, 2^24]", p->capacity);
  GLOC_REQUIRE(p->normal_k >= 3 && p->normal_k <= 16, GLOC_ERR_INVALID, "normal_k = %u outside [3, 16]", p->normal_k);
  return GLOC_OK;
}

int create(const Ctx& x, const gloc_vmap_params* prm, uint32_t* out_map_id) {
  GLOC_TRY(ensure_ws(x.set));
  Set& s = **x.set;
  const hipStream_t q = x.stream;
  std::unique_ptr<Map> m(new (std::nothrow) Map);
  GLOC_REQUIRE(m, GLOC_ERR_NOMEM, "host allocation failed");
  m->resolution = prm->resolution;
  m->capacity = prm->capacity;
  m->normal_k = prm->normal_k;
  size_t slots = 16;
  while (slots < 2 * (size_t)prm->capacity) slots <<= 1;  // at most half full: a probe always ends at an empty slot
  m->mask = (uint32_t)(slots - 1);
  GLOC_TRY(m->vox.ensure(sizeof(Voxel) * (size_t)prm->capacity, q));
  GLOC_TRY(m->sums.ensure(sizeof(Sums) * (size_t)prm->capacity, q));
  GLOC_TRY(m->stamps.ensure(4 * (size_t)prm->capacity, q));
  GLOC_TRY(m->hkey.ensure(8 * slots, q));
  GLOC_TRY(m->hval.ensure(4 * slots, q));
  GLOC_HIP(hipMemsetAsync(m->hkey.p, 0xFF, 8 * slots, q));
  GLOC_HIP(hipStreamSynchronize(q));
  *out_map_id = (uint32_t)s.maps.size();
  s.maps.push_back(std::move(m));
  return GLOC_OK;
}

int check_id(const Ctx& x, uint32_t map_id) {
  Map* m;
  return get(x, map_id, &m);
}

int destroy(const Ctx& x, uint32_t map_id) {
  Map* m;
  GLOC_TRY(get(x, map_id, &m));
  GLOC_HIP(hipStreamSynchronize(x.stream));
  (*x.set)->maps[map_id].reset();
  return GLOC_OK;
}

int insert(const Ctx& x, uint32_t map_id, const uint32_t* scan_ids, size_t n, const float* T) {
  Map* m;
  GLOC_TRY(get(x, map_id, &m));
  GLOC_REQUIRE(x.store, GLOC_ERR_INVALID, "unknown scan id %u", scan_ids[0]);
  DevScan probe;
  for (size_t i = 0; i < n; ++i) GLOC_TRY(reg::store_get(x.store, scan_ids[i], 0, &probe));
  Set& s = **x.set;
  for (size_t i = 0; i < n; ++i) {
    GLOC_TRY(reg::store_ensure_normals(x.store, scan_ids + i, 1, m->normal_k));
    reg::ScopedPins pins(x.store, x.stream);
    GLOC_TRY(pins.pin(scan_ids + i, nullptr, 1));
    GLOC_REQUIRE(pins.scans[0].n == 0 || pins.scans[0].nrm, GLOC_ERR_STATE, "scan %u lost its normals during the call", scan_ids[i]);
    GLOC_TRY(insert_one(x, s, *m, pins.scans[0], T ? T + 16 * i : nullptr));
  }
  return GLOC_OK;
}

int prune(const Ctx& x, uint32_t map_id, const float* center3, float max_dist, uint32_t max_age, uint32_t* out_removed) {
  Map* mp;
  GLOC_TRY(get(x, map_id, &mp));
  Map& m = *mp;
  Set& s = **x.set;
  const hipStream_t q = x.stream;
  if (out_removed) *out_removed = 0;
  const uint32_t nv = m.n_voxels;
  if (nv == 0 || (!center3 && max_age == 0)) return GLOC_OK;
  const dim3 g(voxmap::blocks(nv, 256));
  GLOC_TRY(s.is_new.ensure(4 * (size_t)nv, q));
  GLOC_TRY(s.rank.ensure(4 * (size_t)nv, q));
  GLOC_TRY(s.total.ensure(16, q));
  GLOC_TRY(s.ctr.ensure(sizeof(Counters), q));
  GLOC_TRY(s.tvox.ensure(sizeof(Voxel) * (size_t)nv, q));
  GLOC_TRY(s.tsums.ensure(sizeof(Sums) * (size_t)nv, q));
  GLOC_TRY(s.tstamps.ensure(4 * (size_t)nv, q));
  uint32_t* keep = s.is_new.as<uint32_t>();
  Counters ctr{};
  uint32_t kept = 0;
  {
    ProfScope ps(*x.prof, "vmap_prune_flags", q);
    GLOC_HIP(hipMemsetAsync(s.ctr.p, 0, sizeof(Counters), q));
    const double md = (double)max_dist;
    hipLaunchKernelGGL(prune_flags_kernel, g, dim3(256), 0, q, m.vox.as<Voxel>(), m.stamps.as<uint32_t>(), nv, center3 != nullptr,
                       center3 ? (double)center3[0] : 0.0, center3 ? (double)center3[1] : 0.0, center3 ? (double)center3[2] : 0.0, md * md,
                       max_age, m.n_inserts, keep, s.ctr.as<Counters>());
    GLOC_TRY(voxmap::scan_flags(q, s.build, keep, nv, s.rank.as<uint32_t>(), s.total.as<uint32_t>()));
  }
  GLOC_TRY(read_back(q, s, &ctr, &kept));
  if (out_removed) *out_removed = nv - kept;
  if (kept == nv) return GLOC_OK;
  {
    ProfScope ps(*x.prof, "vmap_prune_compact", q);
    hipLaunchKernelGGL(compact_kernel, g, dim3(256), 0, q, m.vox.as<Voxel>(), m.sums.as<Sums>(), m.stamps.as<uint32_t>(), nv, keep,
                       s.rank.as<uint32_t>(), s.tvox.as<Voxel>(), s.tsums.as<Sums>(), s.tstamps.as<uint32_t>());
    if (kept) {
      GLOC_HIP(hipMemcpyAsync(m.vox.p, s.tvox.p, sizeof(Voxel) * (size_t)kept, hipMemcpyDeviceToDevice, q));
      GLOC_HIP(hipMemcpyAsync(m.sums.p, s.tsums.p, sizeof(Sums) * (size_t)kept, hipMemcpyDeviceToDevice, q));
      GLOC_HIP(hipMemcpyAsync(m.stamps.p, s.tstamps.p, 4 * (size_t)kept, hipMemcpyDeviceToDevice, q));
    }
  }
  {
    ProfScope ps(*x.prof, "vmap_prune_table", q);
    // the table again from the survivors: no tombstones, so every probe still ends at an empty slot
    const uint32_t first[2] = {0u, kept}, zero = 0u;
    GLOC_TRY(s.first.ensure(8, q));
    GLOC_TRY(s.toff.ensure(4, q));
    GLOC_TRY(s.tmask.ensure(4, q));
    GLOC_HIP(hipMemsetAsync(m.hkey.p, 0xFF, 8 * ((size_t)m.mask + 1), q));
    GLOC_HIP(hipMemcpyAsync(s.first.p, first, 8, hipMemcpyHostToDevice, q));
    GLOC_HIP(hipMemcpyAsync(s.toff.p, &zero, 4, hipMemcpyHostToDevice, q));
    GLOC_HIP(hipMemcpyAsync(s.tmask.p, &m.mask, 4, hipMemcpyHostToDevice, q));
    if (kept)
      hipLaunchKernelGGL(voxmap::cell_hash_kernel<Voxel>, dim3(voxmap::blocks(kept, 256), 1), dim3(256), 0, q, s.first.as<uint32_t>(),
                         m.vox.as<Voxel>(), s.toff.as<uint32_t>(), s.tmask.as<uint32_t>(), reinterpret_cast<unsigned long long*>(m.hkey.p),
                         m.hval.as<uint32_t>());
    GLOC_HIP(hipGetLastError());
  }
  GLOC_HIP(hipStreamSynchronize(q));  // (first and zero are this frame's)
  m.n_voxels = kept;
  m.n_points -= ctr.points;
  return GLOC_OK;
}

int info(const Ctx& x, uint32_t map_id, gloc_vmap_info* out) {
  Map* m;
  GLOC_TRY(get(x, map_id, &m));
  out->n_voxels = m->n_voxels;
  out->capacity = m->capacity;
  out->n_inserts = m->n_inserts;
  out->resolution = m->resolution;
  out->n_points = m->n_points;
  return GLOC_OK;
}

int voxels(const Ctx& x, uint32_t map_id, size_t capacity, int32_t* out_key3, uint32_t* out_count, double* out_mean3, double* out_nn6,
           uint32_t* out_stamp, size_t* n_voxels) {
  Map* m;
  GLOC_TRY(get(x, map_id, &m));
  const hipStream_t q = x.stream;
  const size_t nv = m->n_voxels;
  *n_voxels = nv;
  const bool any = out_key3 || out_count || out_mean3 || out_nn6 || out_stamp;
  GLOC_REQUIRE(nv <= capacity || !any, GLOC_ERR_INVALID, "buffers hold %zu voxels, the map has %zu", capacity, nv);
  if (!any || nv == 0) return GLOC_OK;
  std::vector<Voxel> all(nv);
  std::vector<uint32_t> stamps(nv), order(nv);
  GLOC_HIP(hipMemcpyAsync(all.data(), m->vox.p, sizeof(Voxel) * nv, hipMemcpyDeviceToHost, q));
  GLOC_HIP(hipMemcpyAsync(stamps.data(), m->stamps.p, 4 * nv, hipMemcpyDeviceToHost, q));
  GLOC_HIP(hipStreamSynchronize(q));
  for (size_t i = 0; i < nv; ++i) order[i] = (uint32_t)i;
  // (the packed key is biased per axis: its order is that of (kx, ky, kz))
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return all[a].key < all[b].key; });
  for (size_t r = 0; r < nv; ++r) {
    const Voxel& c = all[order[r]];
    if (out_key3) voxmap::unpack_key(c.key, out_key3 + 3 * r);
    if (out_count) out_count[r] = c.count;
    if (out_mean3) std::copy(c.mean, c.mean + 3, out_mean3 + 3 * r);
    if (out_nn6) std::copy(c.nn, c.nn + 6, out_nn6 + 6 * r);
    if (out_stamp) out_stamp[r] = stamps[order[r]];
  }
  return GLOC_OK;
}

int refine(const Ctx& x, const vgicp::Ctx& v, const gn6::Call& c, const gloc_vgicp_params* prm) {
  GLOC_REQUIRE(prm->min_points == 1, GLOC_ERR_INVALID, "min_points = %u: a resident map keeps every voxel (min_points 1)", prm->min_points);
  std::vector<vgicp::Target> tg(c.n, vgicp::Target{nullptr, nullptr, nullptr, 0u, 0u});
  for (size_t j = 0; j < c.n; ++j) {
    if (c.tgt_ids[j] == reg::NO_SCAN) continue;
    Map* m;
    GLOC_TRY(get(x, c.tgt_ids[j], &m));
    GLOC_REQUIRE(std::memcmp(&m->resolution, &prm->resolution, sizeof(float)) == 0, GLOC_ERR_INVALID,
                 "resolution = %g is not that of map %u (%g)", (double)prm->resolution, c.tgt_ids[j], (double)m->resolution);
    tg[j] = vgicp::Target{reinterpret_cast<const unsigned long long*>(m->hkey.p), m->hval.as<uint32_t>(), m->vox.as<Voxel>(), m->mask, 0u};
  }
  return vgicp::run(v, c, prm, tg.data());
}

}  // namespace vmap
}  // namespace gloc

extern "C" {

void gloc_vmap_default_params(gloc_vmap_params* p) {
  if (!p) return;
  p->resolution = 1.0f;  // gloc_vgicp_default_params'
  p->capacity = 1u << 18;
  p->normal_k = 10;
  p->reserved_ = 0;
}

}  // extern "C"
