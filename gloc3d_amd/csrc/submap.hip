// submap.hip -- local submaps (gloc_scan_store_add_submap[s] of include/gloc3d.h): the host side of submap_kernels.hpp.
// A batch is cut into groups of consecutive submaps of at most `group_points` input points (a submap larger than that
// is a group of its own); a group is ONE launch sequence whatever the number of submaps in it, and every submap's
// result is the same bits whatever group it is in.  Two phases: first every group is voxel-filtered into one device
// buffer of kept centroids -- a submap that keeps no cell fails the call here, before the store has been touched --,
// then the centroids become resident scans through store_make_scans, as gloc_scan_store_add_device makes them.
#include <algorithm>
#include <cmath>
#include <new>

#include "scan_store.hpp"
#include "seg_sort.hpp"
#include "submap_kernels.hpp"
#include "voxel_map.hpp"

namespace gloc {
namespace submap {

struct Ws {
  voxmap::Ws vm;  // keys, values, sort scratch, segments, flags, cell numbers, the scan's block sums, totals, first cells
  DevBuf members, mbegin, q, cent, keep, kpos, kfirst, used, bounds;
  DevBuf out;  // the kept centroids of all groups of the call, submap after submap
};

void free_ws(Ws* w) { delete w; }

namespace {

constexpr size_t DEFAULT_GROUP_POINTS = size_t(8) << 20;
constexpr size_t MAX_GRID_Y = 65535;

struct Plan {  // of one call, on the host
  std::vector<DevScan> scans;  // by member, in the order of the caller's arrays (from first[0] on)
  std::vector<uint64_t> points;  // by submap
};

struct GroupHost {  // what a group copies to and from the device: the caller's, so that it outlives a failed group's copies
  std::vector<Member> mem;
  std::vector<uint32_t> mbegin, first, kfirst, used;
  uint32_t bounds[6];  // the group's cell bounds, as the key kernels found them
  std::vector<voxmap::TgtDesc> seg;
  std::vector<segsort::Seg> segs;
};

// Submaps [a, b) of the call: their kept centroids behind the `out_pts` points w.out already holds.  kept / info: by
// submap of the call.  Synchronises twice (the cell bounds and the counts come back to the host) unless it fails.
int run_group(hipStream_t q, Ws& w, GroupHost& gh, const Plan& pl, const float* member_T, const uint32_t* first, size_t a, size_t b,
              const gloc_submap_params& prm, size_t out_pts, uint32_t* kept, gloc_submap_info* info, size_t* group_kept) {
  const uint32_t S = (uint32_t)(b - a), m0 = first[a], M = first[b] - m0;
  std::vector<Member>& mem = gh.mem;
  std::vector<uint32_t>&mbegin = gh.mbegin, &h_first = gh.first, &h_kfirst = gh.kfirst, &h_used = gh.used;
  std::vector<voxmap::TgtDesc>& seg = gh.seg;
  std::vector<segsort::Seg>& segs = gh.segs;
  mem.resize(M);
  mbegin.resize(M + 1);
  seg.resize(S);
  segs.resize(S);
  h_first.resize(S + 1);
  h_kfirst.resize(S + 1);
  h_used.resize(S);
  uint32_t N = 0, max_mem = 0, max_seg = 0;
  for (uint32_t s = 0; s < S; ++s) {
    const uint32_t begin = N;
    for (uint32_t m = first[a + s]; m < first[a + s + 1]; ++m) {
      const DevScan& sc = pl.scans[m - first[0]];
      Member& d = mem[m - m0];
      d = Member{};
      d.xyz = sc.xyz;
      d.n = (uint32_t)sc.n;
      d.begin = N;
      std::copy(member_T + 16 * (size_t)m, member_T + 16 * (size_t)m + 12, d.T);
      mbegin[m - m0] = N;
      N += d.n;
      max_mem = std::max(max_mem, d.n);
    }
    seg[s] = voxmap::TgtDesc{nullptr, N - begin, begin};
    segs[s] = segsort::Seg{begin, N - begin};
    max_seg = std::max(max_seg, N - begin);
  }
  mbegin[M] = N;
  voxmap::Ws& v = w.vm;
  GLOC_TRY(w.members.ensure(sizeof(Member) * M, q));
  GLOC_TRY(w.mbegin.ensure(4 * (size_t)(M + 1), q));
  GLOC_TRY(v.tgt_desc.ensure(sizeof(voxmap::TgtDesc) * S, q));
  GLOC_TRY(v.segs.ensure(sizeof(segsort::Seg) * S, q));
  GLOC_TRY(v.k0.ensure(8 * (size_t)N, q));
  GLOC_TRY(v.k1.ensure(8 * (size_t)N, q));
  GLOC_TRY(v.v0.ensure(4 * (size_t)N, q));
  GLOC_TRY(v.v1.ensure(4 * (size_t)N, q));
  GLOC_TRY(v.flag.ensure(4 * (size_t)N, q));
  GLOC_TRY(v.pos.ensure(4 * (size_t)N, q));
  GLOC_TRY(w.keep.ensure(4 * (size_t)N, q));
  GLOC_TRY(w.kpos.ensure(4 * (size_t)N, q));
  GLOC_TRY(w.q.ensure(12 * (size_t)N, q));
  GLOC_TRY(w.cent.ensure(12 * (size_t)N, q));
  GLOC_TRY(v.total.ensure(16, q));
  GLOC_TRY(v.first.ensure(4 * (size_t)(S + 1), q));
  GLOC_TRY(w.kfirst.ensure(4 * (size_t)(S + 1), q));
  GLOC_TRY(w.used.ensure(4 * (size_t)S, q));
  const uint32_t key_blocks = voxmap::blocks(max_mem, 256);
  GLOC_REQUIRE((uint64_t)key_blocks * M < (1ull << 31), GLOC_ERR_INVALID,
               "a member of %u points beside %u others: more work-groups than one launch sequence takes", max_mem, M - 1);
  GLOC_TRY(w.bounds.ensure(sizeof(gh.bounds) * ((size_t)key_blocks * M + 1), q));  // [the group's | a work-group's ...]
  GLOC_TRY(v.hist.ensure(segsort::scratch_bytes(S, max_seg), q));
  GLOC_HIP(hipMemcpyAsync(w.members.p, mem.data(), sizeof(Member) * M, hipMemcpyHostToDevice, q));
  GLOC_HIP(hipMemcpyAsync(w.mbegin.p, mbegin.data(), 4 * (size_t)(M + 1), hipMemcpyHostToDevice, q));
  GLOC_HIP(hipMemcpyAsync(v.tgt_desc.p, seg.data(), sizeof(voxmap::TgtDesc) * S, hipMemcpyHostToDevice, q));
  GLOC_HIP(hipMemcpyAsync(v.segs.p, segs.data(), sizeof(segsort::Seg) * S, hipMemcpyHostToDevice, q));

  const float inv = 1.0f / prm.leaf;
  const float mr2 = prm.max_range > 0.f ? prm.max_range * prm.max_range : -1.f;
  unsigned long long* kk[2] = {v.k0.as<unsigned long long>(), v.k1.as<unsigned long long>()};
  uint32_t* vv[2] = {v.v0.as<uint32_t>(), v.v1.as<uint32_t>()};
  uint32_t* total = v.total.as<uint32_t>();
  const voxmap::TgtDesc* d_seg = v.tgt_desc.as<voxmap::TgtDesc>();
  hipLaunchKernelGGL(member_keys_kernel, dim3(key_blocks, M), dim3(256), 0, q, w.members.as<Member>(), inv, mr2, w.q.as<float>(), kk[0],
                     vv[0], w.bounds.as<uint32_t>() + 6);
  hipLaunchKernelGGL(bounds_reduce_kernel, dim3(1), dim3(1024), 0, q, w.bounds.as<uint32_t>() + 6, key_blocks * M, w.bounds.as<uint32_t>());
  // The 3 x 21-bit key costs 8 radix passes; relative to the group's cell bounds a lidar submap needs about 30 bits.  The
  // pass count is the host's to choose, so the bounds come down first (one more synchronise per group).
  GLOC_HIP(hipGetLastError());
  GLOC_HIP(hipMemcpyAsync(gh.bounds, w.bounds.p, sizeof(gh.bounds), hipMemcpyDeviceToHost, q));
  GLOC_HIP(hipStreamSynchronize(q));
  uint32_t bits[3] = {0, 0, 0};
  for (int a = 0; a < 3; ++a) {
    if (gh.bounds[a] > gh.bounds[3 + a]) gh.bounds[a] = gh.bounds[3 + a] = 0u;  // (no point of the group has a key)
    while (bits[a] < 21 && ((gh.bounds[3 + a] - gh.bounds[a]) >> bits[a]) != 0u) ++bits[a];
  }
  hipLaunchKernelGGL(narrow_keys_kernel, dim3(voxmap::blocks(N, 256)), dim3(256), 0, q, kk[0], N, gh.bounds[0], gh.bounds[1], gh.bounds[2],
                     bits[1], bits[2]);
  const int key_bits = (int)(bits[0] + bits[1] + bits[2]) + 1;  // (+ 1: KEY_NONE's bit above every cell)
  const int cur = segsort::sort_pairs<unsigned long long, 8>(q, kk[0], kk[1], vv[0], vv[1], v.segs.as<segsort::Seg>(), S, max_seg, 0,
                                                             key_bits, v.hist.as<uint32_t>());
  const dim3 gseg(voxmap::blocks(max_seg, 256), S);
  hipLaunchKernelGGL(voxmap::cell_flags_kernel, gseg, dim3(256), 0, q, d_seg, kk[cur], v.flag.as<uint32_t>());
  GLOC_TRY(voxmap::scan_flags(q, v, v.flag.as<uint32_t>(), N, v.pos.as<uint32_t>(), total));
  hipLaunchKernelGGL(run_stats_kernel, gseg, dim3(256), 0, q, d_seg, kk[cur], vv[cur], v.flag.as<uint32_t>(), v.pos.as<uint32_t>(),
                     w.q.as<float>(), w.mbegin.as<uint32_t>(), M, std::max(prm.min_points, 1u), std::max(prm.min_scans, 1u),
                     w.cent.as<float>(), w.keep.as<uint32_t>(), w.used.as<uint32_t>());
  GLOC_TRY(voxmap::scan_flags(q, v, w.keep.as<uint32_t>(), N, w.kpos.as<uint32_t>(), total + 1));
  hipLaunchKernelGGL(voxmap::cell_first_kernel, dim3(1), dim3(256), 0, q, d_seg, S, v.pos.as<uint32_t>(), total, v.first.as<uint32_t>());
  hipLaunchKernelGGL(voxmap::cell_first_kernel, dim3(1), dim3(256), 0, q, d_seg, S, w.kpos.as<uint32_t>(), total + 1,
                     w.kfirst.as<uint32_t>());
  GLOC_HIP(hipGetLastError());
  GLOC_HIP(hipMemcpyAsync(h_first.data(), v.first.p, 4 * (size_t)(S + 1), hipMemcpyDeviceToHost, q));
  GLOC_HIP(hipMemcpyAsync(h_kfirst.data(), w.kfirst.p, 4 * (size_t)(S + 1), hipMemcpyDeviceToHost, q));
  GLOC_HIP(hipMemcpyAsync(h_used.data(), w.used.p, 4 * (size_t)S, hipMemcpyDeviceToHost, q));
  GLOC_HIP(hipStreamSynchronize(q));
  for (uint32_t s = 0; s < S; ++s) {
    kept[a + s] = h_kfirst[s + 1] - h_kfirst[s];
    if (info) info[a + s] = gloc_submap_info{pl.points[a + s], h_used[s], h_first[s + 1] - h_first[s], kept[a + s]};
    GLOC_REQUIRE(kept[a + s] != 0, GLOC_ERR_INVALID, "submap %zu keeps no cell (%u of %llu points used, %u cells)", a + s, h_used[s],
                 (unsigned long long)pl.points[a + s], h_first[s + 1] - h_first[s]);
  }
  const size_t K = h_kfirst[S];
  GLOC_TRY(w.out.ensure(12 * (out_pts + K), q, true, 12 * out_pts));
  hipLaunchKernelGGL(compact_kernel, dim3(voxmap::blocks(N, 256)), dim3(256), 0, q, w.keep.as<uint32_t>(), v.pos.as<uint32_t>(),
                     w.kpos.as<uint32_t>(), w.cent.as<float>(), N, w.out.as<float>() + 3 * out_pts);
  GLOC_HIP(hipGetLastError());
  *group_kept = K;
  return GLOC_OK;
}

int add_submaps(gloc_scan_store* st, const uint32_t* member_ids, const float* member_T, const uint32_t* first, size_t count,
                const gloc_submap_params* prm, uint32_t* new_ids, gloc_submap_info* info) {
  GLOC_REQUIRE(st && member_ids && member_T && first && prm && new_ids, GLOC_ERR_INVALID, "null argument");
  GLOC_REQUIRE(count >= 1, GLOC_ERR_INVALID, "no submap asked for");
  GLOC_REQUIRE(prm->leaf > 0.f && std::isfinite(prm->leaf), GLOC_ERR_INVALID, "leaf = %g must be positive and finite", (double)prm->leaf);
  for (size_t s = 0; s < count; ++s) {
    GLOC_REQUIRE(first[s] < first[s + 1], GLOC_ERR_INVALID, "submap %zu has no member (first[] must ascend)", s);
    GLOC_REQUIRE(first[s + 1] - first[s] <= MAX_GRID_Y, GLOC_ERR_INVALID, "submap %zu has %u members, more than %zu", s,
                 first[s + 1] - first[s], MAX_GRID_Y);
  }
  for (size_t e = 16 * (size_t)first[0]; e < 16 * (size_t)first[count]; ++e)
    GLOC_REQUIRE(std::isfinite(member_T[e]), GLOC_ERR_INVALID, "pose of member %zu has a non-finite entry", e / 16);
  GLOC_HIP(hipSetDevice(st->device));
  std::lock_guard<std::mutex> lk(st->mu);
  Plan pl;
  pl.scans.resize(first[count] - first[0]);
  pl.points.assign(count, 0);
  for (size_t s = 0; s < count; ++s) {
    for (uint32_t m = first[s]; m < first[s + 1]; ++m) {
      const uint32_t id = member_ids[m];
      GLOC_REQUIRE(id < st->scans.size() && st->scans[id].live, GLOC_ERR_INVALID, "unknown scan id %u", id);
      pl.scans[m - first[0]] = st->scans[id];  // (by value: read only, and the lock is held to the end)
      pl.points[s] += st->scans[id].n;
    }
    GLOC_REQUIRE(pl.points[s] < (1ull << 31), GLOC_ERR_INVALID, "the members of submap %zu hold %llu points, 2^31 or more", s,
                 (unsigned long long)pl.points[s]);
    GLOC_REQUIRE(pl.points[s] != 0, GLOC_ERR_INVALID, "the members of submap %zu hold no point", s);
  }
  GLOC_TRY(ensure_ws(&st->submap_ws));
  Ws& w = *st->submap_ws;
  hipStream_t q = st->stream;
  const size_t budget = std::min<size_t>(prm->group_points ? prm->group_points : DEFAULT_GROUP_POINTS, (size_t(1) << 31) - 1);
  std::vector<uint32_t> kept(count);
  std::vector<size_t> out_off(count);
  size_t out_pts = 0;
  for (size_t a = 0; a < count;) {
    size_t b = a, pts = 0;
    while (b < count && (b == a || (pts + pl.points[b] <= budget && first[b + 1] - first[a] <= MAX_GRID_Y && b - a < MAX_GRID_Y)))
      pts += pl.points[b++];
    size_t K = 0;
    GroupHost gh;
    const int rc = run_group(q, w, gh, pl, member_T, first, a, b, *prm, out_pts, kept.data(), info, &K);
    if (rc != GLOC_OK) {
      (void)hipStreamSynchronize(q);  // (nothing has been added to the store)
      return rc;
    }
    for (size_t s = a; s < b; ++s) {
      out_off[s] = out_pts;
      out_pts += kept[s];
    }
    a = b;
  }
  // the kept centroids become resident scans, some at a time (the indexing scratch grows with scans x points)
  constexpr size_t CHUNK_SCANS = 256, CHUNK_POINTS = size_t(8) << 20;
  size_t done = 0;
  int rc = GLOC_OK;
  while (done < count && rc == GLOC_OK) {
    size_t e = done, pts = 0;
    while (e < count && e - done < CHUNK_SCANS && (e == done || pts + kept[e] <= CHUNK_POINTS)) pts += kept[e++];
    std::vector<const float*> ptrs(e - done);
    std::vector<size_t> ns(e - done);
    for (size_t s = done; s < e; ++s) {
      ptrs[s - done] = w.out.as<float>() + 3 * out_off[s];
      ns[s - done] = kept[s];
    }
    std::vector<DevScan> made(e - done);
    rc = reg::store_make_scans(st, e - done, ptrs.data(), ns.data(), 3, true, made.data());
    if (rc != GLOC_OK) break;
    for (size_t s = done; s < e; ++s) reg::store_insert_scan(st, made[s - done], &new_ids[s]);
    done = e;
  }
  if (rc != GLOC_OK)  // the store as it was: what this call added goes again
    for (size_t s = 0; s < done; ++s) reg::store_remove_scan(st, new_ids[s]);
  return rc;
}

}  // namespace
}  // namespace submap
}  // namespace gloc

extern "C" {

void gloc_submap_default_params(gloc_submap_params* p) {
  if (!p) return;
  p->leaf = 0.2f;
  p->min_points = 1;
  p->min_scans = 1;
  p->max_range = 0.f;
  p->group_points = 0;
}

int gloc_scan_store_add_submaps(gloc_scan_store* st, const uint32_t* member_ids, const float* member_T, const uint32_t* first,
                                size_t count, const gloc_submap_params* prm, uint32_t* new_ids, gloc_submap_info* info) {
  return gloc::submap::add_submaps(st, member_ids, member_T, first, count, prm, new_ids, info);
}

int gloc_scan_store_add_submap(gloc_scan_store* st, const uint32_t* member_ids, const float* member_T, size_t n,
                               const gloc_submap_params* prm, uint32_t* new_id, gloc_submap_info* info) {
  GLOC_REQUIRE(n < (1ull << 32), GLOC_ERR_INVALID, "too many members");
  const uint32_t first[2] = {0u, (uint32_t)n};
  return gloc::submap::add_submaps(st, member_ids, member_T, first, 1, prm, new_id, info);
}

}  // extern "C"
