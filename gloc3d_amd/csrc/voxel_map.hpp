// voxel_map.hpp -- the host side of voxel_map_kernels.hpp, shared by ndt.hip and vgicp.hip: the workspace of a map, the
// flag scan, the builder of the maps of a call's targets and the export of one map's cells.  What a cell holds is the
// includer's: build() is a template over the cell type and a callable that enqueues the statistics kernel.
#pragma once
#include <algorithm>
#include <vector>

#include "common.hpp"
#include "scan_store.hpp"
#include "seg_sort.hpp"
#include "voxel_map_kernels.hpp"

namespace gloc {
namespace voxmap {

inline uint32_t blocks(size_t n, uint32_t t) { return (uint32_t)((n + t - 1) / t); }

// One per method and handle (ndt::Ws and vgicp::Ws each embed their own: calls of the two on one handle share nothing).
struct Ws {
  DevBuf k0, k1, v0, v1, hist, segs, flag, pos, bsum, total;  // the sort and the flag scan (NDT's source filter uses them too)
  DevBuf tgt_desc, first, cells, hkey, hval, toff, tmask;     // cells of the call's targets and their hash tables
};

struct Maps {                    // of the targets of a call, on the host
  std::vector<uint32_t> first;   // [n_tgt + 1] cell ranges
  std::vector<uint32_t> toff, tmask;
};

// exclusive prefix of n 0/1 flags into pos; *total (device) = their sum
inline int scan_flags(hipStream_t q, Ws& w, const uint32_t* flag, uint32_t n, uint32_t* pos, uint32_t* total) {
  const uint32_t nb = std::max<uint32_t>(1, blocks(n, SCAN_BLOCK));
  GLOC_TRY(w.bsum.ensure(sizeof(uint32_t) * nb, q));
  hipLaunchKernelGGL(scan_sum_kernel, dim3(nb), dim3(SCAN_BLOCK), 0, q, flag, n, w.bsum.as<uint32_t>());
  hipLaunchKernelGGL(scan_top_kernel, dim3(1), dim3(SCAN_BLOCK), 0, q, w.bsum.as<uint32_t>(), nb, total);
  hipLaunchKernelGGL(scan_apply_kernel, dim3(nb), dim3(SCAN_BLOCK), 0, q, flag, n, w.bsum.as<uint32_t>(), pos);
  GLOC_HIP(hipGetLastError());
  return GLOC_OK;
}

// Cells (CellT, into w.cells) of every target and their hash tables.  stats(grid, targets on the device, sorted keys,
// sorted values, flag, pos) enqueues the kernel that writes w.cells.as<CellT>()[pos[i]] for every i with flag[i] set.
// Synchronises twice: to size the tables, and before it returns (*out and whatever the caller uploaded from host vectors
// of its own for `stats` may go when it does).
template <class CellT, class Stats>
int build(hipStream_t q, Ws& w, const std::vector<DevScan>& tg, float resolution, Stats&& stats, Maps* out) {
  const uint32_t T = (uint32_t)tg.size();
  std::vector<TgtDesc> desc(T);
  uint64_t total = 0;
  uint32_t N = 0, max_n = 0;
  for (uint32_t t = 0; t < T; ++t) total += tg[t].n;
  GLOC_REQUIRE(total < (1ull << 31), GLOC_ERR_INVALID, "the targets of one call hold %llu points, more than 2^31", (unsigned long long)total);
  for (uint32_t t = 0; t < T; ++t) {
    desc[t] = TgtDesc{tg[t].xyz, (uint32_t)tg[t].n, N};
    N += (uint32_t)tg[t].n;
    max_n = std::max(max_n, (uint32_t)tg[t].n);
  }
  const size_t NN = std::max<uint32_t>(N, 1);
  GLOC_TRY(w.tgt_desc.ensure(sizeof(TgtDesc) * T, q));
  GLOC_TRY(w.segs.ensure(sizeof(segsort::Seg) * T, q));
  GLOC_TRY(w.k0.ensure(8 * NN, q));
  GLOC_TRY(w.k1.ensure(8 * NN, q));
  GLOC_TRY(w.v0.ensure(4 * NN, q));
  GLOC_TRY(w.v1.ensure(4 * NN, q));
  GLOC_TRY(w.flag.ensure(4 * NN, q));
  GLOC_TRY(w.pos.ensure(4 * NN, q));
  GLOC_TRY(w.total.ensure(16, q));
  GLOC_TRY(w.first.ensure(4 * (T + 1), q));
  GLOC_TRY(w.cells.ensure(sizeof(CellT) * NN, q));
  GLOC_TRY(w.hist.ensure(segsort::scratch_bytes(T, std::max<uint32_t>(max_n, 1)), q));
  std::vector<segsort::Seg> segs(T);
  for (uint32_t t = 0; t < T; ++t) segs[t] = segsort::Seg{desc[t].begin, desc[t].n};
  GLOC_HIP(hipMemcpyAsync(w.tgt_desc.p, desc.data(), sizeof(TgtDesc) * T, hipMemcpyHostToDevice, q));
  GLOC_HIP(hipMemcpyAsync(w.segs.p, segs.data(), sizeof(segsort::Seg) * T, hipMemcpyHostToDevice, q));
  const float inv = 1.0f / resolution;
  const dim3 g(std::max<uint32_t>(1, blocks(max_n, 256)), T);
  auto* K = reinterpret_cast<unsigned long long*>(w.k0.p);
  auto* K1 = reinterpret_cast<unsigned long long*>(w.k1.p);
  hipLaunchKernelGGL(cell_keys_kernel, g, dim3(256), 0, q, w.tgt_desc.as<TgtDesc>(), inv, K, w.v0.as<uint32_t>());
  unsigned long long* kk[2] = {K, K1};
  uint32_t* vv[2] = {w.v0.as<uint32_t>(), w.v1.as<uint32_t>()};
  const int cur = max_n ? segsort::sort_pairs<unsigned long long, 8>(q, kk[0], kk[1], vv[0], vv[1], w.segs.as<segsort::Seg>(), T,
                                                                       max_n, 0, 64, w.hist.as<uint32_t>())
                        : 0;
  hipLaunchKernelGGL(cell_flags_kernel, g, dim3(256), 0, q, w.tgt_desc.as<TgtDesc>(), kk[cur], w.flag.as<uint32_t>());
  GLOC_TRY(scan_flags(q, w, w.flag.as<uint32_t>(), N, w.pos.as<uint32_t>(), w.total.as<uint32_t>()));
  hipLaunchKernelGGL(cell_first_kernel, dim3(1), dim3(256), 0, q, w.tgt_desc.as<TgtDesc>(), T, w.pos.as<uint32_t>(),
                     w.total.as<uint32_t>(), w.first.as<uint32_t>());
  stats(g, w.tgt_desc.as<TgtDesc>(), kk[cur], vv[cur], w.flag.as<uint32_t>(), w.pos.as<uint32_t>());
  GLOC_HIP(hipGetLastError());
  out->first.assign(T + 1, 0);
  GLOC_HIP(hipMemcpyAsync(out->first.data(), w.first.p, 4 * (T + 1), hipMemcpyDeviceToHost, q));
  GLOC_HIP(hipStreamSynchronize(q));
  for (uint32_t t = T; t-- > 0;)  // an empty target has no cells: its range starts where the next one does
    if (desc[t].n == 0) out->first[t] = out->first[t + 1];
  out->toff.assign(T, 0);
  out->tmask.assign(T, 0);
  size_t slots = 0, max_cells = 0;
  for (uint32_t t = 0; t < T; ++t) {
    const size_t nc = out->first[t + 1] - out->first[t];
    max_cells = std::max(max_cells, nc);
    size_t s = 16;
    while (s < 2 * nc) s <<= 1;  // at most half full: a probe always ends at an empty slot
    out->toff[t] = (uint32_t)slots;
    out->tmask[t] = (uint32_t)(s - 1);
    slots += s;
  }
  GLOC_TRY(w.hkey.ensure(8 * slots, q));
  GLOC_TRY(w.hval.ensure(4 * slots, q));
  GLOC_TRY(w.toff.ensure(4 * T, q));
  GLOC_TRY(w.tmask.ensure(4 * T, q));
  GLOC_HIP(hipMemsetAsync(w.hkey.p, 0xFF, 8 * slots, q));
  GLOC_HIP(hipMemcpyAsync(w.toff.p, out->toff.data(), 4 * T, hipMemcpyHostToDevice, q));
  GLOC_HIP(hipMemcpyAsync(w.tmask.p, out->tmask.data(), 4 * T, hipMemcpyHostToDevice, q));
  GLOC_HIP(hipMemcpyAsync(w.first.p, out->first.data(), 4 * (T + 1), hipMemcpyHostToDevice, q));
  if (max_cells)
    hipLaunchKernelGGL(cell_hash_kernel<CellT>, dim3(blocks(max_cells, 256), T), dim3(256), 0, q, w.first.as<uint32_t>(),
                       w.cells.as<CellT>(), w.toff.as<uint32_t>(), w.tmask.as<uint32_t>(),
                       reinterpret_cast<unsigned long long*>(w.hkey.p), w.hval.as<uint32_t>());
  GLOC_HIP(hipGetLastError());
  GLOC_HIP(hipStreamSynchronize(q));  // (out's vectors are the caller's)
  return GLOC_OK;
}

// the three signed voxel indices of a packed key (pack_key's inverse)
inline void unpack_key(unsigned long long key, int32_t out[3]) {
  for (int a = 0; a < 3; ++a) out[a] = (int32_t)((long long)((key >> (42 - 21 * a)) & 0x1FFFFF) - KEY_BIAS);
}

// The valid cells of target 0 of the last build(), in key order: key, count and mean of the first `capacity` of them into
// those of the three arrays that are not null, rest(cell, row) for the columns that are the includer's; *n_valid = how
// many there are, whatever the capacity.  Synchronises.
template <class CellT, class Rest>
int export_valid(hipStream_t q, const Ws& w, const Maps& m, size_t capacity, int32_t* out_key3, uint32_t* out_count, double* out_mean3,
                 Rest&& rest, size_t* n_valid) {
  const uint32_t nc = m.first[1] - m.first[0];
  std::vector<CellT> all(nc);
  if (nc) GLOC_HIP(hipMemcpyAsync(all.data(), w.cells.as<CellT>() + m.first[0], sizeof(CellT) * nc, hipMemcpyDeviceToHost, q));
  GLOC_HIP(hipStreamSynchronize(q));
  size_t v = 0;
  for (const CellT& c : all) {
    if (!c.valid) continue;
    if (v < capacity) {
      if (out_key3) unpack_key(c.key, out_key3 + 3 * v);
      if (out_count) out_count[v] = c.count;
      if (out_mean3) std::copy(c.mean, c.mean + 3, out_mean3 + 3 * v);
      rest(c, v);
    }
    ++v;
  }
  *n_valid = v;
  return GLOC_OK;
}

}  // namespace voxmap
}  // namespace gloc
