// pillar.hip -- C ABI of the PointPillar scan front end (include/gloc3d.h, "PointPillar-NetVLAD scan descriptor").
// Replaces points_to_voxels + the input packing of the traced scan model (model/voxel.py:23-133,
// s2s_libtorch/gen_libtorch_pointpillar.py:47-62; the C++ demo's per-point loop, i2i_feature_extract.cpp:41-137) and the
// PointNet + scatter-mean at the head of PointPillarTest.forward (model/s2s_merged.py:113-127,204-222), and the 2-D
// backbone behind it (PointPillarTest after the scatter-mean, s2s_merged.py:152-188,219-247; pillar_backbone_kernels.hpp).
#include <algorithm>
#include <cmath>

#include "common.hpp"
#include "pillar_backbone_kernels.hpp"
#include "pillar_kernels.hpp"
#include "seg_sort.hpp"

using namespace gloc;
using namespace gloc::pillar;

namespace {

// The backbone's 13 convolutions (include/gloc3d.h, gloc_pillar_backbone_layer_shape): 3x3, pad 1, no bias, eval
// BatchNorm; `up`: the bilinear upsample (align_corners=True) in front of the layer (up2, up3)
constexpr int BB_LAYERS = 13;
struct BbLayer {
  int cin, cout, stride;
  bool relu;
  int up;
};
constexpr BbLayer BB[BB_LAYERS] = {
    {64, 64, 1, true, 1},   {64, 64, 1, true, 1},   {64, 128, 2, true, 1},  {128, 128, 1, true, 1},  // block1, block2
    {128, 128, 1, true, 1}, {128, 256, 2, true, 1}, {256, 256, 1, true, 1}, {256, 256, 1, true, 1},  // block3
    {64, 64, 1, true, 1},   {128, 128, 1, true, 2}, {256, 256, 1, true, 4},                          // up1, up2, up3
    {448, 256, 1, true, 1}, {256, 128, 1, false, 1}};                                                // conv_out
const char* const BB_FAMILY[BB_LAYERS] = {"pillar_conv0", "pillar_conv1", "pillar_conv2",  "pillar_conv3",
                                          "pillar_conv4", "pillar_conv5", "pillar_conv6",  "pillar_conv7",
                                          "pillar_conv8", "pillar_conv9", "pillar_conv10", "pillar_conv11",
                                          "pillar_conv12"};
constexpr size_t BB_CHUNK = 16;        // scans per pass through the backbone (bounds the activations: ~42 MB a scan)
constexpr uint32_t BB_MAX_SIDE = 4096;

}  // namespace

struct gloc_pillar : Handle {
  DevBuf keys[2], vals[2], flags, hist, segs, offsets, vrange, vcent, vcnt, inputs, part, pn;
  Staging stage;                          // host-pointer API staging
  std::vector<segsort::Seg> h_segs;       // kept alive until the next call (the uploads are asynchronous)
  std::vector<uint64_t> h_offsets;
  bool have_pn = false;
  // backbone: split weights [Cout][9 Cin / 8][h | m], BatchNorm scale and shift [Cout]; activations NHWC
  DevBuf bw[BB_LAYERS], bscale[BB_LAYERS], bshift[BB_LAYERS];
  bool bset[BB_LAYERS] = {};
  DevBuf braw, canvas, big, a64, f1, half[2], quarter[2], cat, lay_in, lay_up;
  bool bb_lds_attr[2] = {};  // dynamic-LDS limit raised for bb_conv_kernel<2, 1>, <2, 2>
};

namespace {

int make_grid(const gloc_pillar_params* p, Grid* g) {
  GLOC_REQUIRE(p, GLOC_ERR_INVALID, "params is NULL");
  const float* b[3] = {p->xbound, p->ybound, p->zbound};
  uint64_t nv = 1;
  for (int k = 0; k < 3; ++k) {
    GLOC_REQUIRE(std::isfinite(b[k][0]) && std::isfinite(b[k][1]) && std::isfinite(b[k][2]) && b[k][2] > 0.f &&
                     b[k][1] > b[k][0],
                 GLOC_ERR_INVALID, "bound %d must be finite [lo, hi, res] with hi > lo and res > 0", k);
    // the grid size from the bounds widened to double and truncated, as voxel.py:40-45 does with numpy
    const double cells = ((double)b[k][1] - (double)b[k][0]) / (double)b[k][2];
    GLOC_REQUIRE(cells >= 1.0 && cells < 16777216.0, GLOC_ERR_INVALID, "bound %d gives %.0f cells", k, cells);
    g->off[k] = b[k][0];
    g->res[k] = b[k][2];
    g->size[k] = (int)cells;
    nv *= (uint64_t)g->size[k];
  }
  // the index goes through float channel 14: exact below 2^24
  GLOC_REQUIRE(nv <= (1u << 24), GLOC_ERR_INVALID, "%llu voxels exceed 2^24", (unsigned long long)nv);
  GLOC_REQUIRE(p->num_points >= 1 && p->num_points <= (1u << 24), GLOC_ERR_INVALID, "num_points must be in [1, 2^24]");
  GLOC_REQUIRE(p->mask_mode == GLOC_PILLAR_MASK_INPUT || p->mask_mode == GLOC_PILLAR_MASK_VALID, GLOC_ERR_INVALID,
               "unknown mask_mode %u", p->mask_mode);
  g->nv = (uint32_t)nv;
  return GLOC_OK;
}

int check_batch(const float* d_pts, const uint64_t* offsets, size_t n_scans, size_t stride, const gloc_pillar_params* p,
                const void* d_out) {
  GLOC_REQUIRE(stride >= 4 && stride <= 64, GLOC_ERR_INVALID, "stride_floats must be in [4, 64]");
  GLOC_REQUIRE(n_scans > 0 && n_scans <= 65535, GLOC_ERR_INVALID, "n_scans must be in [1, 65535]");
  GLOC_REQUIRE(offsets && d_out, GLOC_ERR_INVALID, "NULL argument");
  GLOC_REQUIRE(((uintptr_t)d_out & 15) == 0, GLOC_ERR_INVALID, "output must be 16-byte aligned");
  for (size_t i = 0; i < n_scans; ++i)
    GLOC_REQUIRE(offsets[i + 1] >= offsets[i], GLOC_ERR_INVALID, "offsets must be non-decreasing");
  GLOC_REQUIRE(offsets[n_scans] == 0 || d_pts, GLOC_ERR_INVALID, "points pointer is NULL");
  GLOC_REQUIRE((uint64_t)n_scans * p->num_points <= (1ull << 31), GLOC_ERR_INVALID,
               "n_scans x num_points exceeds 2^31 rows");
  return GLOC_OK;
}

// classify -> sort -> runs -> voxel -> gather into d_out [n_scans][P][16]; leaves the sorted order, flags and voxel
// ranges in the handle for the canvas.  Returns the index of the sorted key / row buffers in *cur.
int front(gloc_pillar* h, const float* d_pts, const uint64_t* offsets, size_t n_scans, size_t stride,
          const gloc_pillar_params* p, const Grid& g, float* d_out, int* cur) {
  GLOC_HIP(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  const uint32_t P = p->num_points, B = (uint32_t)n_scans;
  const size_t rows = (size_t)B * P;
  for (DevBuf* k : {&h->keys[0], &h->keys[1], &h->vals[0], &h->vals[1], &h->flags}) GLOC_TRY(k->ensure(rows * 4, s));
  GLOC_TRY(h->hist.ensure(segsort::scratch_bytes(B, P), s));
  GLOC_TRY(h->segs.ensure(sizeof(segsort::Seg) * B, s));
  GLOC_TRY(h->offsets.ensure(sizeof(uint64_t) * (B + 1), s));
  GLOC_TRY(h->vrange.ensure(sizeof(uint2) * B * g.nv, s));
  GLOC_TRY(h->vcent.ensure(sizeof(float4) * B * g.nv, s));
  GLOC_TRY(h->vcnt.ensure(sizeof(float) * B * g.nv, s));
  h->h_segs.resize(B);
  for (uint32_t b = 0; b < B; ++b) h->h_segs[b] = segsort::Seg{b * P, P};
  h->h_offsets.assign(offsets, offsets + n_scans + 1);
  GLOC_HIP(hipMemcpyAsync(h->offsets.p, h->h_offsets.data(), sizeof(uint64_t) * (B + 1), hipMemcpyHostToDevice, s));
  GLOC_HIP(hipMemcpyAsync(h->segs.p, h->h_segs.data(), sizeof(segsort::Seg) * B, hipMemcpyHostToDevice, s));
  const float* pts = offsets[n_scans] ? d_pts : h->keys[0].as<float>();  // any valid pointer: no point is read
  const dim3 rgrid((P + 255) / 256, B), vgrid((g.nv + 255) / 256, B);
  {
    ProfScope ps(h->prof, "pillar_classify", s);
    hipLaunchKernelGGL(pillar_classify_kernel, rgrid, dim3(256), 0, s, pts, h->offsets.as<uint64_t>(), (int)stride, P, g,
                       h->keys[0].as<uint32_t>(), h->vals[0].as<uint32_t>(), h->flags.as<uint32_t>());
    GLOC_HIP(hipGetLastError());
  }
  {
    ProfScope ps(h->prof, "pillar_sort", s);
    int bits = 0;
    while (bits < 32 && ((g.nv - 1) >> bits)) ++bits;
    const int end_bit = std::max(8, (bits + 7) / 8 * 8);  // 11 200 voxels: two 8-bit passes
    *cur = segsort::sort_pairs<uint32_t, 8>(s, h->keys[0].as<uint32_t>(), h->keys[1].as<uint32_t>(),
                                            h->vals[0].as<uint32_t>(), h->vals[1].as<uint32_t>(),
                                            h->segs.as<segsort::Seg>(), B, P, 0, end_bit, h->hist.as<uint32_t>());
    GLOC_HIP(hipGetLastError());
  }
  {
    ProfScope ps(h->prof, "pillar_runs", s);
    GLOC_HIP(hipMemsetAsync(h->vrange.p, 0, sizeof(uint2) * B * g.nv, s));
    hipLaunchKernelGGL(pillar_runs_kernel, rgrid, dim3(256), 0, s, h->keys[*cur].as<uint32_t>(), P, g.nv,
                       h->vrange.as<uint2>());
    GLOC_HIP(hipGetLastError());
  }
  {
    ProfScope ps(h->prof, "pillar_voxel", s);
    hipLaunchKernelGGL(pillar_voxel_kernel, vgrid, dim3(256), 0, s, pts, h->offsets.as<uint64_t>(), (int)stride, P, g.nv,
                       h->vals[*cur].as<uint32_t>(), h->flags.as<uint32_t>(), h->vrange.as<uint2>(),
                       h->vcent.as<float4>(), h->vcnt.as<float>());
    GLOC_HIP(hipGetLastError());
  }
  {
    ProfScope ps(h->prof, "pillar_gather", s);
    hipLaunchKernelGGL(pillar_gather_kernel, rgrid, dim3(256), 0, s, pts, h->offsets.as<uint64_t>(), (int)stride, P, g,
                       h->vcent.as<float4>(), h->vcnt.as<float>(), reinterpret_cast<float4*>(d_out));
    GLOC_HIP(hipGetLastError());
  }
  return GLOC_OK;
}

int inputs_device(gloc_pillar* h, const float* d_pts, const uint64_t* offsets, size_t n_scans, size_t stride,
                  const gloc_pillar_params* p, float* d_out) {
  Grid g;
  GLOC_TRY(make_grid(p, &g));
  GLOC_TRY(check_batch(d_pts, offsets, n_scans, stride, p, d_out));
  int cur = 0;
  return front(h, d_pts, offsets, n_scans, stride, p, g, d_out, &cur);
}

int canvas_device(gloc_pillar* h, const float* d_pts, const uint64_t* offsets, size_t n_scans, size_t stride,
                  const gloc_pillar_params* p, float* d_out) {
  Grid g;
  GLOC_TRY(make_grid(p, &g));
  GLOC_TRY(check_batch(d_pts, offsets, n_scans, stride, p, d_out));
  GLOC_REQUIRE(h->have_pn, GLOC_ERR_STATE, "no PointNet weights: call gloc_pillar_set_pointnet first");
  const uint32_t P = p->num_points, B = (uint32_t)n_scans;
  hipStream_t s = h->stream;
  GLOC_HIP(hipSetDevice(h->device));
  GLOC_TRY(h->inputs.ensure(sizeof(float) * 16 * B * (size_t)P, s));
  int cur = 0;
  GLOC_TRY(front(h, d_pts, offsets, n_scans, stride, p, g, h->inputs.as<float>(), &cur));
  const uint32_t n_tiles = (P + TILE - 1) / TILE;
  GLOC_TRY(h->part.ensure(sizeof(double) * 2 * FEAT * n_tiles * B, s));
  const bool valid = p->mask_mode == GLOC_PILLAR_MASK_VALID;
  {
    ProfScope ps(h->prof, "pillar_partial", s);
    const dim3 grid((n_tiles + 3) / 4, B);
    auto k = valid ? pillar_partial_kernel<1> : pillar_partial_kernel<0>;
    hipLaunchKernelGGL(k, grid, dim3(256), 0, s, h->inputs.as<float>(), h->keys[cur].as<uint32_t>(),
                       h->vals[cur].as<uint32_t>(), h->flags.as<uint32_t>(), P, n_tiles, h->pn.as<Pn>(),
                       h->part.as<double>());
    GLOC_HIP(hipGetLastError());
  }
  {
    ProfScope ps(h->prof, "pillar_canvas", s);
    const dim3 grid((g.nv + 63) / 64, B);
    auto k = valid ? pillar_canvas_kernel<1> : pillar_canvas_kernel<0>;
    hipLaunchKernelGGL(k, grid, dim3(1024), 0, s, h->inputs.as<float>(), h->vals[cur].as<uint32_t>(),
                       h->flags.as<uint32_t>(), h->vrange.as<uint2>(), P, g.nv, n_tiles, h->pn.as<Pn>(),
                       h->part.as<double>(), d_out);
    GLOC_HIP(hipGetLastError());
  }
  return GLOC_OK;
}

// ---- backbone ------------------------------------------------------------------------------------------------------

int bb_out_side(int in, int stride) { return (in - 1) / stride + 1; }  // 3x3, pad 1

// one convolution: `in` NHWC [n][Hi][Wi][Cin] -> `out` in the layout `epi` selects (pillar_backbone_kernels.hpp)
template <int WN>
int bb_launch(gloc_pillar* h, int layer, const float* in, float* out, size_t n, int Hi, int Wi, int epi, int ldc,
              int c_off) {
  const BbLayer& L = BB[layer];
  constexpr int WM = 2, BN = 64 * WN, TROWS = 4 * WM;
  constexpr int lds = conv_lds_bytes<WM, WN>();
  auto kern = bb_conv_kernel<WM, WN>;
  if (!h->bb_lds_attr[WN - 1]) {  // once per handle (and so per device)
    GLOC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    h->bb_lds_attr[WN - 1] = true;
  }
  const int Ho = bb_out_side(Hi, L.stride), Wo = bb_out_side(Wi, L.stride);
  const int tiles_x = (Wo + 15) / 16, tiles_y = (Ho + TROWS - 1) / TROWS;
  ProfScope ps(h->prof, BB_FAMILY[layer], h->stream);
  hipLaunchKernelGGL(kern, dim3(tiles_x * tiles_y, L.cout / BN, (unsigned)n), dim3(256), lds, h->stream, in,
                     h->bw[layer].as<u32x4>(), h->bscale[layer].as<float>(), h->bshift[layer].as<float>(), out, Hi, Wi,
                     Ho, Wo, L.cin, L.cout, L.stride, tiles_x, epi | (L.relu ? BB_RELU : 0), ldc, c_off);
  GLOC_HIP(hipGetLastError());
  return GLOC_OK;
}

int bb_conv(gloc_pillar* h, int layer, const float* in, float* out, size_t n, int Hi, int Wi, int epi, int ldc = 0,
            int c_off = 0) {
  if (BB[layer].cout == 64) return bb_launch<1>(h, layer, in, out, n, Hi, Wi, epi, ldc ? ldc : 64, c_off);
  return bb_launch<2>(h, layer, in, out, n, Hi, Wi, epi, ldc ? ldc : BB[layer].cout, c_off);
}

int bb_layout(gloc_pillar* h, const float* in, size_t n, int C, int HW, float* out) {
  const size_t count = n * (size_t)C * HW;
  ProfScope ps(h->prof, "pillar_layout", h->stream);
  hipLaunchKernelGGL(bb_nchw_to_nhwc_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, h->stream, in, n, C,
                     HW, out);
  GLOC_HIP(hipGetLastError());
  return GLOC_OK;
}

int bb_upsample(gloc_pillar* h, const float* in, size_t n, int H, int W, int C, int s, float* out) {
  const size_t count = n * (size_t)H * s * W * s * C;
  ProfScope ps(h->prof, "pillar_upsample", h->stream);
  hipLaunchKernelGGL(bb_upsample_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, h->stream, in, n, H, W, C,
                     s, out);
  GLOC_HIP(hipGetLastError());
  return GLOC_OK;
}

int bb_check_layers(gloc_pillar* h) {
  for (int l = 0; l < BB_LAYERS; ++l)
    GLOC_REQUIRE(h->bset[l], GLOC_ERR_STATE, "backbone layer %d was never set (gloc_pillar_set_backbone_layer)", l);
  return GLOC_OK;
}

int bb_check_grid(size_t n, uint32_t gx, uint32_t gy) {
  GLOC_REQUIRE(n >= 1 && n <= 65535, GLOC_ERR_INVALID, "n must be in [1, 65535]");
  // up2 and up3 must give block1's size back: gx and gy multiples of 4 (torch.cat refuses the others)
  GLOC_REQUIRE(gx >= 4 && gy >= 4 && gx <= BB_MAX_SIDE && gy <= BB_MAX_SIDE && gx % 4 == 0 && gy % 4 == 0,
               GLOC_ERR_INVALID, "gx and gy must be multiples of 4 in [4, %u] (got %u x %u)", BB_MAX_SIDE, gx, gy);
  return GLOC_OK;
}

// The whole backbone on device buffers: canvas [n][64][gx * gy] (viewed as [64][H = gx][W = gy]) -> out
// [n][128][gy][gx], BB_CHUNK scans at a time.  f1 = block1, f2 = block2 (half), f3 = block3 (quarter); up1, up2, up3
// write their channels of the 448-channel concat buffer in place.
int backbone_run(gloc_pillar* h, const float* d_canvas, size_t n, int H, int W, float* d_out) {
  hipStream_t s = h->stream;
  const size_t nc = std::min(n, BB_CHUNK), hw = (size_t)H * W;
  const int H2 = bb_out_side(H, 2), W2 = bb_out_side(W, 2), H4 = bb_out_side(H2, 2), W4 = bb_out_side(W2, 2);
  GLOC_TRY(h->big.ensure(sizeof(float) * nc * 256 * hw, s));
  GLOC_TRY(h->a64.ensure(sizeof(float) * nc * 64 * hw, s));
  GLOC_TRY(h->f1.ensure(sizeof(float) * nc * 64 * hw, s));
  GLOC_TRY(h->cat.ensure(sizeof(float) * nc * 448 * hw, s));
  for (int i = 0; i < 2; ++i) {
    GLOC_TRY(h->half[i].ensure(sizeof(float) * nc * 128 * H2 * W2, s));
    GLOC_TRY(h->quarter[i].ensure(sizeof(float) * nc * 256 * H4 * W4, s));
  }
  float *big = h->big.as<float>(), *a64 = h->a64.as<float>(), *f1 = h->f1.as<float>(), *cat = h->cat.as<float>();
  float *t0 = h->half[0].as<float>(), *t1 = h->half[1].as<float>();
  float *q0 = h->quarter[0].as<float>(), *q1 = h->quarter[1].as<float>();
  for (size_t i0 = 0; i0 < n; i0 += BB_CHUNK) {
    const size_t m = std::min(BB_CHUNK, n - i0);
    GLOC_TRY(bb_layout(h, d_canvas + i0 * 64 * hw, m, 64, (int)hw, big));
    GLOC_TRY(bb_conv(h, 0, big, a64, m, H, W, 0));
    GLOC_TRY(bb_conv(h, 1, a64, f1, m, H, W, 0));   // f1
    GLOC_TRY(bb_conv(h, 2, f1, t0, m, H, W, 0));
    GLOC_TRY(bb_conv(h, 3, t0, t1, m, H2, W2, 0));
    GLOC_TRY(bb_conv(h, 4, t1, t0, m, H2, W2, 0));  // f2
    GLOC_TRY(bb_conv(h, 5, t0, q0, m, H2, W2, 0));
    GLOC_TRY(bb_conv(h, 6, q0, q1, m, H4, W4, 0));
    GLOC_TRY(bb_conv(h, 7, q1, q0, m, H4, W4, 0));  // f3
    GLOC_TRY(bb_conv(h, 8, f1, cat, m, H, W, 0, 448, 0));
    GLOC_TRY(bb_upsample(h, t0, m, H2, W2, 128, 2, big));
    GLOC_TRY(bb_conv(h, 9, big, cat, m, H, W, 0, 448, 64));
    GLOC_TRY(bb_upsample(h, q0, m, H4, W4, 256, 4, big));
    GLOC_TRY(bb_conv(h, 10, big, cat, m, H, W, 0, 448, 192));
    GLOC_TRY(bb_conv(h, 11, cat, big, m, H, W, 0));
    GLOC_TRY(bb_conv(h, 12, big, d_out + i0 * 128 * hw, m, H, W, BB_NCWH));
  }
  return GLOC_OK;
}

int features_device(gloc_pillar* h, const float* d_pts, const uint64_t* offsets, size_t n_scans, size_t stride,
                    const gloc_pillar_params* p, float* d_out) {
  Grid g;
  GLOC_TRY(make_grid(p, &g));
  GLOC_REQUIRE(g.size[2] == 1, GLOC_ERR_INVALID, "the backbone views the canvas as [64][gx][gy]: zbound must give one cell");
  GLOC_TRY(bb_check_grid(n_scans, (uint32_t)g.size[0], (uint32_t)g.size[1]));
  GLOC_TRY(check_batch(d_pts, offsets, n_scans, stride, p, d_out));
  GLOC_TRY(bb_check_layers(h));
  GLOC_HIP(hipSetDevice(h->device));
  GLOC_TRY(h->canvas.ensure(sizeof(float) * n_scans * FEAT * g.nv, h->stream));
  GLOC_TRY(canvas_device(h, d_pts, offsets, n_scans, stride, p, h->canvas.as<float>()));
  return backbone_run(h, h->canvas.as<float>(), n_scans, g.size[0], g.size[1], d_out);
}

// host buffers: stage the points, run the device call, copy `out_floats_per_scan` floats per scan back
template <typename F>
int host_call(gloc_pillar* h, const float* pts, const uint64_t* offsets, size_t n_scans, size_t stride,
              const gloc_pillar_params* p, float* out, size_t out_floats, F&& dev) {
  GLOC_REQUIRE(h && p && out && offsets, GLOC_ERR_INVALID, "NULL argument");
  GLOC_REQUIRE(n_scans > 0 && n_scans <= 65535, GLOC_ERR_INVALID, "n_scans must be in [1, 65535]");
  GLOC_REQUIRE(stride >= 4 && stride <= 64, GLOC_ERR_INVALID, "stride_floats must be in [4, 64]");
  GLOC_REQUIRE(offsets[n_scans] == 0 || pts, GLOC_ERR_INVALID, "points pointer is NULL");
  GLOC_HIP(hipSetDevice(h->device));
  return h->stage.call(h->stream, pts, sizeof(float) * offsets[n_scans] * stride, out, sizeof(float) * out_floats,
                       [&](void* d_in, void* d_out) { return dev(h, (const float*)d_in, offsets, n_scans, stride, p, (float*)d_out); });
}

}  // namespace

extern "C" {

int gloc_pillar_default_params(gloc_pillar_params* p) {
  GLOC_REQUIRE(p, GLOC_ERR_INVALID, "params is NULL");
  std::memset(p, 0, sizeof(*p));
  const float xb[3] = {-35.f, 35.f, 0.5f}, yb[3] = {-20.f, 20.f, 0.5f}, zb[3] = {-10.f, 10.f, 20.f};
  std::memcpy(p->xbound, xb, sizeof(xb));  // gen_libtorch_pointpillar.py:27
  std::memcpy(p->ybound, yb, sizeof(yb));  // :28
  std::memcpy(p->zbound, zb, sizeof(zb));  // :29
  p->num_points = 122480;                  // dataset/kitti_s2s.py:222-227, s2s_libtorch/s2s_feature_extract.cpp:143
  p->mask_mode = GLOC_PILLAR_MASK_INPUT;   // the traced model: input channel 15 (model/s2s_merged.py:204-206)
  return GLOC_OK;
}

int gloc_pillar_create(int device, gloc_pillar** out) { return create_handle(device, out); }

int gloc_pillar_destroy(gloc_pillar* h) { return destroy_handle(h); }

int gloc_pillar_set_stream(gloc_pillar* h, void* hip_stream) { return handle_set_stream(h, hip_stream); }

int gloc_pillar_synchronize(gloc_pillar* h) { return handle_synchronize(h); }

int gloc_pillar_set_pointnet(gloc_pillar* h, const float* w, const float* bn_weight, const float* bn_bias,
                             const float* bn_mean, const float* bn_var, float eps) {
  GLOC_REQUIRE(h && w && bn_weight && bn_bias && bn_mean && bn_var, GLOC_ERR_INVALID, "NULL argument");
  GLOC_REQUIRE(eps >= 0.f && std::isfinite(eps), GLOC_ERR_INVALID, "eps must be finite and >= 0");
  Pn pn;
  for (int c = 0; c < FEAT; ++c) {
    for (int k = 0; k < IN_CH; ++k) pn.w[c][k] = w[c * IN_CH + k];
    // BatchNorm1d in eval mode folded into one scale and shift per channel (in double, then rounded once)
    const double sc = (double)bn_weight[c] / std::sqrt((double)bn_var[c] + (double)eps);
    pn.scale[c] = (float)sc;
    pn.shift[c] = (float)((double)bn_bias[c] - (double)bn_mean[c] * sc);
  }
  GLOC_HIP(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  GLOC_TRY(h->pn.ensure(sizeof(Pn), s));
  GLOC_HIP(hipMemcpyAsync(h->pn.p, &pn, sizeof(Pn), hipMemcpyHostToDevice, s));
  GLOC_HIP(hipStreamSynchronize(s));  // pn lives on this stack frame
  h->have_pn = true;
  return GLOC_OK;
}

int gloc_pillar_inputs(gloc_pillar* h, const float* pts, const uint64_t* offsets, size_t n_scans, size_t stride_floats,
                       const gloc_pillar_params* p, float* out) {
  GLOC_REQUIRE(p, GLOC_ERR_INVALID, "params is NULL");
  return host_call(h, pts, offsets, n_scans, stride_floats, p, out, n_scans * (size_t)p->num_points * 16, inputs_device);
}

int gloc_pillar_inputs_device(gloc_pillar* h, const float* d_pts, const uint64_t* offsets, size_t n_scans,
                              size_t stride_floats, const gloc_pillar_params* p, float* d_out) {
  GLOC_REQUIRE(h, GLOC_ERR_INVALID, "handle is NULL");
  return inputs_device(h, d_pts, offsets, n_scans, stride_floats, p, d_out);
}

int gloc_pillar_canvas(gloc_pillar* h, const float* pts, const uint64_t* offsets, size_t n_scans, size_t stride_floats,
                       const gloc_pillar_params* p, float* out) {
  Grid g;
  GLOC_TRY(make_grid(p, &g));
  return host_call(h, pts, offsets, n_scans, stride_floats, p, out, n_scans * (size_t)FEAT * g.nv, canvas_device);
}

int gloc_pillar_canvas_device(gloc_pillar* h, const float* d_pts, const uint64_t* offsets, size_t n_scans,
                              size_t stride_floats, const gloc_pillar_params* p, float* d_out) {
  GLOC_REQUIRE(h, GLOC_ERR_INVALID, "handle is NULL");
  return canvas_device(h, d_pts, offsets, n_scans, stride_floats, p, d_out);
}

int gloc_pillar_backbone_layer_shape(int layer, uint32_t* cin, uint32_t* cout, int* stride, int* relu) {
  GLOC_REQUIRE(layer >= 0 && layer < BB_LAYERS, GLOC_ERR_INVALID, "layer must be in [0, %d]", BB_LAYERS - 1);
  const BbLayer& L = BB[layer];
  if (cin) *cin = (uint32_t)L.cin;
  if (cout) *cout = (uint32_t)L.cout;
  if (stride) *stride = L.stride;
  if (relu) *relu = L.relu;
  return GLOC_OK;
}

int gloc_pillar_set_backbone_layer(gloc_pillar* h, int layer, const float* w, const float* bn_weight,
                                   const float* bn_bias, const float* bn_mean, const float* bn_var, float eps) {
  GLOC_REQUIRE(h && w && bn_weight && bn_bias && bn_mean && bn_var, GLOC_ERR_INVALID, "NULL argument");
  GLOC_REQUIRE(layer >= 0 && layer < BB_LAYERS, GLOC_ERR_INVALID, "layer must be in [0, %d]", BB_LAYERS - 1);
  GLOC_REQUIRE(eps >= 0.f && std::isfinite(eps), GLOC_ERR_INVALID, "eps must be finite and >= 0");
  const BbLayer& L = BB[layer];
  // BatchNorm2d in eval mode as one scale and shift per channel (in double, then rounded once)
  std::vector<float> sc(L.cout), sh(L.cout);
  for (int c = 0; c < L.cout; ++c) {
    const double k = (double)bn_weight[c] / std::sqrt((double)bn_var[c] + (double)eps);
    sc[c] = (float)k;
    sh[c] = (float)((double)bn_bias[c] - (double)bn_mean[c] * k);
  }
  GLOC_HIP(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  const size_t count = (size_t)L.cout * L.cin * 9;
  h->bset[layer] = false;
  GLOC_TRY(h->braw.ensure(sizeof(float) * count, s));
  GLOC_TRY(h->bw[layer].ensure(sizeof(uint16_t) * 2 * count, s));
  GLOC_TRY(h->bscale[layer].ensure(sizeof(float) * L.cout, s));
  GLOC_TRY(h->bshift[layer].ensure(sizeof(float) * L.cout, s));
  GLOC_HIP(hipMemcpyAsync(h->braw.p, w, sizeof(float) * count, hipMemcpyHostToDevice, s));
  GLOC_HIP(hipMemcpyAsync(h->bscale[layer].p, sc.data(), sizeof(float) * L.cout, hipMemcpyHostToDevice, s));
  GLOC_HIP(hipMemcpyAsync(h->bshift[layer].p, sh.data(), sizeof(float) * L.cout, hipMemcpyHostToDevice, s));
  const int chunks = L.cout * (9 * L.cin / 8);
  hipLaunchKernelGGL(bb_split_weights_kernel, dim3((chunks + 255) / 256), dim3(256), 0, s, h->braw.as<float>(), L.cout,
                     L.cin, h->bw[layer].as<u32x4>());
  GLOC_HIP(hipGetLastError());
  GLOC_HIP(hipStreamSynchronize(s));  // the host arrays may go once this returns
  h->bset[layer] = true;
  return GLOC_OK;
}

int gloc_pillar_backbone_device(gloc_pillar* h, const float* d_canvas, size_t n, uint32_t gx, uint32_t gy,
                                float* d_out) {
  GLOC_REQUIRE(h && d_canvas && d_out, GLOC_ERR_INVALID, "NULL argument");
  GLOC_TRY(bb_check_grid(n, gx, gy));
  GLOC_TRY(bb_check_layers(h));
  GLOC_HIP(hipSetDevice(h->device));
  return backbone_run(h, d_canvas, n, (int)gx, (int)gy, d_out);
}

int gloc_pillar_backbone_layer_device(gloc_pillar* h, int layer, const float* d_in, size_t n, uint32_t H, uint32_t W,
                                      float* d_out) {
  GLOC_REQUIRE(h && d_in && d_out, GLOC_ERR_INVALID, "NULL argument");
  GLOC_REQUIRE(layer >= 0 && layer < BB_LAYERS, GLOC_ERR_INVALID, "layer must be in [0, %d]", BB_LAYERS - 1);
  GLOC_REQUIRE(n >= 1 && n <= 65535, GLOC_ERR_INVALID, "n must be in [1, 65535]");
  const BbLayer& L = BB[layer];
  GLOC_REQUIRE(H >= 1 && W >= 1 && H <= BB_MAX_SIDE && W <= BB_MAX_SIDE && H * L.up <= BB_MAX_SIDE && W * L.up <= BB_MAX_SIDE, GLOC_ERR_INVALID,
               "H and W (after the upsample) must be in [1, %u]", BB_MAX_SIDE);
  GLOC_REQUIRE(h->bset[layer], GLOC_ERR_STATE, "backbone layer %d was never set (gloc_pillar_set_backbone_layer)",
               layer);
  GLOC_HIP(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  const size_t count = n * (size_t)L.cin * H * W;
  GLOC_TRY(h->lay_in.ensure(sizeof(float) * count, s));
  GLOC_TRY(bb_layout(h, d_in, n, L.cin, (int)(H * W), h->lay_in.as<float>()));
  const float* in = h->lay_in.as<float>();
  if (L.up > 1) {
    GLOC_TRY(h->lay_up.ensure(sizeof(float) * count * L.up * L.up, s));
    GLOC_TRY(bb_upsample(h, in, n, (int)H, (int)W, L.cin, L.up, h->lay_up.as<float>()));
    in = h->lay_up.as<float>();
  }
  return bb_conv(h, layer, in, d_out, n, (int)(H * L.up), (int)(W * L.up), BB_NCHW);
}

int gloc_pillar_upsample_device(gloc_pillar* h, const float* d_in, size_t n, uint32_t C, uint32_t H, uint32_t W,
                                uint32_t factor, float* d_out) {
  GLOC_REQUIRE(h && d_in && d_out, GLOC_ERR_INVALID, "NULL argument");
  GLOC_REQUIRE(n >= 1 && n <= 65535 && C >= 1 && C <= 4096, GLOC_ERR_INVALID, "n must be in [1, 65535], C in [1, 4096]");
  GLOC_REQUIRE(factor >= 1 && factor <= 8 && H >= 1 && W >= 1 && H * factor <= BB_MAX_SIDE && W * factor <= BB_MAX_SIDE,
               GLOC_ERR_INVALID, "factor must be in [1, 8] and H, W in [1, %u] after it", BB_MAX_SIDE);
  GLOC_HIP(hipSetDevice(h->device));
  // NCHW is NHWC with one channel and n * C images: the backbone's kernel, element for element
  return bb_upsample(h, d_in, n * C, (int)H, (int)W, 1, (int)factor, d_out);
}

int gloc_pillar_features(gloc_pillar* h, const float* pts, const uint64_t* offsets, size_t n_scans,
                         size_t stride_floats, const gloc_pillar_params* p, float* out) {
  Grid g;
  GLOC_TRY(make_grid(p, &g));
  return host_call(h, pts, offsets, n_scans, stride_floats, p, out, n_scans * (size_t)128 * g.nv, features_device);
}

int gloc_pillar_features_device(gloc_pillar* h, const float* d_pts, const uint64_t* offsets, size_t n_scans,
                                size_t stride_floats, const gloc_pillar_params* p, float* d_out) {
  GLOC_REQUIRE(h, GLOC_ERR_INVALID, "handle is NULL");
  return features_device(h, d_pts, offsets, n_scans, stride_floats, p, d_out);
}

int gloc_pillar_set_profile(gloc_pillar* h, int enable) { return handle_set_profile(h, enable); }

int gloc_pillar_profile(gloc_pillar* h, const char* kernel, double* total_ms, uint64_t* launches) {
  return handle_profile(h, kernel, total_ms, launches);
}

int gloc_pillar_profile_reset(gloc_pillar* h) { return handle_profile_reset(h); }

}  // extern "C"
