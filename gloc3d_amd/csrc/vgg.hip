// vgg.hip -- C ABI of the VGG16 place-descriptor encoder (include/gloc3d.h, "VGG16 encoder").
// Replaces the encoder of the reference's i2i model, VGG16 features[:-2] (s2s_libtorch/gen_libtorch_i2i.py:36-60,
// main.py:531-541), the head of the TorchScript module RpyPCLoopDetector::get_place_feature runs
// (registration/loop_detector.cpp:137-172).  Kernels and precision: vgg_kernels.hpp.
#include <algorithm>

#include "common.hpp"
#include "vgg_kernels.hpp"

using namespace gloc;
using namespace gloc::vgg;

namespace {

constexpr int NLAYERS = 13;
struct LayerDef {
  int cin, cout;
  bool relu, pool;
};
// VGG16 features[:-2]: the last convolution keeps neither its ReLU nor the pool after it
constexpr LayerDef LAYERS[NLAYERS] = {
    {3, 64, true, false},    {64, 64, true, true},    {64, 128, true, false},  {128, 128, true, true},
    {128, 256, true, false}, {256, 256, true, false}, {256, 256, true, true},  {256, 512, true, false},
    {512, 512, true, false}, {512, 512, true, true},  {512, 512, true, false}, {512, 512, true, false},
    {512, 512, false, false}};
const char* const FAMILY[NLAYERS] = {"vgg_conv0", "vgg_conv1", "vgg_conv2",  "vgg_conv3",  "vgg_conv4",
                                     "vgg_conv5", "vgg_conv6", "vgg_conv7",  "vgg_conv8",  "vgg_conv9",
                                     "vgg_conv10", "vgg_conv11", "vgg_conv12"};
constexpr size_t CHUNK = 8;  // images per pass through the network (bounds the two activation buffers)
constexpr uint32_t MAX_SIDE = 8192;

int kpad(int cin) { return (9 * cin + BK - 1) / BK * BK; }

}  // namespace

struct gloc_vgg : Handle {
  DevBuf w[NLAYERS], b[NLAYERS];  // split weights [Cout][Kp / 8][h | m], bias [Cout]
  bool set[NLAYERS] = {};
  DevBuf act[2], nhwc, raw;       // activations (NHWC), the per-layer call's channels-last input, raw weights
  Staging stage;                  // host-pointer API staging
  bool lds_attr_set[3] = {};       // dynamic-LDS limit raised for <2,1,true>, <2,1,false>, <2,2,false>
};

namespace {

template <int WM, int WN, bool CIN3>
int launch(gloc_vgg* h, int layer, const float* in, float* out, size_t n, int H, int W, int epi) {
  const LayerDef& L = LAYERS[layer];
  constexpr int BN = 64 * WN, TROWS = 4 * WM;
  constexpr int lds = conv_lds_bytes<WM, WN>();
  auto kern = vgg_conv_kernel<WM, WN, CIN3>;
  constexpr int slot = CIN3 ? 0 : WN;  // the three instantiations conv() launches
  if (!h->lds_attr_set[slot]) {        // once per handle (and so per device)
    GLOC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    h->lds_attr_set[slot] = true;
  }
  const int tiles_x = (W + 15) / 16, tiles_y = (H + TROWS - 1) / TROWS;
  ProfScope ps(h->prof, FAMILY[layer], h->stream);
  hipLaunchKernelGGL(kern, dim3(tiles_x * tiles_y, L.cout / BN, (unsigned)n), dim3(256), lds, h->stream, in,
                     h->w[layer].as<u32x4>(), h->b[layer].as<float>(), out, H, W, L.cin, L.cout, kpad(L.cin), tiles_x,
                     epi);
  GLOC_HIP(hipGetLastError());
  return GLOC_OK;
}

// in: NCHW for layer 0, NHWC otherwise; out NHWC, or NCHW when `nchw`
int conv(gloc_vgg* h, int layer, const float* in, float* out, size_t n, int H, int W, bool nchw) {
  const LayerDef& L = LAYERS[layer];
  const int epi = (L.relu ? EPI_RELU : 0) | (L.pool ? EPI_POOL : 0) | (nchw ? EPI_NCHW : 0);
  if (layer == 0) return launch<2, 1, true>(h, layer, in, out, n, H, W, epi);
  if (L.cout == 64) return launch<2, 1, false>(h, layer, in, out, n, H, W, epi);
  return launch<2, 2, false>(h, layer, in, out, n, H, W, epi);
}

int check_layers(gloc_vgg* h, int first, int last) {
  for (int l = first; l <= last; ++l)
    GLOC_REQUIRE(h->set[l], GLOC_ERR_STATE, "weights of layer %d were never set (gloc_vgg_set_layer)", l);
  return GLOC_OK;
}

int check_sizes(size_t n, uint32_t H, uint32_t W) {
  GLOC_REQUIRE(n >= 1 && n <= 65535, GLOC_ERR_INVALID, "n must be in [1, 65535]");
  GLOC_REQUIRE(H >= 1 && W >= 1 && H <= MAX_SIDE && W <= MAX_SIDE, GLOC_ERR_INVALID, "H and W must be in [1, %u]",
               MAX_SIDE);
  return GLOC_OK;
}

// The whole network on device buffers: images [n][3][H][W] -> out [n][512][H / 16][W / 16], CHUNK images at a time.
int forward_device(gloc_vgg* h, const float* d_images, size_t n, int H, int W, float* d_out) {
  hipStream_t s = h->stream;
  const size_t nc = std::min(n, CHUNK);
  const size_t act_bytes = sizeof(float) * nc * (size_t)H * W * 64;  // the largest activation: conv1_1's output
  GLOC_TRY(h->act[0].ensure(act_bytes, s));
  GLOC_TRY(h->act[1].ensure(act_bytes, s));
  const size_t in_per = (size_t)3 * H * W, out_per = (size_t)512 * (H / 16) * (W / 16);
  for (size_t i0 = 0; i0 < n; i0 += CHUNK) {
    const size_t m = std::min(CHUNK, n - i0);
    const float* in = d_images + i0 * in_per;
    int hh = H, ww = W;
    for (int l = 0; l < NLAYERS; ++l) {
      const bool last = l == NLAYERS - 1;
      float* out = last ? d_out + i0 * out_per : h->act[l & 1].as<float>();
      GLOC_TRY(conv(h, l, in, out, m, hh, ww, last));
      if (LAYERS[l].pool) hh /= 2, ww /= 2;
      in = out;
    }
  }
  return GLOC_OK;
}

}  // namespace

extern "C" {

int gloc_vgg_create(int device, gloc_vgg** out) { return create_handle(device, out); }

int gloc_vgg_destroy(gloc_vgg* h) { return destroy_handle(h); }

int gloc_vgg_set_stream(gloc_vgg* h, void* hip_stream) { return handle_set_stream(h, hip_stream); }

int gloc_vgg_synchronize(gloc_vgg* h) { return handle_synchronize(h); }

int gloc_vgg_layer_shape(int layer, uint32_t* cin, uint32_t* cout, int* relu, int* pool) {
  GLOC_REQUIRE(layer >= 0 && layer < NLAYERS, GLOC_ERR_INVALID, "layer must be in [0, %d]", NLAYERS - 1);
  const LayerDef& L = LAYERS[layer];
  if (cin) *cin = (uint32_t)L.cin;
  if (cout) *cout = (uint32_t)L.cout;
  if (relu) *relu = L.relu;
  if (pool) *pool = L.pool;
  return GLOC_OK;
}

int gloc_vgg_set_layer(gloc_vgg* h, int layer, const float* w, const float* b) {
  GLOC_REQUIRE(h, GLOC_ERR_INVALID, "handle is NULL");
  GLOC_REQUIRE(layer >= 0 && layer < NLAYERS, GLOC_ERR_INVALID, "layer must be in [0, %d]", NLAYERS - 1);
  GLOC_REQUIRE(w && b, GLOC_ERR_INVALID, "weights and bias are required");
  GLOC_HIP(hipSetDevice(h->device));
  const LayerDef& L = LAYERS[layer];
  const int Kp = kpad(L.cin);
  const size_t count = (size_t)L.cout * L.cin * 9;
  hipStream_t s = h->stream;
  h->set[layer] = false;
  GLOC_TRY(h->raw.ensure(sizeof(float) * count, s));
  GLOC_TRY(h->w[layer].ensure(sizeof(uint16_t) * 2 * (size_t)L.cout * Kp, s));
  GLOC_TRY(h->b[layer].ensure(sizeof(float) * L.cout, s));
  GLOC_HIP(hipMemcpyAsync(h->raw.p, w, sizeof(float) * count, hipMemcpyHostToDevice, s));
  GLOC_HIP(hipMemcpyAsync(h->b[layer].p, b, sizeof(float) * L.cout, hipMemcpyHostToDevice, s));
  const int chunks = L.cout * (Kp / 8);
  hipLaunchKernelGGL(vgg_split_weights_kernel, dim3((chunks + 255) / 256), dim3(256), 0, s, h->raw.as<float>(), L.cout,
                     L.cin, Kp, h->w[layer].as<u32x4>());
  GLOC_HIP(hipGetLastError());
  GLOC_HIP(hipStreamSynchronize(s));  // the host arrays may go once this returns
  h->set[layer] = true;
  return GLOC_OK;
}

int gloc_vgg_forward_device(gloc_vgg* h, const float* d_images, size_t n, uint32_t H, uint32_t W, float* d_out) {
  GLOC_REQUIRE(h && d_images && d_out, GLOC_ERR_INVALID, "NULL argument");
  GLOC_TRY(check_sizes(n, H, W));
  GLOC_REQUIRE(H % 16 == 0 && W % 16 == 0, GLOC_ERR_INVALID, "H and W must be multiples of 16 (got %u x %u)", H, W);
  GLOC_TRY(check_layers(h, 0, NLAYERS - 1));
  GLOC_HIP(hipSetDevice(h->device));
  return forward_device(h, d_images, n, (int)H, (int)W, d_out);
}

int gloc_vgg_forward(gloc_vgg* h, const float* images, size_t n, uint32_t H, uint32_t W, float* out) {
  GLOC_REQUIRE(h && images && out, GLOC_ERR_INVALID, "NULL argument");
  GLOC_TRY(check_sizes(n, H, W));
  GLOC_REQUIRE(H % 16 == 0 && W % 16 == 0, GLOC_ERR_INVALID, "H and W must be multiples of 16 (got %u x %u)", H, W);
  GLOC_TRY(check_layers(h, 0, NLAYERS - 1));
  GLOC_HIP(hipSetDevice(h->device));
  const size_t in_count = n * 3 * (size_t)H * W, out_count = n * 512 * (size_t)(H / 16) * (W / 16);
  return h->stage.call(h->stream, images, sizeof(float) * in_count, out, sizeof(float) * out_count, [&](void* d_in, void* d_out) {
    return forward_device(h, (const float*)d_in, n, (int)H, (int)W, (float*)d_out);
  });
}

int gloc_vgg_forward_layer(gloc_vgg* h, int layer, const float* d_in, size_t n, uint32_t H, uint32_t W, float* d_out) {
  GLOC_REQUIRE(h && d_in && d_out, GLOC_ERR_INVALID, "NULL argument");
  GLOC_REQUIRE(layer >= 0 && layer < NLAYERS, GLOC_ERR_INVALID, "layer must be in [0, %d]", NLAYERS - 1);
  GLOC_TRY(check_sizes(n, H, W));
  const LayerDef& L = LAYERS[layer];
  GLOC_REQUIRE(!L.pool || (H % 2 == 0 && W % 2 == 0), GLOC_ERR_INVALID, "layer %d pools: H and W must be even", layer);
  GLOC_TRY(check_layers(h, layer, layer));
  GLOC_HIP(hipSetDevice(h->device));
  const float* in = d_in;
  if (layer > 0) {
    const size_t count = n * (size_t)L.cin * H * W;
    GLOC_TRY(h->nhwc.ensure(sizeof(float) * count, h->stream));
    ProfScope ps(h->prof, "vgg_layout", h->stream);
    hipLaunchKernelGGL(vgg_nchw_to_nhwc_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, h->stream, d_in, n,
                       L.cin, (int)(H * W), h->nhwc.as<float>());
    GLOC_HIP(hipGetLastError());
    in = h->nhwc.as<float>();
  }
  return conv(h, layer, in, d_out, n, (int)H, (int)W, true);
}

int gloc_vgg_set_profile(gloc_vgg* h, int enable) { return handle_set_profile(h, enable); }

int gloc_vgg_profile(gloc_vgg* h, const char* kernel, double* total_ms, uint64_t* launches) {
  return handle_profile(h, kernel, total_ms, launches);
}

int gloc_vgg_profile_reset(gloc_vgg* h) { return handle_profile_reset(h); }

}  // extern "C"
