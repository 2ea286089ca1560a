// s2s_feature_extract -- drop-in for the reference's s2s_libtorch/s2s_feature_extract.cpp: PointPillar-NetVLAD scan
// descriptors through the C ABI only (include/gloc3d.h): scans -> model input + PointNet canvas -> 2-D backbone
// (gloc_pillar_features_device) -> NetVLAD-FC (gloc_vlad_forward_device), on one stream.
//
//   s2s_feature_extract WEIGHTS SCAN.bin [SCAN.bin ...]
//
// WEIGHTS: a GLOCPPW file (tools/export_pillar_weights.py, which documents the layout) in place of the traced
// s2s_kitti.pt.  Scans are KITTI .bin files (float32 x y z i); the grid and P = 122 480 are the reference's
// (:143,161-163; gloc_pillar_default_params).  Prints "Processing time per frame = ... sec" as the reference does (:228),
// the mean over the scans of the host time from a scan in host memory to its descriptor in host memory, after one
// untimed pass over the first scan.  GLOC_DUMP_DESCRIPTORS=FILE writes the descriptors [n][128] as a GLOCDESC file.
#include <hip/hip_runtime_api.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "gloc3d.h"
#include "gloc_io.hpp"

using namespace gloc_host;

namespace {

void check(int rc) {
  if (rc != GLOC_OK) throw std::runtime_error(gloc_last_error());
}
void hip_check(hipError_t e, const char* what) {
  if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}

struct Layer {
  uint32_t cout = 0, cin = 0;
  std::vector<float> w, bn_w, bn_b, mean, var;
  float eps = 0.f;
};

struct Weights {
  Layer pointnet;
  std::vector<Layer> backbone;
  uint32_t clusters = 0, dim = 0, out_dim = 0, has_bias = 0;
  std::vector<float> conv_w, conv_b, centroids, fc_w;
};

template <class T>
bool rd(std::ifstream& f, T* p, size_t count) {
  return count == 0 || (bool)f.read(reinterpret_cast<char*>(p), (std::streamsize)(count * sizeof(T)));
}

bool read_layer(std::ifstream& f, Layer& L, size_t taps) {
  uint32_t shape[2];
  if (!rd(f, shape, 2) || shape[0] == 0 || shape[0] > 4096 || shape[1] == 0 || shape[1] > 4096) return false;
  L.cout = shape[0];
  L.cin = shape[1];
  L.w.resize((size_t)L.cout * L.cin * taps);
  for (auto* v : {&L.bn_w, &L.bn_b, &L.mean, &L.var}) v->resize(L.cout);
  return rd(f, L.w.data(), L.w.size()) && rd(f, L.bn_w.data(), L.cout) && rd(f, L.bn_b.data(), L.cout) &&
         rd(f, L.mean.data(), L.cout) && rd(f, L.var.data(), L.cout) && rd(f, &L.eps, 1);
}

// false with a message in `err` for a file that is not a whole GLOCPPW version 1 file
bool read_weights(const std::string& path, Weights& W, std::string& err) {
  std::ifstream f(path, std::ifstream::in | std::ifstream::binary);
  char magic[8];
  uint32_t version = 0, layers = 0;
  if (!f.is_open()) return err = path + ": cannot open", false;
  if (!f.read(magic, 8) || std::memcmp(magic, "GLOCPPW\0", 8) != 0 || !rd(f, &version, 1) || version != 1)
    return err = path + ": not a GLOCPPW version 1 file (tools/export_pillar_weights.py writes one)", false;
  if (!read_layer(f, W.pointnet, 1) || !rd(f, &layers, 1) || layers != 13)
    return err = path + ": truncated or not 13 backbone layers", false;
  W.backbone.resize(layers);
  for (uint32_t l = 0; l < layers; ++l) {
    uint32_t cin = 0, cout = 0;
    gloc_pillar_backbone_layer_shape((int)l, &cin, &cout, nullptr, nullptr);
    if (!read_layer(f, W.backbone[l], 9) || W.backbone[l].cin != cin || W.backbone[l].cout != cout)
      return err = path + ": backbone layer " + std::to_string(l) + " is truncated or of the wrong shape", false;
  }
  uint32_t head[4];
  if (!rd(f, head, 4) || head[0] == 0 || head[0] > 4096 || head[1] != 128 || head[2] == 0 || head[2] > 65536)
    return err = path + ": truncated NetVLAD-FC header (the backbone gives 128 channels)", false;
  W.clusters = head[0];
  W.dim = head[1];
  W.out_dim = head[2];
  W.has_bias = head[3];
  const size_t KD = (size_t)W.clusters * W.dim;
  W.conv_w.resize(KD);
  W.conv_b.resize(W.has_bias ? W.clusters : 0);
  W.centroids.resize(KD);
  W.fc_w.resize(KD * W.out_dim);
  if (!rd(f, W.conv_w.data(), KD) || !rd(f, W.conv_b.data(), W.conv_b.size()) || !rd(f, W.centroids.data(), KD) ||
      !rd(f, W.fc_w.data(), W.fc_w.size()))
    return err = path + ": truncated NetVLAD-FC tensors", false;
  return true;
}

struct Model {
  gloc_pillar* pillar = nullptr;
  gloc_vlad* vlad = nullptr;
  hipStream_t stream = nullptr;
  float *d_pts = nullptr, *d_feat = nullptr, *d_desc = nullptr;
  size_t pts_cap = 0;
  gloc_pillar_params params;
  size_t hw = 0, out_dim = 0;

  explicit Model(const Weights& W, int device = 0) {
    try {
      check(gloc_pillar_create(device, &pillar));
      const Layer& pn = W.pointnet;
      check(gloc_pillar_set_pointnet(pillar, pn.w.data(), pn.bn_w.data(), pn.bn_b.data(), pn.mean.data(), pn.var.data(),
                                     pn.eps));
      for (int l = 0; l < 13; ++l) {
        const Layer& L = W.backbone[l];
        check(gloc_pillar_set_backbone_layer(pillar, l, L.w.data(), L.bn_w.data(), L.bn_b.data(), L.mean.data(),
                                             L.var.data(), L.eps));
      }
      check(gloc_vlad_create(device, W.dim, W.clusters, W.out_dim, W.conv_w.data(),
                             W.has_bias ? W.conv_b.data() : nullptr, W.centroids.data(), W.fc_w.data(), 1, &vlad));
      hip_check(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking), "hipStreamCreate");
      check(gloc_pillar_set_stream(pillar, stream));
      check(gloc_vlad_set_stream(vlad, stream));
      gloc_pillar_default_params(&params);
      const size_t gx = (size_t)((params.xbound[1] - params.xbound[0]) / params.xbound[2]);
      const size_t gy = (size_t)((params.ybound[1] - params.ybound[0]) / params.ybound[2]);
      hw = gx * gy;
      out_dim = W.out_dim;
      hip_check(hipMalloc(&d_feat, sizeof(float) * 128 * hw), "hipMalloc");
      hip_check(hipMalloc(&d_desc, sizeof(float) * out_dim), "hipMalloc");
    } catch (...) {
      release();
      throw;
    }
  }
  ~Model() { release(); }
  Model(const Model&) = delete;
  Model& operator=(const Model&) = delete;

  // one scan (x y z i rows) -> its descriptor
  void describe(const std::vector<float>& scan, float* out) {
    const size_t n = scan.size() / 4;
    if (n > pts_cap) {
      if (d_pts) hip_check(hipFree(d_pts), "hipFree");
      d_pts = nullptr;
      pts_cap = 0;
      hip_check(hipMalloc(&d_pts, sizeof(float) * 4 * n), "hipMalloc");
      pts_cap = n;
    }
    const uint64_t off[2] = {0, n};
    if (n) hip_check(hipMemcpyAsync(d_pts, scan.data(), sizeof(float) * 4 * n, hipMemcpyHostToDevice, stream), "upload");
    check(gloc_pillar_features_device(pillar, d_pts ? d_pts : d_feat, off, 1, 4, &params, d_feat));
    check(gloc_vlad_forward_device(vlad, d_feat, 1, hw, d_desc));
    hip_check(hipMemcpyAsync(out, d_desc, sizeof(float) * out_dim, hipMemcpyDeviceToHost, stream), "download");
    hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");
  }

  void release() {
    if (stream) (void)hipStreamSynchronize(stream);
    gloc_pillar_destroy(pillar);
    gloc_vlad_destroy(vlad);
    pillar = nullptr;
    vlad = nullptr;
    for (float** p : {&d_pts, &d_feat, &d_desc}) {
      if (*p) (void)hipFree(*p);
      *p = nullptr;
    }
    if (stream) (void)hipStreamDestroy(stream);
    stream = nullptr;
  }
};

}  // namespace

int main(int argc, char* argv[]) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: %s WEIGHTS SCAN.bin [SCAN.bin ...]\n  WEIGHTS: a GLOCPPW file "
                 "(tools/export_pillar_weights.py)\n", argv[0]);
    return 2;
  }
  Weights W;
  std::string err;
  if (!read_weights(argv[1], W, err)) {
    std::fprintf(stderr, "%s\n", err.c_str());
    return 1;
  }
  std::vector<std::vector<float>> scans;
  for (int i = 2; i < argc; ++i) {
    if (!std::ifstream(argv[i], std::ifstream::in | std::ifstream::binary).is_open()) {
      std::fprintf(stderr, "cannot open scan %s\n", argv[i]);
      return 1;
    }
    scans.push_back(read_lidar_kitti(argv[i]));
  }
  try {
    Model model(W);
    std::vector<float> desc(scans.size() * model.out_dim);
    model.describe(scans[0], desc.data());  // warm-up: first launches, buffer growth
    double sec = 0;
    for (size_t i = 0; i < scans.size(); ++i) {
      const auto t1 = std::chrono::steady_clock::now();
      model.describe(scans[i], desc.data() + i * model.out_dim);
      const auto t2 = std::chrono::steady_clock::now();
      sec += std::chrono::duration<double>(t2 - t1).count();
    }
    std::printf("Processing time per frame = %g sec\n", sec / (double)scans.size());
    if (const char* dump = std::getenv("GLOC_DUMP_DESCRIPTORS")) {
      if (!write_descriptors(dump, desc, scans.size(), model.out_dim)) {
        std::fprintf(stderr, "cannot write %s\n", dump);
        return 1;
      }
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "fatal: %s\n", e.what());
    return 1;
  }
  return 0;
}
