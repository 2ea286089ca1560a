// common.hip -- error reporting, device selection, device buffers, HIP-event profiler.
#include "common.hpp"

#include <algorithm>

namespace gloc {

char* err_buf() {
  static thread_local char buf[512] = {0};
  return buf;
}

void set_err(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(err_buf(), 512, fmt, ap);
  va_end(ap);
}

int select_device(int device) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) {
    set_err("no HIP device visible (%s): the gloc3d hot path has no CPU fallback",
            e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    return GLOC_ERR_NODEVICE;
  }
  if (device < 0 || device >= n) {
    set_err("device ordinal %d out of range [0,%d)", device, n);
    return GLOC_ERR_INVALID;
  }
  hipDeviceProp_t prop;
  GLOC_HIP(hipGetDeviceProperties(&prop, device));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    set_err("device %d is %s; this library is built for gfx950 (MI355X) only", device,
            prop.gcnArchName);
    return GLOC_ERR_NODEVICE;
  }
  GLOC_HIP(hipSetDevice(device));
  return GLOC_OK;
}

int DevBuf::ensure(size_t bytes, hipStream_t s, bool keep, size_t used) {
  if (bytes <= cap) return GLOC_OK;
  size_t ncap = cap ? cap : 256;
  while (ncap < bytes) ncap += ncap / 2 + 256;
  void* np = nullptr;
  GLOC_HIP(hipMalloc(&np, ncap));
  if (keep && p && used) {
    hipError_t e = hipMemcpyAsync(np, p, used, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
      (void)hipFree(np);  // the old buffer stays valid
      set_err("device buffer growth failed: %s", hipGetErrorString(e));
      return GLOC_ERR_HIP;
    }
  }
  if (p) GLOC_HIP(hipFree(p));
  p = np;
  cap = ncap;
  return GLOC_OK;
}

void DevBuf::release() {
  if (p) (void)hipFree(p);
  p = nullptr;
  cap = 0;
}

hipEvent_t Profiler::get_event() {
  if (!pool.empty()) {
    hipEvent_t e = pool.back();
    pool.pop_back();
    return e;
  }
  hipEvent_t e;
  (void)hipEventCreate(&e);
  return e;
}

void Profiler::begin(const char* name, hipStream_t s, bool joined) {
  Family& f = fam[name];
  Span sp;
  if (joined && tail && tail_s == s) {
    sp.a = tail;  // (recorded already, by the scope that ended here)
  } else {
    sp.a = get_event();
    (void)hipEventRecord(sp.a, s);
  }
  sp.b = get_event();
  tail = nullptr;  // (work follows: the next scope joins this one's end, not its start)
  f.open.push_back(sp);
}

void Profiler::end(const char* name, hipStream_t s, const char* also) {
  Family& f = fam[name];
  if (f.open.empty()) return;
  const Span sp = f.open.back();
  (void)hipEventRecord(sp.b, s);
  tail = sp.b;
  tail_s = s;
  f.launches++;
  if (also) {
    Family& g = fam[also];
    g.open.push_back(sp);
    g.launches++;
  }
  // bound the number of live events: fold when many are open
  size_t live = 0;
  for (auto& kv : fam) live += kv.second.open.size();
  if (live > 8192) (void)collect(s);
}

int Profiler::open_stamps(int device, unsigned long long* d_words, uint32_t cap) {
  if (ms_per_tick == 0) {
    int khz = 0;
    GLOC_HIP(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device));
    GLOC_REQUIRE(khz > 0, GLOC_ERR_HIP, "the device reports no wall clock rate");
    ms_per_tick = 1.0 / (double)khz;
  }
  slots.clear();  // (a batch that was closed and never folded is dropped)
  h_stamps = nullptr;
  d_stamps = d_words;
  stamp_cap = cap;
  tail = nullptr;
  stamping = true;
  return GLOC_OK;
}

unsigned long long* Profiler::next_stamp(const char* name, const char* also) {
  slots.push_back(Slot{name, also});
  return slots.size() < stamp_cap ? d_stamps + (slots.size() - 1) : nullptr;  // (the last word is the closing stamp's)
}

unsigned long long* Profiler::close_stamps(const unsigned long long* h_words) {
  stamping = false;
  h_stamps = h_words;
  return d_stamps + std::min<size_t>(slots.size(), stamp_cap - 1);
}

// Scope k lasted from its stamp to the next one there is (a scope that launched nothing left its word zero, and one
// past the array has none: counted, no time of its own).
void Profiler::fold_stamps() {
  if (!h_stamps) return;
  const size_t n = std::min<size_t>(slots.size(), stamp_cap - 1);
  for (size_t k = 0; k < slots.size(); ++k) {
    double ms = 0;
    if (k < n && h_stamps[k]) {
      size_t e = k + 1;
      while (e < n && !h_stamps[e]) ++e;
      if (h_stamps[e] > h_stamps[k]) ms = (double)(h_stamps[e] - h_stamps[k]) * ms_per_tick;
    }
    for (const char* name : {slots[k].name, slots[k].also}) {
      if (!name) continue;
      Family& f = fam[name];
      f.total_ms += ms;
      f.launches++;
    }
  }
  slots.clear();
  h_stamps = nullptr;
}

// The events of the open spans back into the pool, each ONCE (joined scopes and second families share events), and no
// span open any more; the tail goes with them.
void Profiler::release_open() {
  const size_t first = pool.size();
  for (auto& kv : fam) {
    for (Span& sp : kv.second.open) {
      pool.push_back(sp.a);
      pool.push_back(sp.b);
    }
    kv.second.open.clear();
  }
  std::sort(pool.begin() + first, pool.end());
  pool.erase(std::unique(pool.begin() + first, pool.end()), pool.end());
  tail = nullptr;
}

int Profiler::collect(hipStream_t s) {
  GLOC_HIP(hipStreamSynchronize(s));
  fold_stamps();
  for (auto& kv : fam)
    for (Span& sp : kv.second.open) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, sp.a, sp.b) == hipSuccess) kv.second.total_ms += ms;
    }
  release_open();
  return GLOC_OK;
}

void Profiler::reset() {
  release_open();
  for (auto& kv : fam) {
    kv.second.total_ms = 0;
    kv.second.launches = 0;
  }
}

void Profiler::destroy() {
  reset();
  for (hipEvent_t e : pool) (void)hipEventDestroy(e);
  pool.clear();
  fam.clear();
}

Handle::~Handle() {
  prof.destroy();
  if (own_stream) (void)hipStreamDestroy(own_stream);
}

int handle_open(Handle* h, int device) {
  h->device = device;
  hipError_t e = hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking);
  if (e != hipSuccess) {
    set_err("hipStreamCreate failed: %s", hipGetErrorString(e));
    return GLOC_ERR_HIP;
  }
  h->stream = h->own_stream;
  return GLOC_OK;
}

int handle_set_stream(Handle* h, void* hip_stream) {
  GLOC_TRY(handle_synchronize(h));
  h->stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : h->own_stream;
  return GLOC_OK;
}

int handle_synchronize(Handle* h) {
  GLOC_REQUIRE(h, GLOC_ERR_INVALID, "handle is NULL");
  GLOC_HIP(hipSetDevice(h->device));
  GLOC_HIP(hipStreamSynchronize(h->stream));
  return GLOC_OK;
}

int handle_set_profile(Handle* h, int enable) {
  GLOC_REQUIRE(h, GLOC_ERR_INVALID, "handle is NULL");
  h->prof.enabled = enable != 0;
  return GLOC_OK;
}

int handle_profile(Handle* h, const char* kernel, double* total_ms, uint64_t* launches) {
  GLOC_REQUIRE(h && kernel, GLOC_ERR_INVALID, "NULL argument");
  GLOC_HIP(hipSetDevice(h->device));
  GLOC_TRY(h->prof.collect(h->stream));
  auto it = h->prof.fam.find(kernel);
  if (total_ms) *total_ms = it == h->prof.fam.end() ? 0.0 : it->second.total_ms;
  if (launches) *launches = it == h->prof.fam.end() ? 0 : it->second.launches;
  return GLOC_OK;
}

int handle_profile_reset(Handle* h) {
  GLOC_REQUIRE(h, GLOC_ERR_INVALID, "handle is NULL");
  GLOC_HIP(hipSetDevice(h->device));
  GLOC_TRY(h->prof.collect(h->stream));
  h->prof.reset();
  return GLOC_OK;
}

}  // namespace gloc

extern "C" {

const char* gloc_last_error(void) { return gloc::err_buf(); }
int gloc_abi_version(void) { return GLOC3D_ABI_VERSION; }
int gloc_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

}  // extern "C"
