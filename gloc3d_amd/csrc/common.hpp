// common.hpp -- shared host-side plumbing for the gloc3d C ABI (error reporting, HIP checks,
// per-kernel profiler on HIP events or device stamps, device buffers).  gfx950 only; no CPU fallback anywhere.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/gloc3d.h"

namespace gloc {

char* err_buf();
void set_err(const char* fmt, ...);

#define GLOC_HIP(expr)                                                                    \
  do {                                                                                    \
    hipError_t e_ = (expr);                                                               \
    if (e_ != hipSuccess) {                                                               \
      ::gloc::set_err("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__,    \
                      __LINE__);                                                          \
      return (e_ == hipErrorOutOfMemory) ? GLOC_ERR_NOMEM : GLOC_ERR_HIP;                 \
    }                                                                                     \
  } while (0)

#define GLOC_REQUIRE(cond, code, ...)  \
  do {                                 \
    if (!(cond)) {                     \
      ::gloc::set_err(__VA_ARGS__);    \
      return (code);                   \
    }                                  \
  } while (0)

#define GLOC_TRY(expr)            \
  do {                            \
    int rc_ = (expr);             \
    if (rc_ != GLOC_OK) return rc_; \
  } while (0)

int select_device(int device);  // validates ordinal + gfx950, hipSetDevice

// Growable device buffer (never shrinks).  Keeps contents on growth if `keep`.  Owns its memory: freed when the
// buffer goes (with the owner's device current: see destroy_handle), or early by release().
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      release();
      p = o.p, cap = o.cap;
      o.p = nullptr, o.cap = 0;
    }
    return *this;
  }
  ~DevBuf() { release(); }
  int ensure(size_t bytes, hipStream_t s, bool keep = false, size_t used = 0);
  void release();
  template <class T>
  T* as() const {
    return reinterpret_cast<T*>(p);
  }
};

static_assert(!std::is_copy_constructible<DevBuf>::value && !std::is_copy_assignable<DevBuf>::value,
              "a DevBuf has one owner: two copies would free the same memory");

// Profiler: brackets kernel launches of one family with HIP events and sums elapsed time lazily -- or, for a batch whose
// kernels stamp the device clock themselves, takes the times from those stamps (below).
struct Profiler {
  bool enabled = false;
  struct Span {
    hipEvent_t a, b;
  };
  struct Family {
    std::vector<Span> open;
    double total_ms = 0;
    uint64_t launches = 0;
  };
  std::map<std::string, Family> fam;
  std::vector<hipEvent_t> pool;
  // The event the last end() recorded and its stream.  A scope that begins where that one ended -- `joined`: the caller
  // has enqueued NOTHING on the stream in between -- takes it as its start instead of recording another: one event, not
  // two, between two dependent kernels.  The idle gap between the kernels then counts for the later family.
  hipEvent_t tail = nullptr;
  hipStream_t tail_s = nullptr;
  // A device-stamped batch (the registration batch, reg.hip): no event between its kernels.  Every scope of it takes a
  // slot of a device array of 64-bit words -- the caller's, zero when the batch starts -- and the first work-group of the
  // scope's first kernel leaves the device's constant-rate clock there (stamp_launch, reg_kernels.hpp).  Kernels of one
  // stream run back to back, so scope k lasted stamp(k + 1) - stamp(k): the idle time and the runtime's fills and copies
  // behind a scope's kernels count for that scope, and the last scope ends at the stamp of a trivial kernel the caller
  // launches behind it (close_stamps).  The caller brings the words down with the batch's results and folds them.
  struct Slot {
    const char *name, *also;
  };
  bool stamping = false;          // between open_stamps and close_stamps: ProfScope hands out slots, records nothing
  unsigned long long* d_stamps = nullptr;
  uint32_t stamp_cap = 0;
  std::vector<Slot> slots;        // of the batch being enqueued, or enqueued last and not folded yet
  double ms_per_tick = 0;         // of the device clock (hipDeviceAttributeWallClockRate)
  int open_stamps(int device, unsigned long long* d_words, uint32_t cap);  // (the batch before has been folded)
  unsigned long long* next_stamp(const char* name, const char* also);      // null: no slot left (the batch's owner makes that an error)
  // the slot of the closing stamp; h_words: where the caller's copy leaves the slots' words and that one, on the host
  unsigned long long* close_stamps(const unsigned long long* h_words);
  void fold_stamps();  // once that copy has been waited for: the scopes into their families (no batch to fold: nothing)
  const unsigned long long* h_stamps = nullptr;  // set: a closed batch waits to be folded
  hipEvent_t get_event();
  void begin(const char* name, hipStream_t s, bool joined = false);
  // also: a second family that counts the same span (the same two events, no record of its own)
  void end(const char* name, hipStream_t s, const char* also = nullptr);
  int collect(hipStream_t s);  // sync + fold open spans into totals
  void release_open();
  void reset();
  void destroy();
};

struct ProfScope {
  enum Join { Apart, Joined };  // Joined: nothing was enqueued on the stream since the scope before this one ended
  Profiler& p;
  const char* name;
  hipStream_t s;
  const char* also;
  unsigned long long* stamp = nullptr;  // in a device-stamped batch: the scope's slot, for its first kernel
  ProfScope(Profiler& p_, const char* n, hipStream_t s_, Join j = Apart, const char* also_ = nullptr) : p(p_), name(n), s(s_), also(also_) {
    if (p.stamping) stamp = p.next_stamp(name, also);
    else if (p.enabled) p.begin(name, s, j == Joined);
  }
  ~ProfScope() {
    if (!p.stamping && p.enabled) p.end(name, s, also);
  }
};

// What every handle of the C ABI starts with: its device, the stream it enqueues on (its own unless the caller gave
// one), the per-kernel profiler.  Each `struct gloc_xxx` derives from it and adds what is its own; members that own
// device memory (DevBuf) free it themselves, and what is not of that kind (pinned memory, events, blocks of a cache,
// inner handles) goes in the struct's own destructor.
struct Handle {
  int device = 0;
  hipStream_t own_stream = nullptr, stream = nullptr;
  Profiler prof;
  Handle() = default;
  Handle(const Handle&) = delete;
  Handle& operator=(const Handle&) = delete;
  ~Handle();  // the profiler's events and the owned stream (runs after the derived handle's members have gone)
};

int handle_open(Handle* h, int device);  // the owned stream, made current; the device is selected already
int handle_set_stream(Handle* h, void* hip_stream);  // waits for the old stream; null: back to the owned one
int handle_synchronize(Handle* h);
int handle_set_profile(Handle* h, int enable);
int handle_profile(Handle* h, const char* kernel, double* total_ms, uint64_t* launches);
int handle_profile_reset(Handle* h);

// gloc_xxx_create: device selection, allocation, the owned stream.  *out is null on every failure.
template <class H>
int create_handle(int device, H** out) {
  GLOC_REQUIRE(out, GLOC_ERR_INVALID, "out is NULL");
  *out = nullptr;
  GLOC_TRY(select_device(device));
  H* h = new (std::nothrow) H();
  GLOC_REQUIRE(h, GLOC_ERR_NOMEM, "out of host memory");
  const int rc = handle_open(h, device);
  if (rc != GLOC_OK) {
    delete h;
    return rc;
  }
  *out = h;
  return GLOC_OK;
}

// gloc_xxx_destroy, once the module's own refusals (live views, attached handles) are past: the handle's work is waited
// for, then -- with its device current -- the struct's destructor lets go of what is not a DevBuf and the members free
// their memory.  (The wait is here and not in ~Handle: a base's destructor runs after the derived members have gone.)
template <class H>
int destroy_handle(H* h) {
  if (!h) return GLOC_OK;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);
  delete h;
  return GLOC_OK;
}

// A workspace that a handle makes on first use: *slot is filled if it is still null.
template <class W>
int ensure_ws(W** slot) {
  if (!*slot) *slot = new (std::nothrow) W;
  GLOC_REQUIRE(*slot, GLOC_ERR_NOMEM, "host allocation failed");
  return GLOC_OK;
}

// The host-pointer form of a device entry point: `src` goes up into the first staging buffer (never null: an empty
// input still gets 16 bytes), run(d_in, d_out) enqueues the device form on `s`, the second staging buffer comes down into
// `dst`, and the stream is waited for.
struct Staging {
  DevBuf in, out;
  template <class F>
  int call(hipStream_t s, const void* src, size_t in_bytes, void* dst, size_t out_bytes, F&& run) {
    GLOC_TRY(in.ensure(in_bytes > 16 ? in_bytes : 16, s));
    GLOC_TRY(out.ensure(out_bytes, s));
    if (in_bytes) GLOC_HIP(hipMemcpyAsync(in.p, src, in_bytes, hipMemcpyHostToDevice, s));
    GLOC_TRY(run(in.p, out.p));
    GLOC_HIP(hipMemcpyAsync(dst, out.p, out_bytes, hipMemcpyDeviceToHost, s));
    GLOC_HIP(hipStreamSynchronize(s));
    return GLOC_OK;
  }
};

}  // namespace gloc
