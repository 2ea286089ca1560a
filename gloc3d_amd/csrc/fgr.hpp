// fgr.hpp -- what reg.hip (which owns the registration handle and the pair lists) calls of fgr.hip: the Fast Global
// Registration of a batch of match lists (include/gloc3d.h R1 - R4).
#pragma once
#include "common.hpp"
#include "math3.hpp"

namespace gloc {
namespace fgr {

constexpr int NSYS = 27;                   // H's upper triangle (21, row-major) and g (6)

struct JobIn {
  uint32_t m, stream;  // the list's length and the sample stream
};

struct Result {
  double Td[12];      // the pose after the last completed update (R row-major 9, t 3)
  double d2;          // R2's D^2 (0 without an active pair)
  double system[NSYS];  // of the last update that was formed
  float Tf[12];       // Td rounded
  uint32_t inliers, n_tuples, updates;  // updates: those that completed
  int status;         // 0: all updates ran; 2: degenerate
};

struct Ws {  // a registration handle's workspace, made on first use
  DevBuf jobs;     // [job] JobIn: filled by the caller (reg.hip knows the job table)
  DevBuf bits;     // [job][ceil(tuple_tries / 64)] pass bits of the tuple test
  DevBuf mult;     // [job][ld] multiplicities
  DevBuf act;      // [job][ld] positions of the active pairs
  DevBuf results;  // [job] Result
  bool lds_attr = false;  // the GNC kernel's dynamic LDS limit has been raised (once per handle, and so per device)
};
void ws_free(Ws* w);

int check_params(const gloc_fgr_params* prm);

// The pair lists of a batch in the RANSAC stage's layout: w.jobs[c].m pairs at pairs[(c * ld + i) * 2 + {0, 1}], none
// longer than m_max (known on the host).
struct Batch {
  const reg::f32x4* pairs;
  size_t ld;
  uint32_t n_jobs, m_max;
};

// R1 - R4's numbers for every job, enqueued on s: w.results, and w.mult's rows.
int enqueue(hipStream_t s, Profiler& prof, Ws& w, const Batch& b, const gloc_fgr_params& prm);

}  // namespace fgr
}  // namespace gloc
