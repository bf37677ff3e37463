// pipeline_util.h — what pipeline.cpp (runtime) and submit.cpp (batch planner) share.
#pragma once
#include <string>
#include <vector>

#include "pipeline.h"

namespace dg {

void set_error(const std::string &s);

#define HIPCHK(x)                                                                          \
  do {                                                                                     \
    hipError_t e_ = (x);                                                                   \
    if (e_ != hipSuccess) {                                                                \
      set_error(std::string("HIP error: ") + hipGetErrorString(e_) + " at " #x);          \
      return DG_ERR_DEVICE;                                                                \
    }                                                                                      \
  } while (0)

static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// submit(): the batch does not fit the device (budget or allocation); the
// caller splits it (submit_split).  Never returned through the C ABI.
static constexpr dg_status kNeedSplit = (dg_status)15;  // (inside the enum's value range)

// Table pool sizes (see flush_pools): a pool above kPoolKeep tables starts
// over at the next submit; no pool ever holds more than kPoolMax.
static constexpr size_t kPoolKeep = 16384;
static constexpr size_t kPoolMax = 65535;

// Host-side copies of a finished batch's outputs (pinned staging -> the
// caller's buffers, ~3 MB per 1024-bucket image): split into 1 MiB pieces
// and spread over up to `nthreads` threads -- one thread's memcpy (~6-8 GB/s)
// was the limit of the host-in/host-out path, not PCIe.
struct CopyJob {
  void *dst;
  const void *src;
  size_t n;
};
void parallel_copy(const std::vector<CopyJob> &jobs, int nthreads);

}  // namespace dg
