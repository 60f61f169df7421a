// cox_plan.h -- the survival plan that cox.hip makes (osd_val_cox_plan_create) and that cox.hip and cox_score.hip follow: what
// depends on a cohort's (time, event) columns alone, by position p in descending-time order.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <mutex>
#include "handle.h"

namespace osd {

constexpr int COX_MAX_D = 8192;
constexpr int COX_MAX_DEVICES = 64;

struct CoxPlan {
  int device = 0;
  hipStream_t stream = nullptr;
  int64_t rows = 0;
  DevBuf<int> order, gstart, gend;       // by position in descending time: the row, the first and the last position of its tie group
  DevBuf<unsigned char> ev;              // the event flag of the position
  DevBuf<int> gev;                       // the events of the tie group that ENDS at the position, 0 anywhere else (cox_score.hip)
};

// A grow-only device workspace, one per device and entry point, held for the length of a call: a fit or a screen's Newton
// iterations call again and again.  Its pieces start at multiples of 256 bytes.
struct CoxWorkspace {
  std::mutex mu;
  DevBuf<char> buf;
};

inline size_t up256(size_t v) { return (v + 255) / 256 * 256; }

}  // namespace osd
