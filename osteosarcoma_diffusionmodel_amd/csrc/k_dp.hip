// k_dp.hip -- differentially private training (dp.h): the per-row gradient-norm launch, the clip-factor launch, their cached item
// lists, and the entry points that set the option and read the norms back.  Both kernels are HBM-bound row walks: a wave owns one
// batch row across every item, reads it with 16-byte loads, reduces across its lanes and writes once -- no atomics, so two calls on
// the same inputs give the same bits.
#include <string.h>
#include <cmath>
#include "dp.h"
#include "handle.h"

namespace osd {

__device__ __forceinline__ float dp_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// this lane's share of sum_i p[i]^2, i < k: float4 loads where the row starts on a 16-byte boundary (every workspace row whose width is a
// multiple of four; rows of an odd width D only every fourth), scalar loads for the tail / otherwise
__device__ __forceinline__ float dp_lane_sumsq(const float* __restrict__ p, int k, int lane) {
  float s = 0.f;
  int done = 0;
  if ((reinterpret_cast<uintptr_t>(p) & 15) == 0) {
    const int k4 = k >> 2;
    const float4* p4 = reinterpret_cast<const float4*>(p);
    for (int i = lane; i < k4; i += 64) {
      const float4 v = p4[i];
      s += (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
    }
    done = 4 * k4;
  }
  for (int i = done + lane; i < k; i += 64) { const float v = p[i]; s += v * v; }
  return s;
}

__global__ __launch_bounds__(256) void k_dp_row_norms(const DpNormItem* __restrict__ items, int n_items, int64_t rows, float unscale, float clip,
                                                      float* __restrict__ norms, float* __restrict__ factors, const float* __restrict__ cond,
                                                      const int* __restrict__ gather) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;                       // whole waves leave: nothing below synchronises the block
  float total = 0.f;
  for (int i = 0; i < n_items; ++i) {
    const DpNormItem& it = items[i];            // the same for every lane: scalar loads
    if (it.kind == 0) {
      float sx = 0.f;
#pragma unroll
      for (int j = 0; j < 3; ++j)
        if (it.k[j] > 0) {
          const float* x = (j == 0 && it.x0_is_cond) ? cond : it.x[j];
          const int64_t row = (j == 2 && it.gathered) ? (int64_t)gather[r] : r;
          sx += dp_lane_sumsq(x + row * it.ldx[j], it.k[j], lane);
        }
      const float sd = dp_lane_sumsq(it.d + r * it.ldd, it.nd, lane);
      total += (dp_wave_sum(sx) + it.nbias) * dp_wave_sum(sd);
    } else {
      const int C = it.nd, ngrp = C / it.gw;    // C and gw are multiples of four and the rows 16-byte aligned (dp_supported on the host)
      const float* gy = it.d + r * it.ldd;
      const float* z = it.z + r * it.ldd;
      const float* st = it.stats + r * ngrp * 2;
      float s = 0.f;
      for (int c = 4 * lane; c < C; c += 256) {
        const float4 g4 = *reinterpret_cast<const float4*>(gy + c);
        const float4 z4 = *reinterpret_cast<const float4*>(z + c);
        const float2 ms = *reinterpret_cast<const float2*>(st + (c / it.gw) * 2);
        const float a0 = g4.x * ((z4.x - ms.x) * ms.y), a1 = g4.y * ((z4.y - ms.x) * ms.y);
        const float a2 = g4.z * ((z4.z - ms.x) * ms.y), a3 = g4.w * ((z4.w - ms.x) * ms.y);
        s += ((a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3)) + ((g4.x * g4.x + g4.y * g4.y) + (g4.z * g4.z + g4.w * g4.w));
      }
      total += dp_wave_sum(s);
    }
  }
  if (lane == 0) {
    const float nr = unscale * sqrtf(total);
    float c = clip / (nr + 1e-6f);
    if (!(c < 1.0f)) c = 1.0f;
    norms[r] = nr;
    factors[r] = c;
  }
}

__global__ __launch_bounds__(256) void k_dp_scale_rows(const DpScaleItem* __restrict__ items, int n_items, int64_t rows, const float* __restrict__ factors) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const float c = factors[r];
  if (c == 1.0f) return;                       // an unclipped row: nothing to read or write
  for (int i = 0; i < n_items; ++i) {
    const DpScaleItem it = items[i];
    float* p = it.p + r * it.ld;
    int done = 0;
    if ((reinterpret_cast<uintptr_t>(p) & 15) == 0) {
      const int k4 = it.cols >> 2;
      float4* p4 = reinterpret_cast<float4*>(p);
      for (int j = lane; j < k4; j += 64) {
        float4 v = p4[j];
        v.x *= c; v.y *= c; v.z *= c; v.w *= c;
        p4[j] = v;
      }
      done = 4 * k4;
    }
    for (int j = done + lane; j < it.cols; j += 64) p[j] *= c;
  }
}

hipError_t launch_dp_row_norms(hipStream_t s, const DpNormItem* d_items, int n_items, int64_t rows, float unscale, float clip, float* norms, float* factors,
                               const float* cond, const int* gather) {
  if (rows <= 0 || n_items <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_dp_row_norms, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, d_items, n_items, rows, unscale, clip, norms, factors, cond, gather);
  return hipGetLastError();
}
hipError_t launch_dp_scale_rows(hipStream_t s, const DpScaleItem* d_items, int n_items, int64_t rows, const float* factors) {
  if (rows <= 0 || n_items <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_dp_scale_rows, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, d_items, n_items, rows, factors);
  return hipGetLastError();
}

// the item lists as the device holds them (devmem.h: DevList)
struct DpPlan {
  const float* cond = nullptr; const int* gather = nullptr;      // the last launch's arguments (osd_dp_replay)
  DevList<DpNormItem> norms;
  DevList<DpScaleItem> scales;
};

// the callers memset every item before filling it, so padding bytes compare equal
template <class E> static bool same_bytes(const E& a, const E& b) { return memcmp(&a, &b, sizeof(E)) == 0; }

int dp_clip_rows(osd_handle* h, hipStream_t s, const std::vector<DpNormItem>& norms, const std::vector<DpScaleItem>& scales, int64_t rows, double unscale,
                 const float* cond, const int* gather) {
  if (!h->dp_plan) h->dp_plan = new DpPlan();
  DpPlan* pl = static_cast<DpPlan*>(h->dp_plan);
  OSD_TRY(h->dp_norms.reserve(2 * ((rows + 1023) / 1024 * 1024), s));      // 1024-row granules
  OSD_TRY(pl->norms.upload(s, norms, same_bytes<DpNormItem>));
  OSD_TRY(pl->scales.upload(s, scales, same_bytes<DpScaleItem>));
  float* factors = h->dp_norms + h->dp_norms.cap() / 2;
  OSD_HIP(launch_dp_row_norms(s, pl->norms.dev, (int)pl->norms.kept.size(), rows, (float)unscale, (float)h->dp_clip, h->dp_norms, factors, cond, gather));
  OSD_HIP(launch_dp_scale_rows(s, pl->scales.dev, (int)pl->scales.kept.size(), rows, factors));
  h->dp_rows = rows;
  pl->cond = cond; pl->gather = gather;
  // a replay reads `cond` again: only while it is the workspace's own copy (a batch source, condition dropout), never a caller's tensor
  h->dp_replay_ok = cond >= h->train_arena && cond < h->train_arena + h->train_arena.cap();
  return OSD_OK;
}

void dp_free(osd_handle* h) {
  delete static_cast<DpPlan*>(h->dp_plan);
  h->dp_plan = nullptr;
}

}  // namespace osd

using namespace osd;

extern "C" {

int osd_set_dp_clip(osd_handle* h, double max_grad_norm) {
  if (!h) { set_error("null handle"); return OSD_EINVAL; }
  if (!(max_grad_norm >= 0.0) || !std::isfinite(max_grad_norm)) { set_error("max_grad_norm must be finite and >= 0 (0 switches the per-row clip off), got %g", max_grad_norm); return OSD_EINVAL; }
  h->dp_clip = max_grad_norm;
  return OSD_OK;
}

int osd_dp_row_norms(osd_handle* h, float* dst_dev, int64_t n) {
  if (!h || !dst_dev) { set_error("null argument"); return OSD_EINVAL; }
  if (h->dp_rows < 0) { set_error("no training call with a per-row clip (osd_set_dp_clip) has run on this handle"); return OSD_ESTATE; }
  if (n != h->dp_rows) { set_error("the last clipped training call had %lld rows, not %lld", (long long)h->dp_rows, (long long)n); return OSD_EINVAL; }
  OSD_HIP(hipSetDevice(h->cfg.device));
  OSD_HIP(hipMemcpyAsync(dst_dev, h->dp_norms, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
  return OSD_OK;
}

// Measurement aid (tools/dp_bench.py): one of the last clipped call's two launches again, on the buffers that call left
int osd_dp_replay(osd_handle* h, int which, float fill) {
  if (!h) { set_error("null handle"); return OSD_EINVAL; }
  DpPlan* pl = static_cast<DpPlan*>(h->dp_plan);
  if (h->dp_rows < 0 || !pl) { set_error("no training call with a per-row clip (osd_set_dp_clip) has run on this handle"); return OSD_ESTATE; }
  if (!h->dp_replay_ok) {
    set_error("the workspace no longer holds the last clipped call (another call carved it since), or that call read the caller's own condition tensor");
    return OSD_ESTATE;
  }
  OSD_HIP(hipSetDevice(h->cfg.device));
  float* factors = h->dp_norms + h->dp_norms.cap() / 2;
  if (which == 0) {
    OSD_HIP(launch_dp_row_norms(h->stream, pl->norms.dev, (int)pl->norms.kept.size(), h->dp_rows, (float)h->dp_rows, (float)h->dp_clip, h->dp_norms, factors, pl->cond, pl->gather));
  } else if (which == 1) {
    OSD_HIP(launch_dp_scale_rows(h->stream, pl->scales.dev, (int)pl->scales.kept.size(), h->dp_rows, factors));
  } else if (which == 2) {          // every clip factor = fill
    unsigned bits;
    memcpy(&bits, &fill, sizeof(bits));
    OSD_HIP(hipMemsetD32Async((hipDeviceptr_t)factors, (int)bits, (size_t)h->dp_rows, h->stream));
  } else {
    set_error("which must be 0 (row norms), 1 (clip rows) or 2 (fill the clip factors)");
    return OSD_EINVAL;
  }
  return OSD_OK;
}

}  // extern "C"
