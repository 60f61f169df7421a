// dp.h -- differentially private training (DP-SGD, Abadi et al. 2016): per-row gradient norms from the buffers a backward pass leaves in
// the training workspace, the per-row clip factor applied to those buffers, and Gaussian noise inside the fused AdamW step.  DESIGN.md 3.21.
//
// Every layer is a Linear on 2-D activations or a per-row GroupNorm, so the gradient of row r's loss with respect to a Linear's weight is
// the outer product delta_r x_r^T (squared norm |x_r|^2 |delta_r|^2), to its bias delta_r, and to a GroupNorm's affine (gy_r * zhat_r,
// gy_r).  The squared norm of a row's whole gradient is the sum of those terms over the layers: no per-sample gradient is materialised.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <vector>

struct osd_handle;

namespace osd {

constexpr uint32_t TAG_DP_NOISE = 0x44504e00u;      // rng.h: distinct from every TAG_* there ("DPN")
constexpr int DP_NOISE_COLS = 4096;                 // the flat buffer read as rows of 4 096 elements: element i is (i / 4096, i % 4096)

// One term of a row's squared gradient norm.
//   kind 0, Linear(s) sharing one output gradient: (sum_j |x_j[r]|^2 + nbias) * |d[r]|^2; source 2 may be gathered (row gather[r] of x[2])
//   kind 1, GroupNorm affine: sum_c (gy[r][c] * zhat[r][c])^2 + gy[r][c]^2, zhat from z and stats [rows][C / gw][2] as k_gn_colsums does
// Pointers that are the caller's and may change from call to call (the batch's conditions, its timesteps) are NOT in the list: an item
// flags them (x0_is_cond, gathered) and the launch takes them as arguments, so that the cached device list stays valid step after step.
struct DpNormItem {
  int kind;
  const float* x[3]; int ldx[3]; int k[3];
  int x0_is_cond;                       // x[0] is the launch's `cond` argument (row stride ldx[0])
  int gathered;                         // row r of x[2] is row gather[r], gather = the launch's argument
  float nbias;
  const float* d; int ldd; int nd;      // kind 1: d = gy, nd = C, ldd = C
  const float* z; const float* stats; int gw;
};
// One buffer whose rows take the clip factor in place
struct DpScaleItem { float* p; int ld; int cols; };

// s[r] = unscale * sqrt(sum of the items' terms), c[r] = min(1, clip / (s[r] + 1e-6)): one wave per row over all items, no atomics
hipError_t launch_dp_row_norms(hipStream_t s, const DpNormItem* d_items, int n_items, int64_t rows, float unscale, float clip, float* norms, float* factors,
                               const float* cond, const int* gather);
// p[r][:] *= c[r] for every listed buffer (rows with c[r] == 1 are left alone): one wave per row over all items
hipError_t launch_dp_scale_rows(hipStream_t s, const DpScaleItem* d_items, int n_items, int64_t rows, const float* factors);

// the two lists of a step on the device (cached: uploaded only when a workspace pointer or a shape changed), then both launches; leaves s_r and c_r
// in h->dp_norms [2][rows]
int dp_clip_rows(osd_handle* h, hipStream_t s, const std::vector<DpNormItem>& norms, const std::vector<DpScaleItem>& scales, int64_t rows, double unscale,
                 const float* cond, const int* gather);
void dp_free(osd_handle* h);

}  // namespace osd
