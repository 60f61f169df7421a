// glm.hip -- loss, gradient and scores of up to four regularised linear heads over a device-resident cohort, in ONE read of the
// cohort:
//   osd_val_glm_eval              z_ik = W_k[:D] . u_i + W_k[D], u = (x - center) * scale; sum_i a_i l_k(y_ik, z_ik) and its gradient
//   osd_val_col_centered_moments  per-column sum (x - c) and sum (x - c)^2 in double: what the standardisation is made from
//
// A workgroup owns ALL columns of a group of R rows: a lane keeps 4 NV of them per row in registers from the dot product to the
// gradient, so X is fetched once.  Per group:
//   1. d = x - c in place, partial dots against w' = w * scale (so u is never formed: z = sum w' d, and the gradient's factor
//      scale is applied once, in double, by the reducer);
//   2. wave butterfly, one partial per wave and (row, head) through a few hundred bytes of LDS, barrier;
//   3. lanes 0 .. R K - 1 of wave 0 add the waves' partials in wave order, apply the link function, write the score, add the fp32
//      row loss and the bias gradient to their double sums and publish the residual a_i dl/dz, barrier;
//   4. every lane: g[k][col] += residual[r][k] * d[r][col] in fp32.
// The next group's rows are loaded into a second register set before step 1, so loads stay in flight across both barriers.
// An item (one workgroup) is a contiguous run of rows; after at most OSD_GLM_RUN_ROWS rows its fp32 sums are folded into its own
// double slab in global memory (nobody else touches it: plain loads and stores).  glm_reduce adds the items' slabs in a fixed
// order: no floating-point atomics, same inputs, same bits.  The partition into items depends on (rows, D, K) and the load path
// only, never on the device, and the predictor (no gradient) runs the same code without steps 4 and the slab: its scores are the full call's bits.
//
// ALIGNED (base 16-byte aligned, ld % 4 == 0, ld >= roundup(D, 4)): a lane owns column quads tid + T j and loads them as 16 bytes;
// columns D .. roundup(D, 4) - 1 are a neighbour's or padding: their w' is 0 and their sums are never stored.  Otherwise (NARROW)
// a lane owns columns tid + T m and loads dwords, each checked against D: coalesced, in place, no padded copy.
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <mutex>
#include <vector>
#include "handle.h"
#include "val_common.h"

namespace osd {
namespace {

constexpr int GLM_MAX_K = 4;
constexpr int GLM_MAX_D = 8192;
constexpr int GLM_MAX_ITEMS = 768;       // workgroups of a call: three per CU for rows up to 2048 columns wide, three rounds beyond
constexpr int GLM_MIN_ITEM_ROWS = 16;    // an item writes K (D + 1) doubles: not for fewer rows than this
constexpr int GLM_MAX_WAVES = 16;
constexpr int GLM_RED_PARTS = 16;

// Workgroup size classes: up to 256 lanes with 168 registers each (three workgroups per CU), or up to 512 lanes with 256 (one).
__host__ __device__ constexpr int glm_reg_budget(int TMAX) { return TMAX == 256 ? 168 : 256; }
__host__ __device__ constexpr int glm_min_waves(int TMAX) { return TMAX == 256 ? 3 : 2; }
// Registers of a lane with R rows per group: two register sets of R x NV x 4 values beside 4 NV (1 + 2 K) column constants and
// sums, and addresses, partial dots, residuals and temporaries (60 + 10 K, and 24 + 10 K more on the dword path: read off the
// compiler's resource report, on the safe side).
__host__ __device__ constexpr int glm_regs(int K, int NV, bool aligned, int R) {
  return 2 * R * NV * 4 + 4 * NV * (1 + 2 * K) + 60 + 10 * K + (aligned ? 0 : 24 + 10 * K);
}
__host__ __device__ constexpr int glm_group_rows(int K, int NV, int TMAX, bool aligned) {
  return glm_regs(K, NV, aligned, 4) <= glm_reg_budget(TMAX) ? 4 : glm_regs(K, NV, aligned, 2) <= glm_reg_budget(TMAX) ? 2 : 1;
}

struct GlmArgs {
  const float* X; const float* center; const float* scale; const float* Y; const float* a; const float* W;
  double* slab;            // [items][K][Dl]: columns 0 .. D - 1, the bias at D
  double* loss_slab;       // [items][K]
  float* score;
  long long ld, ldy, lds, rows, rows_per;    // rows_per: rows of an item, a multiple of the group
  int D, Dl;
  int kind[GLM_MAX_K];
};

template <int K, int NV, int TMAX, bool ALIGNED>
__global__ __launch_bounds__(TMAX, glm_min_waves(TMAX)) void glm_kernel(GlmArgs a) {
  constexpr int R = glm_group_rows(K, NV, TMAX, ALIGNED);
  const bool GRAD = a.slab != nullptr;                       // the predictor runs the same code without the column sums
  constexpr int RK = R * K;
  static_assert(OSD_GLM_RUN_ROWS % R == 0, "a run is a whole number of groups");
  __shared__ float part[2][GLM_MAX_WAVES][RK];
  __shared__ float resid[2][RK];
  __shared__ double fin[2][RK];

  const int tid = threadIdx.x, T = blockDim.x;
  const int lane = tid & 63, wave = tid >> 6, nw = T >> 6;
  const long long item = blockIdx.x;
  const long long r0 = item * a.rows_per;
  const long long r1 = min(a.rows, r0 + a.rows_per);         // r0 < r1: the host launches no empty item
  const int D = a.D;

  auto col_of = [&](int j, int e) { return ALIGNED ? 4 * (tid + T * j) + e : tid + T * (4 * j + e); };

  float c[NV][4], w[K][NV][4], g[K][NV][4];
#pragma unroll
  for (int j = 0; j < NV; ++j)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int col = col_of(j, e);
      const bool in = col < D;
      c[j][e] = in ? a.center[col] : 0.f;
      const float sc = in ? a.scale[col] : 0.f;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        w[k][j][e] = in ? a.W[(size_t)k * (D + 1) + col] * sc : 0.f;
        g[k][j][e] = 0.f;
      }
    }
  // lanes 0 .. RK - 1 of wave 0 each own one (row of the group, head)
  const int my_r = tid / K, my_k = tid - my_r * K;
  const bool owner = tid < RK;
  const float bias = owner ? a.W[(size_t)my_k * (D + 1) + D] : 0.f;
  const int kind = my_k == 0 ? a.kind[0] : my_k == 1 ? a.kind[1] : my_k == 2 ? a.kind[2] : a.kind[3];
  double loss_acc = 0.0, bias_acc = 0.0;

  auto load = [&](float (&xb)[R][NV][4], float& yb, float& ab, long long gr) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const long long row = min(gr + r, r1 - 1);            // a row beyond the item re-reads its last row, with weight 0
      const float* p = a.X + (size_t)row * (size_t)a.ld;
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        if (ALIGNED) {
          const int q = 4 * (tid + T * j);
          float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
          if (q < D) v = *reinterpret_cast<const float4*>(p + q);
          xb[r][j][0] = v.x; xb[r][j][1] = v.y; xb[r][j][2] = v.z; xb[r][j][3] = v.w;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int col = col_of(j, e);
            xb[r][j][e] = col < D ? p[col] : 0.f;
          }
        }
      }
    }
    yb = 0.f; ab = 0.f;
    if (owner) {
      const long long row = gr + my_r;
      if (row < r1) {
        yb = a.Y ? a.Y[(size_t)row * (size_t)a.ldy + my_k] : 0.f;
        ab = a.a ? a.a[row] : 1.f;
      }
    }
  };

  auto process = [&](float (&xb)[R][NV][4], float yb, float ab, long long gr, int par) {
    float p[R][K];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int k = 0; k < K; ++k) p[r][k] = 0.f;
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int j = 0; j < NV; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float d = xb[r][j][e] - c[j][e];
          xb[r][j][e] = d;
#pragma unroll
          for (int k = 0; k < K; ++k) p[r][k] += w[k][j][e] * d;
        }
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int k = 0; k < K; ++k) {
        float v = p[r][k];
        wave_sum(v);
        if (lane == 0) part[par][wave][r * K + k] = v;
      }
    __syncthreads();
    if (owner) {
      float z = part[par][0][tid];
      for (int q = 1; q < nw; ++q) z += part[par][q][tid];
      z += bias;
      float f, l;
      if (kind == OSD_GLM_LOGISTIC) {
        const float t = expf(-fabsf(z));                     // in (0, 1]: nothing overflows for any finite z
        const float sg = z >= 0.f ? 1.f / (1.f + t) : t / (1.f + t);
        f = sg - yb;
        l = fmaxf(z, 0.f) - yb * z + log1pf(t);
      } else {
        f = z - yb;
        l = 0.5f * (f * f);
      }
      const long long row = gr + my_r;
      if (row < r1) {
        if (a.score) a.score[(size_t)row * (size_t)a.lds + my_k] = z;
        loss_acc += (double)(ab * l);
        bias_acc += (double)(ab * f);
      }
      if (GRAD) resid[par][tid] = ab * f;                    // 0 for a row beyond the item
    }
    if (GRAD) {
      __syncthreads();
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const float f = resid[par][r * K + k];
#pragma unroll
          for (int j = 0; j < NV; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) g[k][j][e] += f * xb[r][j][e];
        }
    }
  };

  // end of an fp32 run: into the item's own double slab (first run of the item: stored, later runs: added)
  int folds = 0;
  auto fold = [&]() {
    if (!GRAD) return;                                       // uniform
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
      for (int j = 0; j < NV; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int col = col_of(j, e);
          if (col < D) {
            double* s = a.slab + ((size_t)item * K + k) * (size_t)a.Dl + col;
            *s = (folds ? *s : 0.0) + (double)g[k][j][e];
          }
          g[k][j][e] = 0.f;
        }
    ++folds;
  };

  const long long n_rows = r1 - r0;
  const long long ngroups = (n_rows + R - 1) / R;
  long long done = 0;
  auto after = [&]() {
    done += R;
    if (done % OSD_GLM_RUN_ROWS == 0 || done >= n_rows) fold();
  };
  float x0[R][NV][4], x1[R][NV][4];
  float y0, a0, y1 = 0.f, a1 = 0.f;
  load(x0, y0, a0, r0);
  for (long long gi = 0; gi < ngroups; gi += 2) {            // every condition below is the same in the whole workgroup
    const bool second = gi + 1 < ngroups;
    if (second) load(x1, y1, a1, r0 + (gi + 1) * R);
    process(x0, y0, a0, r0 + gi * R, 0);
    after();
    if (second) {
      if (gi + 2 < ngroups) load(x0, y0, a0, r0 + (gi + 2) * R);
      process(x1, y1, a1, r0 + (gi + 1) * R, 1);
      after();
    }
  }

  // the item's loss and bias gradient: rows of the group added in row order
  if (owner) { fin[0][tid] = loss_acc; fin[1][tid] = bias_acc; }
  __syncthreads();
  if (tid < K) {
    double ls = 0.0, bs = 0.0;
    for (int r = 0; r < R; ++r) { ls += fin[0][r * K + tid]; bs += fin[1][r * K + tid]; }
    a.loss_slab[(size_t)item * K + tid] = ls;
    if (GRAD) a.slab[((size_t)item * K + tid) * (size_t)a.Dl + D] = bs;
  }
}

// grad[k][col] = scale[col] * sum over the items, col < D; the bias (col == D) as it is.  64 columns x 16 parts per workgroup:
// part p adds items p, p + 16, ... in that order, then the parts are added in part order.
__global__ __launch_bounds__(64 * GLM_RED_PARTS) void glm_reduce(const double* __restrict__ slab, int items, int K, int D, int Dl,
                                                                 const float* __restrict__ scale, double* __restrict__ grad) {
  __shared__ double part[GLM_RED_PARTS][64];
  const int cx = threadIdx.x & 63, p = threadIdx.x >> 6;
  const int k = blockIdx.y, col = blockIdx.x * 64 + cx;
  double s = 0.0;
  if (col <= D)
    for (int it = p; it < items; it += GLM_RED_PARTS) s += slab[((size_t)it * K + k) * (size_t)Dl + col];
  part[p][cx] = s;
  __syncthreads();
  if (p == 0 && col <= D) {
    double t = part[0][cx];
    for (int q = 1; q < GLM_RED_PARTS; ++q) t += part[q][cx];
    if (col < D) {
      const float sc = scale[col];
      t = sc == 0.f ? 0.0 : t * (double)sc;                  // a dropped column: exactly zero
    }
    grad[(size_t)k * (D + 1) + col] = t;
  }
}

// ---- column moments -------------------------------------------------------------------------------------------------------------
constexpr int MOM_MAX_SLICES = 256;

// slab[slice][0][col] = sum (x - c), slab[slice][1][col] = sum (x - c)^2 over the slice's rows, in double; a lane per column
__global__ __launch_bounds__(256) void col_moments_kernel(const float* __restrict__ X, long long ld, long long rows, int D,
                                                          const float* __restrict__ center, long long rows_per,
                                                          double* __restrict__ slab) {
  const int col = blockIdx.x * 256 + threadIdx.x;
  if (col >= D) return;
  const long long r0 = (long long)blockIdx.y * rows_per, r1 = min(rows, r0 + rows_per);
  const double c = center ? (double)center[col] : 0.0;
  double s = 0.0, q = 0.0;
  long long r = r0;
  for (; r + 4 <= r1; r += 4) {
    float v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = X[(size_t)(r + i) * (size_t)ld + col];
#pragma unroll
    for (int i = 0; i < 4; ++i) { const double d = (double)v[i] - c; s += d; q += d * d; }
  }
  for (; r < r1; ++r) { const double d = (double)X[(size_t)r * (size_t)ld + col] - c; s += d; q += d * d; }
  slab[((size_t)blockIdx.y * 2 + 0) * D + col] = s;
  slab[((size_t)blockIdx.y * 2 + 1) * D + col] = q;
}

__global__ void col_moments_reduce(const double* __restrict__ slab, int slices, int D, double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;       // over [2][D]
  if (i >= 2 * D) return;
  const int which = i / D, col = i - which * D;
  double s = 0.0;
  for (int sl = 0; sl < slices; ++sl) s += slab[((size_t)sl * 2 + which) * D + col];
  out[i] = s;
}

// One grow-only workspace per device, held for the length of a call: a fit calls osd_val_glm_eval hundreds of times.
struct Workspace {
  std::mutex mu;
  DevBuf<char> buf;
};
constexpr int GLM_MAX_DEVICES = 64;
Workspace* const g_ws = new Workspace[GLM_MAX_DEVICES];      // never destroyed: no hipFree from a static destructor at process exit

template <int K, int NV, int TMAX>
int glm_launch2(bool aligned, bool dry, unsigned items, unsigned T, hipStream_t s, const GlmArgs& a) {
  if (dry) return glm_group_rows(K, NV, TMAX, aligned);      // the rows of a group: what the partition is made from
  // not dry: the launch's hipError_t
  return (int)launched(aligned ? glm_kernel<K, NV, TMAX, true> : glm_kernel<K, NV, TMAX, false>, dim3(items), dim3(T), 0, s, a);
}

template <int K>
int glm_launch(int NV, bool aligned, bool dry, unsigned items, unsigned T, hipStream_t s, const GlmArgs& a) {
  switch (NV) {
    case 1: return glm_launch2<K, 1, 256>(aligned, dry, items, T, s, a);
    case 2:                                                  // the small class only where two rows per group fit its registers
      return T <= 256 && glm_regs(K, 2, aligned, 2) <= glm_reg_budget(256) ? glm_launch2<K, 2, 256>(aligned, dry, items, T, s, a)
                                                                           : glm_launch2<K, 2, 512>(aligned, dry, items, T, s, a);
    case 3: return glm_launch2<K, 3, 512>(aligned, dry, items, T, s, a);
    default: return glm_launch2<K, 4, 512>(aligned, dry, items, T, s, a);
  }
}

int glm_dispatch(int K, int NV, bool aligned, bool dry, unsigned items, unsigned T, hipStream_t s, const GlmArgs& a) {
  switch (K) {
    case 1: return glm_launch<1>(NV, aligned, dry, items, T, s, a);
    case 2: return glm_launch<2>(NV, aligned, dry, items, T, s, a);
    case 3: return glm_launch<3>(NV, aligned, dry, items, T, s, a);
    default: return glm_launch<4>(NV, aligned, dry, items, T, s, a);
  }
}

}  // namespace
}  // namespace osd

using namespace osd;

extern "C" {

int osd_val_glm_eval(void* stream, int device, const float* X, int64_t rows, int ld, int D, const float* center, const float* scale,
                     const float* Y, int ldy, const float* row_weight, const float* W, int K, const int32_t* kind_host,
                     double* loss_host, double* grad_dev, float* score_dev, int lds) {
  if (!X || !center || !scale || !W || !kind_host || K < 1 || K > GLM_MAX_K || rows < 1 || D < 1 || D > GLM_MAX_D || ld < D ||
      device < 0 || device >= GLM_MAX_DEVICES) {
    set_error("bad argument (1 <= K <= 4, rows >= 1, 1 <= D <= 8192, ld >= D)");
    return OSD_EINVAL;
  }
  if ((!Y && (loss_host || grad_dev)) || (Y && ldy < K) || (score_dev && lds < K) || (!grad_dev && !score_dev && !loss_host)) {
    set_error("bad argument (targets [rows][ldy >= K] for a loss or a gradient, scores [rows][lds >= K], at least one output)");
    return OSD_EINVAL;
  }
  for (int k = 0; k < K; ++k)
    if (kind_host[k] != OSD_GLM_LOGISTIC && kind_host[k] != OSD_GLM_SQUARED) {
      set_error("head %d: unknown kind %d", k, (int)kind_host[k]);
      return OSD_EINVAL;
    }
  OSD_HIP(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;

  const int Dq = (D + 3) / 4 * 4, quads = Dq / 4;
  const int NV = quads <= 256 ? 1 : quads <= 1024 ? 2 : quads <= 1536 ? 3 : 4;
  const unsigned T = (unsigned)(((quads + NV - 1) / NV + 63) / 64 * 64);       // 64 .. 512 lanes, 4 NV T >= Dq columns
  const bool aligned = (reinterpret_cast<uintptr_t>(X) & 15) == 0 && ld % 4 == 0 && ld >= Dq;
  GlmArgs a{};
  const int R = glm_dispatch(K, NV, aligned, true, 0, T, s, a);
  // the partition: a function of (rows, D, K) and of which of the two load paths X takes
  const int64_t groups = (rows + R - 1) / R;
  int64_t want = (rows + GLM_MIN_ITEM_ROWS - 1) / GLM_MIN_ITEM_ROWS;
  if (want > GLM_MAX_ITEMS) want = GLM_MAX_ITEMS;
  const int64_t gpi = (groups + want - 1) / want;
  const unsigned items = (unsigned)((groups + gpi - 1) / gpi);

  a.X = X; a.center = center; a.scale = scale; a.Y = Y; a.a = row_weight; a.W = W; a.score = score_dev;
  a.ld = ld; a.ldy = ldy; a.lds = lds; a.rows = rows; a.rows_per = gpi * R;
  a.D = D; a.Dl = (D + 1 + 3) / 4 * 4;
  for (int k = 0; k < K; ++k) a.kind[k] = kind_host[k];

  Workspace& ws = g_ws[device];
  std::lock_guard<std::mutex> hold(ws.mu);
  const size_t loss_bytes = (size_t)items * K * sizeof(double);
  const size_t slab_bytes = grad_dev ? (size_t)items * K * a.Dl * sizeof(double) : 0;
  OSD_TRY(ws.buf.reserve((int64_t)(loss_bytes + slab_bytes)));
  a.loss_slab = (double*)ws.buf.get();
  a.slab = grad_dev ? a.loss_slab + (size_t)items * K : nullptr;

  const bool grad = grad_dev != nullptr;
  OSD_HIP((hipError_t)glm_dispatch(K, NV, aligned, false, items, T, s, a));
  if (grad)
    OSD_HIP(launched(glm_reduce, dim3((unsigned)((D + 1 + 63) / 64), (unsigned)K), dim3(64 * GLM_RED_PARTS), 0, s, a.slab, (int)items, K, D,
                     a.Dl, scale, grad_dev));
  std::vector<double> part(loss_host ? (size_t)items * K : 0);
  if (loss_host) OSD_HIP(hipMemcpyAsync(part.data(), a.loss_slab, loss_bytes, hipMemcpyDeviceToHost, s));
  OSD_HIP(hipStreamSynchronize(s));
  if (loss_host)
    for (int k = 0; k < K; ++k) {
      double t = 0.0;
      for (unsigned it = 0; it < items; ++it) t += part[(size_t)it * K + k];
      loss_host[k] = t;
    }
  return OSD_OK;
}

int osd_val_col_centered_moments(void* stream, int device, const float* X, int64_t rows, int ld, int D, const float* center,
                                 double* sum_host, double* sumsq_host) {
  if (!X || !sum_host || !sumsq_host || rows < 1 || D < 1 || D > 65535 * 256 || ld < D || device < 0 || device >= GLM_MAX_DEVICES) {
    set_error("bad argument (rows >= 1, D >= 1, ld >= D)");
    return OSD_EINVAL;
  }
  OSD_HIP(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  int64_t slices = (rows + 63) / 64;
  if (slices > MOM_MAX_SLICES) slices = MOM_MAX_SLICES;
  const int64_t rows_per = (rows + slices - 1) / slices;
  slices = (rows + rows_per - 1) / rows_per;
  Workspace& ws = g_ws[device];
  std::lock_guard<std::mutex> hold(ws.mu);
  OSD_TRY(ws.buf.reserve((int64_t)(((size_t)slices * 2 * D + (size_t)2 * D) * sizeof(double))));
  double* slab = (double*)ws.buf.get();
  double* out = slab + (size_t)slices * 2 * D;
  OSD_HIP(launched(col_moments_kernel, dim3((unsigned)((D + 255) / 256), (unsigned)slices), dim3(256), 0, s, X, (long long)ld,
                   (long long)rows, D, center, (long long)rows_per, slab));
  OSD_HIP(launched(col_moments_reduce, dim3((unsigned)((2 * D + 255) / 256)), dim3(256), 0, s, slab, (int)slices, D, out));
  std::vector<double> h((size_t)2 * D);
  OSD_HIP(read_back(s, h.data(), out, h.size() * sizeof(double)));
  for (int i = 0; i < D; ++i) { sum_host[i] = h[i]; sumsq_host[i] = h[(size_t)D + i]; }
  return OSD_OK;
}

}  // extern "C"
