// k_elem.hip -- HBM-bound elementwise kernels: Philox fills, q_sample, mixup, copies.
#include "kernels.h"

namespace osd {

__global__ void k_set_int(int* p, int v) { *p = v; }
__global__ void k_add_int(int* p, int d) { *p += d; }
hipError_t launch_set_int(hipStream_t s, int* p, int v) { hipLaunchKernelGGL(k_set_int, 1, 1, 0, s, p, v); return hipGetLastError(); }
hipError_t launch_add_int(hipStream_t s, int* p, int d) { hipLaunchKernelGGL(k_add_int, 1, 1, 0, s, p, d); return hipGetLastError(); }

// dst[r][:] = src[idx[r]][:], one workgroup per row (the caller keeps idx inside src's rows)
__global__ void k_gather_rows(const float* src, int cols, const int* idx, float* dst) {
  const float* s = src + (size_t)idx[blockIdx.x] * cols;
  float* d = dst + (size_t)blockIdx.x * cols;
  for (int c = threadIdx.x; c < cols; c += blockDim.x) d[c] = s[c];
}
hipError_t launch_gather_rows(hipStream_t s, const float* src, int cols, const int* idx, int rows, float* dst) {
  if (rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_gather_rows, rows, 256, 0, s, src, cols, idx, dst);
  return hipGetLastError();
}

static inline int ew_grid(int64_t work) {
  int64_t b = (work + 255) / 256;
  if (b > 8192) b = 8192;
  if (b < 1) b = 1;
  return (int)b;
}

// one thread per (row, 4 columns)
__global__ void k_fill_randn(float* out, int ld, int64_t rows, int cols, uint64_t seed, uint32_t row_offset, uint32_t step, uint32_t tag) {
  const int c4n = (cols + 3) >> 2;
  const int64_t total = rows * c4n;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / c4n;
    const int c4 = (int)(i - r * c4n);
    const float4 n = randn4(seed, row_offset + (uint32_t)r, (uint32_t)c4, step, tag);
    st4g(out + r * ld, 4 * c4, cols, n);
  }
}
hipError_t launch_fill_randn(hipStream_t s, float* out, int ld, int64_t rows, int cols, uint64_t seed, uint32_t row_offset, uint32_t step, uint32_t tag) {
  if (rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_fill_randn, ew_grid(rows * ((cols + 3) / 4)), 256, 0, s, out, ld, rows, cols, seed, row_offset, step, tag);
  return hipGetLastError();
}

__global__ void k_copy2d(const float* src, int lds, float* dst, int ldd, int64_t rows, int cols) {
  const int c4n = (cols + 3) >> 2;
  const int64_t total = rows * c4n;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / c4n;
    const int c = 4 * (int)(i - r * c4n);
    st4g(dst + r * ldd, c, cols, ld4g(src + r * lds, c, cols));
  }
}
hipError_t launch_copy2d(hipStream_t s, const float* src, int lds, float* dst, int ldd, int64_t rows, int cols) {
  if (rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_copy2d, ew_grid(rows * ((cols + 3) / 4)), 256, 0, s, src, lds, dst, ldd, rows, cols);
  return hipGetLastError();
}

// q_sample (models/diffusion.py:337-340): x_t = sqrt_ac[t]*x0 + sqrt_1m[t]*eps, two roundings of the
// products then one add, as torch evaluates it.
// t == null: the row's timestep is drawn here -- torch.randint(0, T, (B,)) stand-in of models/diffusion.py:361, the same Philox
// word k_randint uses -- and written to t_out by the row's first thread.
// x_t rows have a stride of ldxt >= cols floats; the pad columns [cols, ldxt) are written as zeros (the training forward's
// input_proj reads them against clamped weights, gemm.h: a_kmax).  zl: buffers of the training call that must be zero before
// anything accumulates into them -- zeroed here, by the same grid, instead of by a launch of their own.
// Only the first ZERO_BLOCKS workgroups walk the list: every entry costs a wave two dependent scalar loads from the argument block
// (~40 entries: 10-15 us of latency in front of the wave's real work when all 4096 workgroups did it -- measured).
constexpr int ZERO_BLOCKS = 32;
__device__ __forceinline__ void zero_list(const ZeroList& zl) {
  if (blockIdx.x >= ZERO_BLOCKS) return;
  const int nb = gridDim.x < ZERO_BLOCKS ? gridDim.x : ZERO_BLOCKS;
  for (int e = 0; e < zl.n; ++e) {
    float* p = zl.ptr[e];
    const int64_t n = zl.count[e];
    for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < n; j += (int64_t)nb * blockDim.x) p[j] = 0.f;
  }
}
__device__ __forceinline__ void zero_pad(float* row, int cols, int ldxt, int c) {
  if (c + 4 >= cols)
    for (int k = cols; k < ldxt; ++k) row[k] = 0.f;
}

// The training target (osd_set_prediction) in the pass that has eps and x0 in registers: KIND OSD_PRED_EPSILON leaves eps (today's
// kernel), OSD_PRED_V forms v = a*eps - b*x0 as torch would in fp32 -- two separately rounded products, one subtraction --,
// OSD_PRED_SAMPLE is x0 itself.  The non-eps kinds store the target where eps went (noise_out), injected noise or not.
template <int KIND>
__device__ __forceinline__ float4 q_target(float a, float b, const float4& x, const float4& n) {
  if constexpr (KIND == OSD_PRED_V) {
    float4 v;
    v.x = __fsub_rn(__fmul_rn(a, n.x), __fmul_rn(b, x.x));
    v.y = __fsub_rn(__fmul_rn(a, n.y), __fmul_rn(b, x.y));
    v.z = __fsub_rn(__fmul_rn(a, n.z), __fmul_rn(b, x.z));
    v.w = __fsub_rn(__fmul_rn(a, n.w), __fmul_rn(b, x.w));
    return v;
  } else if constexpr (KIND == OSD_PRED_SAMPLE) {
    return x;
  } else {
    return n;
  }
}

// Training on incomplete rows (osd_set_loss_mask): a NaN element of x0 is "not observed".  MASKED kernels
// test x != x per element (after the mixup: a mixed element is observed iff both parents are), take 0 in its place for x_t and for
// the target, and store the target with NaN at the unobserved elements -- the NaN in the target buffer is the mask the loss epilogue
// reads (epilogues.h: EpiLossT<true>), no mask tensor exists.  With no NaN in x0 the stored bits are the unmasked kernel's.
__device__ __forceinline__ float4 mask_fill(const float4& x) {
  return make_float4(x.x != x.x ? 0.f : x.x, x.y != x.y ? 0.f : x.y, x.z != x.z ? 0.f : x.z, x.w != x.w ? 0.f : x.w);
}
__device__ __forceinline__ float4 mask_mark(const float4& x, const float4& v) {
  const float qn = __builtin_nanf("");
  return make_float4(x.x != x.x ? qn : v.x, x.y != x.y ? qn : v.y, x.z != x.z ? qn : v.z, x.w != x.w ? qn : v.w);
}

template <int KIND, bool MASKED>
__global__ void k_q_sample(const float* x0, const int* t, const float* sqrt_ac, const float* sqrt_1m, const float* noise_in,
                           int64_t rows, int cols, uint64_t seed, uint32_t row_offset, float* x_t, int ldxt, float* noise_out, int* t_out, int T,
                           ZeroList zl) {
  zero_list(zl);
  const int c4n = (cols + 3) >> 2;
  const int64_t total = rows * c4n;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / c4n;
    const int c = 4 * (int)(i - r * c4n);
    int tt;
    if (t) tt = t[r];
    else {
      const uint4 rr = philox_at(seed, row_offset + (uint32_t)r, 0u, 0u, TAG_TSTEP);
      tt = (int)(((uint64_t)rr.x * (uint64_t)T) >> 32);
      if (c == 0) t_out[r] = tt;
    }
    const float a = sqrt_ac[tt], b = sqrt_1m[tt];
    const float4 xr = ld4g(x0 + r * cols, c, cols);
    float4 x = xr;
    if constexpr (MASKED) x = mask_fill(xr);
    float4 n;
    if (noise_in) n = ld4g(noise_in + r * cols, c, cols);
    else n = randn4(seed, row_offset + (uint32_t)r, (uint32_t)(c >> 2), 0u, TAG_QNOISE);
    float4 o;
    o.x = __fadd_rn(__fmul_rn(a, x.x), __fmul_rn(b, n.x));
    o.y = __fadd_rn(__fmul_rn(a, x.y), __fmul_rn(b, n.y));
    o.z = __fadd_rn(__fmul_rn(a, x.z), __fmul_rn(b, n.z));
    o.w = __fadd_rn(__fmul_rn(a, x.w), __fmul_rn(b, n.w));
    st4g(x_t + r * ldxt, c, cols, o);
    zero_pad(x_t + r * ldxt, cols, ldxt, c);
    if constexpr (MASKED) {
      if (noise_out) st4g(noise_out + r * cols, c, cols, mask_mark(xr, q_target<KIND>(a, b, x, n)));
    } else if constexpr (KIND == OSD_PRED_EPSILON) {
      if (noise_out && noise_out != noise_in) st4g(noise_out + r * cols, c, cols, n);
    } else {
      if (noise_out) st4g(noise_out + r * cols, c, cols, q_target<KIND>(a, b, x, n));
    }
  }
}
template <bool MASKED>
static auto pick_q_sample(int kind) {
  return kind == OSD_PRED_V ? k_q_sample<OSD_PRED_V, MASKED> : kind == OSD_PRED_SAMPLE ? k_q_sample<OSD_PRED_SAMPLE, MASKED> : k_q_sample<OSD_PRED_EPSILON, MASKED>;
}
hipError_t launch_q_sample(hipStream_t s, const float* x0, const int* t, const float* sqrt_ac, const float* sqrt_1m,
                           const float* noise_in, int64_t rows, int cols, uint64_t seed, uint32_t row_offset,
                           float* x_t, float* noise_out, int* t_out, int T, int ldxt, const ZeroList* zl, int kind, bool masked) {
  if (rows <= 0) return hipSuccess;
  if (!t && (!t_out || T < 1)) return hipErrorInvalidValue;
  // the target needs a buffer of its own; under the mask (its NaN marks) for every kind
  if ((kind != OSD_PRED_EPSILON || masked) && (noise_out == noise_in || noise_out == x0)) return hipErrorInvalidValue;
  ZeroList z{};
  if (zl) z = *zl;
  auto k = masked ? pick_q_sample<true>(kind) : pick_q_sample<false>(kind);
  hipLaunchKernelGGL(k, ew_grid(rows * ((cols + 3) / 4)), 256, 0, s, x0, t, sqrt_ac, sqrt_1m, noise_in, rows, cols, seed,
                     row_offset, x_t, ldxt > 0 ? ldxt : cols, noise_out, t_out, T, z);
  return hipGetLastError();
}

// The training step's prologue in one pass (SURVEY a5 + a11): batch row r is taken from a device-resident dataset -- row idx_a[r],
// mixed with row idx_b[r] as MixupAugmentation does (utils/train.py:117-119: lam * v + (1 - lam) * v[perm], products rounded
// separately, so the result has the bits of the reference's two-step evaluation) -- and goes straight through q_sample; the mixed
// row itself is only written when somebody needs it (x0_out: the constraint losses).  The row's first thread also mixes the
// condition row into cond_out.  Replaces gather + k_mixup3 + k_q_sample (three passes over the batch) by one.
// One workgroup = QS_ROWS batch rows; a thread walks the row's 16-byte quads t, t + 256, ... (no 64-bit division per element, the
// row's scalars -- t, the two schedule values, the two dataset rows -- are wave-uniform and loaded once), QS_ROWS x 2 independent
// quads per thread in flight at D = 2000.  First version (one quad per thread over a flat index): 37 us = 3.6 TB/s; row by row with
// the zero list folded in: 40 us; all QS_ROWS rows' loads ahead of the stores: 35.4 us = 3.8 TB/s (QS_ROWS 2: 35.9, 8: 46.8).
constexpr int QS_ROWS = 4;
template <int KIND, bool MASKED>
__global__ __launch_bounds__(256) void k_q_sample_src(BatchSrc b, const int* t, const float* sqrt_ac, const float* sqrt_1m, const float* noise_in,
                                                      int64_t rows, int cols, int cd, uint64_t seed, uint32_t row_offset, float* x_t, int ldxt,
                                                      float* noise_out, int* t_out, int T, float* cond_out, float* x0_out, ZeroList zl) {
  zero_list(zl);
  const int c4n = (cols + 3) >> 2;
  for (int64_t r0 = (int64_t)blockIdx.x * QS_ROWS; r0 < rows; r0 += (int64_t)gridDim.x * QS_ROWS) {
    // the rows' scalars first (wave-uniform loads), then per 256-quad column block ALL dataset loads of the QS_ROWS rows before any
    // store: the stores may alias the loads as far as hipcc knows, so a load placed behind a store waits for it -- one row at a time
    // the kernel ran at 3.4 TB/s with two loads in flight per thread
    float a[QS_ROWS], bb[QS_ROWS];
    const float* xa[QS_ROWS]; const float* xb[QS_ROWS];
    int nrow = 0;
#pragma unroll
    for (int rr = 0; rr < QS_ROWS; ++rr) {
      const int64_t r = r0 + rr;
      a[rr] = bb[rr] = 0.f; xa[rr] = xb[rr] = b.data;
      if (r >= rows) continue;                       // uniform over the workgroup
      nrow = rr + 1;
      int tt;
      if (t) tt = t[r];
      else {
        const uint4 rnd = philox_at(seed, row_offset + (uint32_t)r, 0u, 0u, TAG_TSTEP);
        tt = (int)(((uint64_t)rnd.x * (uint64_t)T) >> 32);
        if (threadIdx.x == 0) t_out[r] = tt;
      }
      a[rr] = sqrt_ac[tt]; bb[rr] = sqrt_1m[tt];
      const int64_t ia = b.idx_a ? b.idx_a[r] : r;
      const int64_t ib = b.idx_b ? b.idx_b[r] : 0;
      xa[rr] = b.data + ia * b.ldd;
      xb[rr] = b.data + ib * b.ldd;
      if ((int)threadIdx.x < cd && cond_out) {
        float v = b.cond[ia * b.ldc + threadIdx.x];
        if (b.idx_b) v = __fadd_rn(__fmul_rn(b.lam, v), __fmul_rn(b.oml, b.cond[ib * b.ldc + threadIdx.x]));
        cond_out[r * cd + threadIdx.x] = v;
      }
    }
    for (int q0 = 0; q0 < c4n; q0 += 256) {
      const int q = q0 + (int)threadIdx.x;
      if (q >= c4n) continue;
      const int c = 4 * q;
      float4 x[QS_ROWS], y[QS_ROWS], nz[QS_ROWS];
#pragma unroll
      for (int rr = 0; rr < QS_ROWS; ++rr) {
        if (rr >= nrow) break;
        x[rr] = ld4g(xa[rr], c, cols);
        if (b.idx_b) y[rr] = ld4g(xb[rr], c, cols);
        if (noise_in) nz[rr] = ld4g(noise_in + (r0 + rr) * cols, c, cols);
      }
#pragma unroll
      for (int rr = 0; rr < QS_ROWS; ++rr) {
        if (rr >= nrow) break;
        const int64_t r = r0 + rr;
        float4 xv = x[rr];
        if (b.idx_b) {
          xv.x = __fadd_rn(__fmul_rn(b.lam, xv.x), __fmul_rn(b.oml, y[rr].x));
          xv.y = __fadd_rn(__fmul_rn(b.lam, xv.y), __fmul_rn(b.oml, y[rr].y));
          xv.z = __fadd_rn(__fmul_rn(b.lam, xv.z), __fmul_rn(b.oml, y[rr].z));
          xv.w = __fadd_rn(__fmul_rn(b.lam, xv.w), __fmul_rn(b.oml, y[rr].w));
        }
        float4 xm;                                    // MASKED: the mixed row with its NaN, xv zero-filled
        if constexpr (MASKED) { xm = xv; xv = mask_fill(xm); }
        float4 n;
        if (noise_in) n = nz[rr];
        else n = randn4(seed, row_offset + (uint32_t)r, (uint32_t)q, 0u, TAG_QNOISE);
        float4 o;
        o.x = __fadd_rn(__fmul_rn(a[rr], xv.x), __fmul_rn(bb[rr], n.x));
        o.y = __fadd_rn(__fmul_rn(a[rr], xv.y), __fmul_rn(bb[rr], n.y));
        o.z = __fadd_rn(__fmul_rn(a[rr], xv.z), __fmul_rn(bb[rr], n.z));
        o.w = __fadd_rn(__fmul_rn(a[rr], xv.w), __fmul_rn(bb[rr], n.w));
        st4g(x_t + r * ldxt, c, cols, o);
        zero_pad(x_t + r * ldxt, cols, ldxt, c);
        if constexpr (MASKED) {
          if (noise_out) st4g(noise_out + r * cols, c, cols, mask_mark(xm, q_target<KIND>(a[rr], bb[rr], xv, n)));
        } else if constexpr (KIND == OSD_PRED_EPSILON) {
          if (noise_out && noise_out != noise_in) st4g(noise_out + r * cols, c, cols, n);
        } else {
          if (noise_out) st4g(noise_out + r * cols, c, cols, q_target<KIND>(a[rr], bb[rr], xv, n));
        }
        if (x0_out) st4g(x0_out + r * cols, c, cols, xv);
      }
    }
  }
}
template <bool MASKED>
static auto pick_q_sample_src(int kind) {
  return kind == OSD_PRED_V ? k_q_sample_src<OSD_PRED_V, MASKED> : kind == OSD_PRED_SAMPLE ? k_q_sample_src<OSD_PRED_SAMPLE, MASKED> : k_q_sample_src<OSD_PRED_EPSILON, MASKED>;
}
hipError_t launch_q_sample_src(hipStream_t s, const BatchSrc& b, const int* t, const float* sqrt_ac, const float* sqrt_1m, const float* noise_in,
                               int64_t rows, int cols, int cd, uint64_t seed, uint32_t row_offset, float* x_t, float* noise_out, int* t_out, int T,
                               float* cond_out, float* x0_out, int ldxt, const ZeroList* zl, int kind, bool masked) {
  if (rows <= 0) return hipSuccess;
  if (!t && (!t_out || T < 1)) return hipErrorInvalidValue;
  if ((kind != OSD_PRED_EPSILON || masked) && noise_out == noise_in) return hipErrorInvalidValue;
  ZeroList z{};
  if (zl) z = *zl;
  if (cd > 256) return hipErrorInvalidValue;
  int64_t blocks = (rows + QS_ROWS - 1) / QS_ROWS;
  if (blocks > 4096) blocks = 4096;
  if (blocks < (zl ? 32 : 1)) blocks = zl ? 32 : 1;      // the zero list is walked by the first 32 workgroups
  auto k = masked ? pick_q_sample_src<true>(kind) : pick_q_sample_src<false>(kind);
  hipLaunchKernelGGL(k, dim3((unsigned)blocks), 256, 0, s, b, t, sqrt_ac, sqrt_1m, noise_in, rows, cols, cd, seed,
                     row_offset, x_t, ldxt > 0 ? ldxt : cols, noise_out, t_out, T, cond_out, x0_out, z);
  return hipGetLastError();
}

// q_sample for the likelihood bound: the rows of a launch are (timestep, patient) pairs of a [S][n_pat] grid,
// x0 and the condition row are gathered from the patient -- the cohort is never replicated S times -- and the generated normals of
// patient i at timestep t come from the Philox block (seed, row_offset + i, quad, t, TAG_QNOISE): t sits where k_q_sample passes 0, so
// a draw depends on (seed, global patient id, timestep) alone, not on how the pairs were cut into launches.  The arithmetic per
// element is k_q_sample's.  One workgroup walks whole rows (the row's scalars are wave-uniform); t_out / cond_out receive the row's
// timestep and condition for the layers that gather by row.
template <int KIND>
__global__ __launch_bounds__(256) void k_q_sample_pairs(const float* x0, const float* cond, int cd, PairRows pr, const float* sqrt_ac, const float* sqrt_1m,
                                                        const float* noise_in, int64_t rows, int cols, uint64_t seed, uint32_t row_offset, float* x_t,
                                                        int ldxt, float* target_out, int* t_out, float* cond_out, ZeroList zl) {
  zero_list(zl);
  const int c4n = (cols + 3) >> 2;
  for (int64_t r = blockIdx.x; r < rows; r += gridDim.x) {
    const int64_t pair = pr.pair0 + r;
    const int64_t i = pair % pr.n_pat;
    const int tt = pr.t_row ? pr.t_row[r] : pr.t_list[pair / pr.n_pat];
    const float a = sqrt_ac[tt], b = sqrt_1m[tt];
    if (threadIdx.x == 0) t_out[r] = tt;
    if (cond_out && (int)threadIdx.x < cd) cond_out[r * cd + threadIdx.x] = cond[i * cd + threadIdx.x];
    const float* xrow = x0 + i * cols;
    for (int q = threadIdx.x; q < c4n; q += 256) {
      const int c = 4 * q;
      const float4 x = ld4g(xrow, c, cols);
      float4 n;
      if (noise_in) n = ld4g(noise_in + r * cols, c, cols);
      else n = randn4(seed, row_offset + (uint32_t)i, (uint32_t)q, (uint32_t)tt, TAG_QNOISE);
      float4 o;
      o.x = __fadd_rn(__fmul_rn(a, x.x), __fmul_rn(b, n.x));
      o.y = __fadd_rn(__fmul_rn(a, x.y), __fmul_rn(b, n.y));
      o.z = __fadd_rn(__fmul_rn(a, x.z), __fmul_rn(b, n.z));
      o.w = __fadd_rn(__fmul_rn(a, x.w), __fmul_rn(b, n.w));
      st4g(x_t + r * ldxt, c, cols, o);
      zero_pad(x_t + r * ldxt, cols, ldxt, c);
      if (target_out) st4g(target_out + r * cols, c, cols, q_target<KIND>(a, b, x, n));
    }
  }
}
hipError_t launch_q_sample_pairs(hipStream_t s, const float* x0, const float* cond, int cd, const PairRows& pr, const float* sqrt_ac,
                                 const float* sqrt_1m, const float* noise_in, int64_t rows, int cols, uint64_t seed, uint32_t row_offset, float* x_t,
                                 int ldxt, float* target_out, int* t_out, float* cond_out, const ZeroList* zl, int kind) {
  if (rows <= 0) return hipSuccess;
  if (!t_out || pr.n_pat < 1 || (!pr.t_row && !pr.t_list) || cd > 256) return hipErrorInvalidValue;
  if (!target_out && !(kind == OSD_PRED_EPSILON && noise_in)) return hipErrorInvalidValue;      // only injected eps is its own target
  ZeroList z{};
  if (zl) z = *zl;
  int64_t blocks = rows < 16384 ? rows : 16384;
  if (blocks < (zl ? 32 : 1)) blocks = zl ? 32 : 1;      // the zero list is walked by the first 32 workgroups
  auto k = kind == OSD_PRED_V ? k_q_sample_pairs<OSD_PRED_V> : kind == OSD_PRED_SAMPLE ? k_q_sample_pairs<OSD_PRED_SAMPLE> : k_q_sample_pairs<OSD_PRED_EPSILON>;
  hipLaunchKernelGGL(k, dim3((unsigned)blocks), 256, 0, s, x0, cond, cd, pr, sqrt_ac, sqrt_1m, noise_in, rows, cols, seed, row_offset, x_t,
                     ldxt > 0 ? ldxt : cols, target_out, t_out, cond_out, z);
  return hipGetLastError();
}

// q_sample for the noise map: k_q_sample_pairs' rows, gather and draw address -- the normals of patient i at
// level s are the block (seed, row_offset + i, quad, tau_s, TAG_QNOISE) -- with two levels per row.  Row (s, i) forms y_s, the network's
// input, and, for s > 0, y_{s-1} from that level's OWN draw: recomputed from x0, never fetched from another row, so a launch group needs
// nothing of its neighbours.  What EpiNoiseMap streams in place of a training target is u = y_{s-1} - A_s y_s (one fma: the outermost
// operation of the chain's step fmaf(A, y, fmaf(B, out, C z)) taken back first); its per-row record (B_s, 1 / C_s, the offset of
// noises_out [n_steps-1-s][i]) rides along.  Rows of the last level also write y_s to x_start.  Each product-sum is k_q_sample's.
__global__ __launch_bounds__(256) void k_q_sample_map(const float* x0, const float* cond, int cd, MapRows mr, const float* sqrt_ac, const float* sqrt_1m,
                                                      const float* noise_in, int64_t rows, int cols, uint64_t seed, uint32_t row_offset, float* x_t,
                                                      int ldxt, float* target_out, MapRow* row_out, float* x_start, int* t_out, float* cond_out,
                                                      ZeroList zl) {
  zero_list(zl);
  const int c4n = (cols + 3) >> 2;
  for (int64_t r = blockIdx.x; r < rows; r += gridDim.x) {
    const int64_t pair = mr.pair0 + r;
    const int64_t i = pair % mr.n_pat;
    const int s = mr.s0 + (int)(pair / mr.n_pat);
    const int tt = mr.t_list[s];
    const int tp = mr.t_list[s > 0 ? s - 1 : 0];
    const float a = sqrt_ac[tt], b = sqrt_1m[tt], ap = sqrt_ac[tp], bp = sqrt_1m[tp];
    const float cA = mr.coef[4 * s];
    const bool solve = s > 0 && target_out;          // uniform over the workgroup
    const bool last = s == mr.n_steps - 1 && x_start;
    if (threadIdx.x == 0) {
      if (t_out) t_out[r] = tt;
      if (solve) {
        MapRow rec;
        rec.B = mr.coef[4 * s + 1]; rec.invC = 1.0f / mr.coef[4 * s + 2];
        rec.zoff = ((long long)(mr.n_steps - 1 - s) * mr.n_pat + i) * cols;
        row_out[r] = rec;
      }
    }
    if (cond_out && (int)threadIdx.x < cd) cond_out[r * cd + threadIdx.x] = cond[i * cd + threadIdx.x];
    const float* xrow = x0 + i * cols;
    const float* nrow = noise_in ? noise_in + ((int64_t)s * mr.n_pat + i) * cols : nullptr;
    const float* prow = noise_in && s > 0 ? noise_in + ((int64_t)(s - 1) * mr.n_pat + i) * cols : nullptr;
    for (int q = threadIdx.x; q < c4n; q += 256) {
      const int c = 4 * q;
      const float4 x = ld4g(xrow, c, cols);
      float4 n;
      if (nrow) n = ld4g(nrow, c, cols);
      else n = randn4(seed, row_offset + (uint32_t)i, (uint32_t)q, (uint32_t)tt, TAG_QNOISE);
      float4 y;
      y.x = __fadd_rn(__fmul_rn(a, x.x), __fmul_rn(b, n.x));
      y.y = __fadd_rn(__fmul_rn(a, x.y), __fmul_rn(b, n.y));
      y.z = __fadd_rn(__fmul_rn(a, x.z), __fmul_rn(b, n.z));
      y.w = __fadd_rn(__fmul_rn(a, x.w), __fmul_rn(b, n.w));
      if (x_t) {
        st4g(x_t + r * ldxt, c, cols, y);
        zero_pad(x_t + r * ldxt, cols, ldxt, c);
      }
      if (last) st4g(x_start + i * cols, c, cols, y);
      if (!solve) continue;
      float4 m;
      if (prow) m = ld4g(prow, c, cols);
      else m = randn4(seed, row_offset + (uint32_t)i, (uint32_t)q, (uint32_t)tp, TAG_QNOISE);
      float4 u;
      u.x = fmaf(-cA, y.x, __fadd_rn(__fmul_rn(ap, x.x), __fmul_rn(bp, m.x)));
      u.y = fmaf(-cA, y.y, __fadd_rn(__fmul_rn(ap, x.y), __fmul_rn(bp, m.y)));
      u.z = fmaf(-cA, y.z, __fadd_rn(__fmul_rn(ap, x.z), __fmul_rn(bp, m.z)));
      u.w = fmaf(-cA, y.w, __fadd_rn(__fmul_rn(ap, x.w), __fmul_rn(bp, m.w)));
      st4g(target_out + r * cols, c, cols, u);
    }
  }
}
hipError_t launch_q_sample_map(hipStream_t s, const float* x0, const float* cond, int cd, const MapRows& mr, const float* sqrt_ac,
                               const float* sqrt_1m, const float* noise_in, int64_t rows, int cols, uint64_t seed, uint32_t row_offset, float* x_t,
                               int ldxt, float* target_out, MapRow* row_out, float* x_start, int* t_out, float* cond_out, const ZeroList* zl) {
  if (rows <= 0) return hipSuccess;
  if (mr.n_pat < 1 || !mr.t_list || !mr.coef || mr.s0 < 0 || cd > 256) return hipErrorInvalidValue;
  if (mr.pair0 < 0 || mr.pair0 + rows > (int64_t)(mr.n_steps - mr.s0) * mr.n_pat) return hipErrorInvalidValue;      // every row names a level of the plan
  if ((target_out != nullptr) != (row_out != nullptr) || (x_t && !t_out)) return hipErrorInvalidValue;
  ZeroList z{};
  if (zl) z = *zl;
  int64_t blocks = rows < 16384 ? rows : 16384;
  if (blocks < (zl ? 32 : 1)) blocks = zl ? 32 : 1;      // the zero list is walked by the first 32 workgroups
  hipLaunchKernelGGL(k_q_sample_map, dim3((unsigned)blocks), 256, 0, s, x0, cond, cd, mr, sqrt_ac, sqrt_1m, noise_in, rows, cols, seed, row_offset,
                     x_t, ldxt > 0 ? ldxt : cols, target_out, row_out, x_start, t_out, cond_out, z);
  return hipGetLastError();
}

// Classifier-free guidance (utils/generate.py:97-110, guidance_scale) on the last hidden activation: output_proj is linear, so
// eps_u + w (eps_c - eps_u) = output_proj(h_u + w (h_c - h_u)) and the combination costs a pass over [m][256], not over [m][D].
// h: [2 m][cols], rows [0, m) the conditional branch, rows [m, 2 m) the unconditional one; row r < m is overwritten with
// h_u + w * (h_c - h_u): one subtract, one fma (h_c == h_u leaves h_u exactly, whatever w).
__global__ void k_guide_combine(float* h, int64_t quads, float w) {
  float4* hc = reinterpret_cast<float4*>(h);
  const float4* hu = hc + quads;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < quads; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 c = hc[i], u = hu[i];
    float4 o;
    o.x = fmaf(w, c.x - u.x, u.x); o.y = fmaf(w, c.y - u.y, u.y);
    o.z = fmaf(w, c.z - u.z, u.z); o.w = fmaf(w, c.w - u.w, u.w);
    hc[i] = o;
  }
}
hipError_t launch_guide_combine(hipStream_t s, float* h, int64_t m, int cols, float w) {
  if (m <= 0) return hipSuccess;
  if (cols % 4 || (reinterpret_cast<uintptr_t>(h) & 15)) return hipErrorInvalidValue;
  const int64_t quads = m * (cols / 4);
  hipLaunchKernelGGL(k_guide_combine, ew_grid(quads), 256, 0, s, h, quads, w);
  return hipGetLastError();
}

// Condition dropout of a training batch (classifier-free guidance, Ho & Salimans 2022): out[r] = keep(r) ? cond[r] : null_cond.
// keep(r) = keep[r] != 0 when a keep vector is injected, else u01(word 0 of the Philox block (row_offset + r, 0, 0, TAG_COND_DROP))
// >= p -- the dropout keep-mask's construction (epilogues.h: EpiGnSilu) with one column per row.
__global__ void k_cond_dropout(const float* cond, const float* null_cond, const float* keep, float p, int64_t rows, int cd, uint64_t seed,
                               uint32_t row_offset, float* out) {
  const int64_t total = rows * cd;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / cd;
    const int c = (int)(i - r * cd);
    out[i] = cond_kept(keep, p, seed, row_offset, r) ? cond[i] : null_cond[c];
  }
}
hipError_t launch_cond_dropout(hipStream_t s, const float* cond, const float* null_cond, const float* keep, float p, int64_t rows, int cd,
                               uint64_t seed, uint32_t row_offset, float* out) {
  if (rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_cond_dropout, ew_grid(rows * cd), 256, 0, s, cond, null_cond, keep, p, rows, cd, seed, row_offset, out);
  return hipGetLastError();
}

// caller-supplied timestep indices clamped into [lo, hi]: an index outside [0, T) is a caller error (the Python
// shim raises IndexError as the reference's buffer gather would); the clamp only keeps the table gathers in bounds
__global__ void k_clamp_int(const int* in, int64_t n, int lo, int hi, int* out) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int v = in[i];
    out[i] = v < lo ? lo : (v > hi ? hi : v);
  }
}
hipError_t launch_clamp_int(hipStream_t s, const int* in, int64_t n, int lo, int hi, int* out) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_clamp_int, ew_grid(n), 256, 0, s, in, n, lo, hi, out);
  return hipGetLastError();
}

// torch.randint(0, T, (B,)) stand-in (models/diffusion.py:361): uniform ints from Philox.
__global__ void k_randint(int* out, int64_t n, int hi, uint64_t seed, uint32_t row_offset) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const uint4 r = philox_at(seed, row_offset + (uint32_t)i, 0u, 0u, TAG_TSTEP);
    out[i] = (int)(((uint64_t)r.x * (uint64_t)hi) >> 32);
  }
}
hipError_t launch_randint(hipStream_t s, int* out, int64_t n, int hi, uint64_t seed, uint32_t row_offset) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_randint, ew_grid(n), 256, 0, s, out, n, hi, seed, row_offset);
  return hipGetLastError();
}

// mixup (utils/train.py:117-119): lam*v + (1-lam)*v[perm], products rounded separately.
__global__ void k_mixup(const float* v, const int64_t* perm, float lam, float oml, int64_t rows, int cols, float* out) {
  const int c4n = (cols + 3) >> 2;
  const int64_t total = rows * c4n;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / c4n;
    const int c = 4 * (int)(i - r * c4n);
    const float4 a = ld4g(v + r * cols, c, cols);
    const float4 b = ld4g(v + perm[r] * cols, c, cols);
    float4 o;
    o.x = __fadd_rn(__fmul_rn(lam, a.x), __fmul_rn(oml, b.x));
    o.y = __fadd_rn(__fmul_rn(lam, a.y), __fmul_rn(oml, b.y));
    o.z = __fadd_rn(__fmul_rn(lam, a.z), __fmul_rn(oml, b.z));
    o.w = __fadd_rn(__fmul_rn(lam, a.w), __fmul_rn(oml, b.w));
    st4g(out + r * cols, c, cols, o);
  }
}
hipError_t launch_mixup(hipStream_t s, const float* v, const int64_t* perm, double lam, int64_t rows, int cols, float* out) {
  if (rows <= 0) return hipSuccess;
  // python: lam and (1 - lam) are float64 scalars; torch multiplies an fp32 tensor by each as fp32
  const float oml = (float)(1.0 - lam);
  hipLaunchKernelGGL(k_mixup, ew_grid(rows * ((cols + 3) / 4)), 256, 0, s, v, perm, (float)lam, oml, rows, cols, out);
  return hipGetLastError();
}

// the three tensors of MixupAugmentation.__call__ (data [n][D], conditions [n][cd], survival [n]) in one launch
__global__ void k_mixup3(const float* d, const float* c, const float* sv, const int64_t* perm, float lam, float oml, int64_t rows, int D, int cd,
                         float* od, float* oc, float* os) {
  const int d4 = (D + 3) >> 2, c4 = (cd + 3) >> 2;
  const int per_row = d4 + c4 + 1;
  const int64_t total = rows * per_row;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / per_row;
    int j = (int)(i - r * per_row);
    const int64_t pr = perm[r];
    const float* src; float* dst; int cols, col;
    if (j < d4) { src = d; dst = od; cols = D; col = 4 * j; }
    else if (j < d4 + c4) { src = c; dst = oc; cols = cd; col = 4 * (j - d4); }
    else { src = sv; dst = os; cols = 1; col = 0; }
    if (!src || !dst) continue;
    const float4 a = ld4g(src + r * cols, col, cols);
    const float4 b = ld4g(src + pr * cols, col, cols);
    float4 o;
    o.x = __fadd_rn(__fmul_rn(lam, a.x), __fmul_rn(oml, b.x));
    o.y = __fadd_rn(__fmul_rn(lam, a.y), __fmul_rn(oml, b.y));
    o.z = __fadd_rn(__fmul_rn(lam, a.z), __fmul_rn(oml, b.z));
    o.w = __fadd_rn(__fmul_rn(lam, a.w), __fmul_rn(oml, b.w));
    st4g(dst + r * cols, col, cols, o);
  }
}
hipError_t launch_mixup3(hipStream_t s, const float* d, const float* c, const float* sv, const int64_t* perm, double lam, int64_t rows, int D,
                         int cd, float* od, float* oc, float* os) {
  if (rows <= 0) return hipSuccess;
  const float oml = (float)(1.0 - lam);
  hipLaunchKernelGGL(k_mixup3, ew_grid(rows * ((D + 3) / 4 + (cd + 3) / 4 + 1)), 256, 0, s, d, c, sv, perm, (float)lam, oml, rows, D, cd, od, oc, os);
  return hipGetLastError();
}

__global__ void k_threshold(const float* x, int ldx, int64_t rows, int cols, float thr, float* out) {
  const int64_t total = rows * cols;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / cols;
    const int c = (int)(i - r * cols);
    out[i] = (x[r * ldx + c] > thr) ? 1.0f : 0.0f;
  }
}
hipError_t launch_threshold(hipStream_t s, const float* x, int ldx, int64_t rows, int cols, float thr, float* out) {
  if (rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_threshold, ew_grid(rows * cols), 256, 0, s, x, ldx, rows, cols, thr, out);
  return hipGetLastError();
}

}  // namespace osd
