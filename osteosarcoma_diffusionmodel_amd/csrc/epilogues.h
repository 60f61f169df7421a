// epilogues.h -- fused epilogues for gemm_kernel (see gemm.h for the fragment layout).
//
// Every epilogue loads its side inputs from CLAMPED indices (always in range) and guards only
// the stores, so in FAST mode no load sits behind a branch and the compiler issues them all
// before a single wait.  fast_ok() tells the host whether FAST's alignment/divisibility
// preconditions hold for the epilogue's own pointers.
#pragma once
#include "gemm.h"
#include "rng.h"
#include "xpose.h"
#include <type_traits>

namespace osd {

constexpr float GN_EPS = 1e-5f;

// SiLU with the hardware exp2 / rcp (v_exp_f32, v_rcp_f32; ~1 ulp each): a handful of VALU issues per
// element instead of the ~30 of expf() + an IEEE divide.  Relative error <= ~4e-7 of |silu(x)|.
__device__ __forceinline__ float silu_f(float x) {
  const float e = __builtin_amdgcn_exp2f(x * -1.4426950408889634f);
  return x * __builtin_amdgcn_rcpf(1.0f + e);
}

// value of lane^32 (the other half-wave), through v_permlane32_swap instead of an LDS bpermute
__device__ __forceinline__ float swap_halves(float v) {
  const unsigned u = __float_as_uint(v);
  const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  // after the swap: r[0] holds {own low half | partner's low half -> upper lanes ...}; lane < 32 reads r[1]'s low, lane >= 32 reads r[0]'s high
  return __uint_as_float((__lane_id() < 32) ? r[1] : r[0]);
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ---- bias (+ optional SiLU, + optional accumulate into out) -----------------------
template <bool SILU, bool ACCUM>
struct EpiBias {
  static constexpr bool COUNTED_STORES = true;    // one float4 store per accumulator quad on a full tile
  static constexpr bool XBUF = false;             // true: apply() takes the wave's LDS transposer region (xpose.h)
  struct Args { const float* bias; float* out; int ldo; long long slice_stride; };
  static bool fast_ok(const Args& a, int F) { return F % 4 == 0 && al16(a.bias) && al16(a.out) && a.ldo % 4 == 0 && a.slice_stride % 4 == 0; }
  static __device__ __forceinline__ void slice(Args& a, int y) { a.out += (long long)y * a.slice_stride; }
  template <int NFB> struct Pre { float4 bias[NFB][4]; };
  template <int NFB, bool FAST>
  static __device__ __forceinline__ Pre<NFB> prefetch(const Args& a, int fw, int lane, int F) {
    Pre<NFB> r;
    const int h = lane >> 5;
#pragma unroll
    for (int fb = 0; fb < NFB; ++fb)
#pragma unroll
      for (int q = 0; q < 4; ++q)
        r.bias[fb][q] = a.bias ? ldq<FAST>(a.bias, fw + 32 * fb + 8 * q + 4 * h, F) : make_float4(0.f, 0.f, 0.f, 0.f);
    return r;
  }
  template <int NFB, int NPB, bool FAST>
  static __device__ __forceinline__ void apply(f32x16 (&acc)[NFB][NPB], const Args& a, const Pre<NFB>& pre, int fw, int pw, int lane, int F, int P) {
    const int l31 = lane & 31, h = lane >> 5;
    OSD_FOR_QUADS(fb, pb, q) {
      const int f = fw + 32 * fb + 8 * q + 4 * h;
      const int p = pw + 32 * pb + l31;
      const int pc = p < P ? p : P - 1;
      float4 v = make_float4(acc[fb][pb][4 * q], acc[fb][pb][4 * q + 1], acc[fb][pb][4 * q + 2], acc[fb][pb][4 * q + 3]);
      { const float4 bv = pre.bias[fb][q]; v.x += bv.x; v.y += bv.y; v.z += bv.z; v.w += bv.w; }
      float* row = a.out + (size_t)pc * a.ldo;
      if (ACCUM) { const float4 o = ldq<FAST>(row, f, F); v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w; }
      if (SILU) { v.x = silu_f(v.x); v.y = silu_f(v.y); v.z = silu_f(v.z); v.w = silu_f(v.w); }
      if (p < P) stq<FAST>(row, f, F, v);
    }
  }
};

// ---- input_proj: h = ((x W^T + b) + t_emb[t]) + c_proj   (models/diffusion.py:229-232) ----
struct EpiInput {
  static constexpr bool KSPLIT2 = true;            // launch.h: the two-wave-group variant of the LDS-DMA kernel is instantiated for it
  static constexpr bool COUNTED_STORES = true;
  static constexpr bool XBUF = false;
  template <class A> static __device__ __forceinline__ void slice(A&, int) {}
  struct Args {
    const float* bias;
    const float* temb; int ldt;   // [T][F] time_proj(TimeEmbedding(t/T))
    const int* t_index;           // per-row t or null
    const int* t_dev; int t_imm;  // shared t: *t_dev if non-null else t_imm
    const float* cproj; int ldc;  // [P][F]
    float* out; int ldo;
  };
  static bool fast_ok(const Args& a, int F) {
    return F % 4 == 0 && al16(a.bias) && al16(a.temb) && al16(a.cproj) && al16(a.out) && a.ldt % 4 == 0 && a.ldc % 4 == 0 && a.ldo % 4 == 0;
  }
  template <int NFB> struct Pre { float4 bias[NFB][4]; };
  template <int NFB, bool FAST>
  static __device__ __forceinline__ Pre<NFB> prefetch(const Args& a, int fw, int lane, int F) {
    Pre<NFB> r;
    const int h = lane >> 5;
#pragma unroll
    for (int fb = 0; fb < NFB; ++fb)
#pragma unroll
      for (int q = 0; q < 4; ++q) r.bias[fb][q] = ldq<FAST>(a.bias, fw + 32 * fb + 8 * q + 4 * h, F);
    return r;
  }
  template <int NFB, int NPB, bool FAST>
  static __device__ __forceinline__ void apply(f32x16 (&acc)[NFB][NPB], const Args& a, const Pre<NFB>& pre, int fw, int pw, int lane, int F, int P) {
    const int l31 = lane & 31, h = lane >> 5;
    const int t_shared = a.t_dev ? *a.t_dev : a.t_imm;
#pragma unroll
    for (int pb = 0; pb < NPB; ++pb) {
      const int p = pw + 32 * pb + l31;
      const int pc = p < P ? p : P - 1;
      const int t = a.t_index ? a.t_index[pc] : t_shared;
      const float* trow = a.temb + (size_t)t * a.ldt;
      const float* crow = a.cproj + (size_t)pc * a.ldc;
      float* orow = a.out + (size_t)pc * a.ldo;
#pragma unroll
      for (int fb = 0; fb < NFB; ++fb)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int f = fw + 32 * fb + 8 * q + 4 * h;
          const float4 bv = pre.bias[fb][q], tv = ldq<FAST>(trow, f, F), cv = ldq<FAST>(crow, f, F);
          float4 v;
          v.x = ((acc[fb][pb][4 * q] + bv.x) + tv.x) + cv.x;
          v.y = ((acc[fb][pb][4 * q + 1] + bv.y) + tv.y) + cv.y;
          v.z = ((acc[fb][pb][4 * q + 2] + bv.z) + tv.z) + cv.z;
          v.w = ((acc[fb][pb][4 * q + 3] + bv.w) + tv.w) + cv.w;
          if (p < P) stq<FAST>(orow, f, F, v);
        }
    }
  }
};

// ---- input_proj of a classifier-free-guidance step: one product, two outputs ----
// x W^T does not depend on the condition, so the conditional and the unconditional branch of a guided evaluation
// (utils/generate.py:97-110, guidance_scale) share the GEMM: row p of the m state rows leaves as
//   out[p]     = ((acc + b) + t_emb[t]) + c_proj[p]      the row's own condition
//   out[m + p] = ((acc + b) + t_emb[t]) + c_proj0        the null condition, one [F] row for every patient
// Each half is EpiInput's arithmetic operation for operation: a row whose condition IS the null condition gets two
// bit-identical halves.
struct EpiInputGuided {
  static constexpr bool KSPLIT2 = true;
  static constexpr bool COUNTED_STORES = true;     // two float4 stores per accumulator quad on a full tile: the count the kernel waits on is a lower bound
  static constexpr bool XBUF = false;
  template <class A> static __device__ __forceinline__ void slice(A&, int) {}
  struct Args {
    const float* bias;
    const float* temb; int ldt;
    const int* t_index;
    const int* t_dev; int t_imm;
    const float* cproj; int ldc;  // [P][F]
    const float* cproj0;          // [F]
    float* out; int ldo;          // [2 P][F]
    long long half;               // floats between out[p] and out[P + p] (= P * ldo)
  };
  static bool fast_ok(const Args& a, int F) {
    return F % 4 == 0 && al16(a.bias) && al16(a.temb) && al16(a.cproj) && al16(a.cproj0) && al16(a.out) && a.ldt % 4 == 0 && a.ldc % 4 == 0 &&
           a.ldo % 4 == 0 && a.half % 4 == 0;
  }
  template <int NFB> struct Pre { float4 bias[NFB][4]; };
  template <int NFB, bool FAST>
  static __device__ __forceinline__ Pre<NFB> prefetch(const Args& a, int fw, int lane, int F) {
    Pre<NFB> r;
    const int h = lane >> 5;
#pragma unroll
    for (int fb = 0; fb < NFB; ++fb)
#pragma unroll
      for (int q = 0; q < 4; ++q) r.bias[fb][q] = ldq<FAST>(a.bias, fw + 32 * fb + 8 * q + 4 * h, F);
    return r;
  }
  template <int NFB, int NPB, bool FAST>
  static __device__ __forceinline__ void apply(f32x16 (&acc)[NFB][NPB], const Args& a, const Pre<NFB>& pre, int fw, int pw, int lane, int F, int P) {
    const int l31 = lane & 31, h = lane >> 5;
    const int t_shared = a.t_dev ? *a.t_dev : a.t_imm;
#pragma unroll
    for (int pb = 0; pb < NPB; ++pb) {
      const int p = pw + 32 * pb + l31;
      const int pc = p < P ? p : P - 1;
      const int t = a.t_index ? a.t_index[pc] : t_shared;
      const float* trow = a.temb + (size_t)t * a.ldt;
      const float* crow = a.cproj + (size_t)pc * a.ldc;
      float* orow = a.out + (size_t)pc * a.ldo;
#pragma unroll
      for (int fb = 0; fb < NFB; ++fb)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int f = fw + 32 * fb + 8 * q + 4 * h;
          const float4 bv = pre.bias[fb][q], tv = ldq<FAST>(trow, f, F), cv = ldq<FAST>(crow, f, F), nv = ldq<FAST>(a.cproj0, f, F);
          float4 s, v, u;
          s.x = (acc[fb][pb][4 * q] + bv.x) + tv.x;
          s.y = (acc[fb][pb][4 * q + 1] + bv.y) + tv.y;
          s.z = (acc[fb][pb][4 * q + 2] + bv.z) + tv.z;
          s.w = (acc[fb][pb][4 * q + 3] + bv.w) + tv.w;
          v.x = s.x + cv.x; v.y = s.y + cv.y; v.z = s.z + cv.z; v.w = s.w + cv.w;
          u.x = s.x + nv.x; u.y = s.y + nv.y; u.z = s.z + nv.z; u.w = s.w + nv.w;
          if (p < P) {
            stq<FAST>(orow, f, F, v);
            stq<FAST>(orow + a.half, f, F, u);
          }
        }
    }
  }
};

// ---- Linear -> GroupNorm(8) -> SiLU [-> Dropout]   (models/diffusion.py:200-204) ----
// GW = channels per group (C/8), a power of two in [4,128]; the wave's feature extent
// covers whole groups, so a group's statistics are a sum over this lane's registers plus
// (GW >= 8) one exchange with lane^32.
// DROP compiles the dropout code in; drop_mode then selects 0 none, 1 keep-mask from
// memory, 2 Philox keep-mask.  z_out != null also stores the pre-norm activations and
// (mean, rstd) for backward.
template <int GW, bool DROP>
struct EpiGnSilu {
  static constexpr bool KSPLIT2 = GW == 32 || GW == 64;      // the widths of the BASELINE trunk (256 / 512): two-wave-group variant instantiated
  static constexpr bool COUNTED_STORES = true;
  static constexpr bool XBUF = false;
  template <class A> static __device__ __forceinline__ void slice(A&, int) {}
  struct Args {
    const float* bias; const float* gamma; const float* beta;
    float* out; int ldo;
    float* z_out; int ldz;            // optional: pre-norm [P][F]
    float* stats;                     // with z_out: [P][F/GW][2] = (mean, rstd)
    int drop_mode;
    const float* mask; int ldm;       // drop_mode 1
    float keep_scale; float p_drop;   // 1/(1-p), p
    uint64_t seed; uint32_t row_offset; uint32_t step; uint32_t tag;   // drop_mode 2
    const int* step_dev;              // drop_mode 2: step = *step_dev when non-null
  };
  static bool fast_ok(const Args& a, int F) {
    return F % 4 == 0 && al16(a.bias) && al16(a.gamma) && al16(a.beta) && al16(a.out) && a.ldo % 4 == 0 &&
           (!a.z_out || (al16(a.z_out) && a.ldz % 4 == 0)) && (a.drop_mode != 1 || (al16(a.mask) && a.ldm % 4 == 0));
  }
  // per-feature parameters of this lane's quads: fetched before the K loop so their latency is hidden
  template <int NFB> struct Pre { float4 bias[NFB][4], gamma[NFB][4], beta[NFB][4]; };
  template <int NFB, bool FAST>
  static __device__ __forceinline__ Pre<NFB> prefetch(const Args& a, int fw, int lane, int F) {
    Pre<NFB> r;
    const int h = lane >> 5;
#pragma unroll
    for (int fb = 0; fb < NFB; ++fb)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int f = fw + 32 * fb + 8 * q + 4 * h;
        r.bias[fb][q] = ldq<FAST>(a.bias, f, F);
        r.gamma[fb][q] = ldq<FAST>(a.gamma, f, F);
        r.beta[fb][q] = ldq<FAST>(a.beta, f, F);
      }
    return r;
  }
  template <int NFB, int NPB, bool FAST>
  static __device__ __forceinline__ void apply(f32x16 (&acc)[NFB][NPB], const Args& a, const Pre<NFB>& pre, int fw, int pw, int lane, int F, int P) {
    static_assert(NFB * 32 >= GW, "wave must own whole groups");
    constexpr int RPG = (GW >= 8) ? GW / 2 : 4;   // registers of one group in this lane
    constexpr int NG = NFB * 16 / RPG;
    const int l31 = lane & 31, h = lane >> 5;
    // bias
#pragma unroll
    for (int fb = 0; fb < NFB; ++fb)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 bv = pre.bias[fb][q];
#pragma unroll
        for (int pb = 0; pb < NPB; ++pb) {
          acc[fb][pb][4 * q] += bv.x; acc[fb][pb][4 * q + 1] += bv.y;
          acc[fb][pb][4 * q + 2] += bv.z; acc[fb][pb][4 * q + 3] += bv.w;
        }
      }
#pragma unroll
    for (int pb = 0; pb < NPB; ++pb) {
      const int p = pw + 32 * pb + l31;
      const bool prow = p < P;
      const int pc = prow ? p : P - 1;
      float mean[NG], rstd[NG];
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < RPG; ++j) { const int L = g * RPG + j; s += acc[L / 16][pb][L % 16]; }
        if (GW >= 8) s += swap_halves(s);
        const float m = s * (1.0f / GW);
        float qs = 0.f;
#pragma unroll
        for (int j = 0; j < RPG; ++j) { const int L = g * RPG + j; const float d = acc[L / 16][pb][L % 16] - m; qs = fmaf(d, d, qs); }
        if (GW >= 8) qs += swap_halves(qs);
        mean[g] = m;
        rstd[g] = 1.0f / sqrtf(qs * (1.0f / GW) + GN_EPS);
      }
      float* orow = a.out + (size_t)pc * a.ldo;
#pragma unroll
      for (int fb = 0; fb < NFB; ++fb)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int f = fw + 32 * fb + 8 * q + 4 * h;
          const int g = (fb * 16 + 4 * q) / RPG;
          const float4 gv = pre.gamma[fb][q], bev = pre.beta[fb][q];
          const float4 z = make_float4(acc[fb][pb][4 * q], acc[fb][pb][4 * q + 1], acc[fb][pb][4 * q + 2], acc[fb][pb][4 * q + 3]);
          if (a.z_out && prow) {
            stq<FAST>(a.z_out + (size_t)p * a.ldz, f, F, z);
            if ((f % GW) == 0 && f < F) {   // first quad of the group in this lane-pair writes the stats
              float* sp = a.stats + ((size_t)p * (F / GW) + f / GW) * 2;
              sp[0] = mean[g]; sp[1] = rstd[g];
            }
          }
          float4 y;
          y.x = silu_f(fmaf((z.x - mean[g]) * rstd[g], gv.x, bev.x));
          y.y = silu_f(fmaf((z.y - mean[g]) * rstd[g], gv.y, bev.y));
          y.z = silu_f(fmaf((z.z - mean[g]) * rstd[g], gv.z, bev.z));
          y.w = silu_f(fmaf((z.w - mean[g]) * rstd[g], gv.w, bev.w));
          if (DROP && a.drop_mode == 1) {
            const float4 mk = ldq<FAST>(a.mask + (size_t)pc * a.ldm, f, F);
            y.x *= mk.x * a.keep_scale; y.y *= mk.y * a.keep_scale; y.z *= mk.z * a.keep_scale; y.w *= mk.w * a.keep_scale;
          } else if (DROP && a.drop_mode == 2) {
            const uint32_t step = a.step_dev ? (uint32_t)*a.step_dev : a.step;
            const uint4 r = philox_at(a.seed, a.row_offset + (uint32_t)p, (uint32_t)(f >> 2), step, a.tag);
            y.x *= (u01(r.x) >= a.p_drop) ? a.keep_scale : 0.f;
            y.y *= (u01(r.y) >= a.p_drop) ? a.keep_scale : 0.f;
            y.z *= (u01(r.z) >= a.p_drop) ? a.keep_scale : 0.f;
            y.w *= (u01(r.w) >= a.p_drop) ? a.keep_scale : 0.f;
          }
          if (prow) stq<FAST>(orow, f, F, y);
        }
    }
  }
};

// ---- dgrad fused with the GroupNorm(8) + SiLU (+ dropout) BACKWARD of the layer it feeds (loss.backward(), utils/train.py:239) ----
// The GEMM is a dgrad: acc = g = dL/d(out) of layer L, where out = dropout(silu(y)), y = zhat * gamma + beta,
// zhat = (z - mean) * rstd (models/diffusion.py:200-204).  A lane holds one row and whole groups of it (the forward epilogue's
// layout), so the per-(row, group) sums of the GroupNorm backward are a register sum + one lane^32 exchange and dL/dz leaves
// the kernel directly -- no separate pass over g:
//   gy   = g * keep * silu'(y),  gzh = gy * gamma
//   gz   = rstd * (gzh - mean_group(gzh) - zhat * mean_group(gzh * zhat))
// `gy` is stored too (into the buffer g would have gone to): d gamma = colsum(gy * zhat), d beta = colsum(gy) are taken from
// it by one grouped column-sum launch per flush (k_gn_colsums); d bias = colsum(gz) rides with the weight-gradient launch.
// g_add: a partial gradient already in the gy buffer (the skip connection's share) is added first, in place.
template <int GW, bool DROP>
struct EpiGnBwd {
  static constexpr bool KSPLIT2 = true;            // launch.h: the two-wave-group variant of gemm_kernel is instantiated for the 64 x 64 tile
  static constexpr bool COUNTED_STORES = false;
  static constexpr bool XBUF = false;
  template <class A> static __device__ __forceinline__ void slice(A&, int) {}
  struct Args {
    const float* z; int ldz;          // pre-norm activations of layer L  [P][F]
    const float* stats;               // (mean, rstd) [P][F/GW][2]
    const float* gamma; const float* beta;
    float* gz; int ldg;               // dL/dz                            [P][F]
    float* gy; int ldy;               // dL/dy (and, when accumulate, the incoming partial g)  [P][F]
    int accumulate;
    int drop_mode; const float* mask; int ldm; float keep_scale; float p_drop;
    uint64_t seed; uint32_t row_offset; uint32_t step; uint32_t tag;
  };
  static bool fast_ok(const Args& a, int F) {
    return F % 4 == 0 && F % GW == 0 && al16(a.z) && a.ldz % 4 == 0 && al16(a.gamma) && al16(a.beta) && al16(a.gz) && a.ldg % 4 == 0 &&
           al16(a.gy) && a.ldy % 4 == 0 && (a.drop_mode != 1 || (al16(a.mask) && a.ldm % 4 == 0));
  }
  template <int NFB> struct Pre { float4 gamma[NFB][4], beta[NFB][4]; };
  template <int NFB, bool FAST>
  static __device__ __forceinline__ Pre<NFB> prefetch(const Args& a, int fw, int lane, int F) {
    Pre<NFB> r;
    const int h = lane >> 5;
#pragma unroll
    for (int fb = 0; fb < NFB; ++fb)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int f = fw + 32 * fb + 8 * q + 4 * h;
        r.gamma[fb][q] = ldq<FAST>(a.gamma, f, F);
        r.beta[fb][q] = ldq<FAST>(a.beta, f, F);
      }
    return r;
  }
  template <int NFB, int NPB, bool FAST>
  static __device__ __forceinline__ void apply(f32x16 (&acc)[NFB][NPB], const Args& a, const Pre<NFB>& pre, int fw, int pw, int lane, int F, int P) {
    static_assert(GW >= 8 && NFB * 32 >= GW, "wave must own whole groups");
    constexpr int RPG = GW / 2;                 // registers of one group in this lane
    constexpr int NG = NFB * 16 / RPG;
    const int l31 = lane & 31, h = lane >> 5;
#pragma unroll
    for (int pb = 0; pb < NPB; ++pb) {
      const int p = pw + 32 * pb + l31;
      const bool prow = p < P;
      const int pc = prow ? p : P - 1;
      const float* zrow = a.z + (size_t)pc * a.ldz;
      float* gyrow = a.gy + (size_t)pc * a.ldy;
      float* gzrow = a.gz + (size_t)pc * a.ldg;
      // pass 1: gy (kept in acc), zhat recomputed in pass 2 from z; group sums
      float zh[NFB][16];
      float s1[NG], s2[NG];
#pragma unroll
      for (int g = 0; g < NG; ++g) s1[g] = s2[g] = 0.f;
#pragma unroll
      for (int fb = 0; fb < NFB; ++fb)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int f = fw + 32 * fb + 8 * q + 4 * h;
          const int g = (fb * 16 + 4 * q) / RPG;
          const int fc = f < F ? f : F - 4;
          const float2 st = ldg2(a.stats + ((size_t)pc * (F / GW) + fc / GW) * 2);
          const float4 z4 = ldq<FAST>(zrow, f, F);
          float4 add = make_float4(0.f, 0.f, 0.f, 0.f);
          if (a.accumulate) add = ldq<FAST>(gyrow, f, F);
          const float4 gv = pre.gamma[fb][q], bev = pre.beta[fb][q];
          float keep[4] = {1.f, 1.f, 1.f, 1.f};
          if (DROP && a.drop_mode == 1) {
            const float4 mk = ldq<FAST>(a.mask + (size_t)pc * a.ldm, f, F);
            keep[0] = mk.x * a.keep_scale; keep[1] = mk.y * a.keep_scale; keep[2] = mk.z * a.keep_scale; keep[3] = mk.w * a.keep_scale;
          } else if (DROP && a.drop_mode == 2) {
            const uint4 rr = philox_at(a.seed, a.row_offset + (uint32_t)p, (uint32_t)(f >> 2), a.step, a.tag);
            keep[0] = (u01(rr.x) >= a.p_drop) ? a.keep_scale : 0.f;
            keep[1] = (u01(rr.y) >= a.p_drop) ? a.keep_scale : 0.f;
            keep[2] = (u01(rr.z) >= a.p_drop) ? a.keep_scale : 0.f;
            keep[3] = (u01(rr.w) >= a.p_drop) ? a.keep_scale : 0.f;
          }
          const float zv[4] = {z4.x, z4.y, z4.z, z4.w};
          const float av[4] = {add.x, add.y, add.z, add.w};
          const float gm[4] = {gv.x, gv.y, gv.z, gv.w};
          const float bt[4] = {bev.x, bev.y, bev.z, bev.w};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int r = 4 * q + e;
            const float zhat = (zv[e] - st.x) * st.y;
            const float y = zhat * gm[e] + bt[e];
            const float sg = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(y * -1.4426950408889634f));   // hardware exp2 / rcp, as silu_f
            const float gyv = (acc[fb][pb][r] + av[e]) * keep[e] * (sg * (1.0f + y * (1.0f - sg)));
            const float gzh = gyv * gm[e];
            zh[fb][r] = zhat;
            acc[fb][pb][r] = gyv;
            s1[g] += gzh;
            s2[g] += gzh * zhat;
          }
          if (prow) stq<FAST>(gyrow, f, F, make_float4(acc[fb][pb][4 * q], acc[fb][pb][4 * q + 1], acc[fb][pb][4 * q + 2], acc[fb][pb][4 * q + 3]));
        }
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        s1[g] += swap_halves(s1[g]);
        s2[g] += swap_halves(s2[g]);
        s1[g] *= (1.0f / GW);
        s2[g] *= (1.0f / GW);
      }
      // pass 2: dL/dz
#pragma unroll
      for (int fb = 0; fb < NFB; ++fb)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int f = fw + 32 * fb + 8 * q + 4 * h;
          const int g = (fb * 16 + 4 * q) / RPG;
          const int fc = f < F ? f : F - 4;
          const float rstd = ldg1(a.stats + ((size_t)pc * (F / GW) + fc / GW) * 2 + 1);
          const float4 gv = pre.gamma[fb][q];
          const float gm[4] = {gv.x, gv.y, gv.z, gv.w};
          float o[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int r = 4 * q + e;
            o[e] = rstd * (acc[fb][pb][r] * gm[e] - s1[g] - zh[fb][r] * s2[g]);
          }
          if (prow) stq<FAST>(gzrow, f, F, make_float4(o[0], o[1], o[2], o[3]));
        }
    }
  }
};

// ---- output_proj fused with one step of the reverse chain: EpiPosterior<MODE, KNOWN> ----
// One quad walk (apply) serves every per-layer sampler.  MODE picks the element formula, KNOWN adds the overwrite of observed values;
// both are compile-time, so each of the six instantiations is its own kernel with no runtime switch.  t is the plan's step counter.
//
// POST_PLAIN, the DDPM / DDIM posterior (models/diffusion.py:398-425).  eps = acc + bias; the reference's x0 = (x - c0*eps)/c1,
// mean = c2*x0/c3 + c4*x/c3, x' = mean + c5*z is linear in (x, eps, z):   x' = A_t*x + B_t*eps + C_t*z   with
//   A_t = c4/c3 + c2/(c1*c3),  B_t = -c0*c2/(c1*c3),  C_t = c5        (t > 0)
//   A_0 = 1/c1,                B_0 = -c0/c1,          C_0 = 0         (t == 0: x' = x0)
// A, B, C are formed in double on the host from the reference's fp32 scalars and rounded once (osd_set_schedule), which replaces
// three IEEE divides per element by two FMAs; the result differs from the reference's op order by a few ulp of the same
// intermediate magnitudes.  coef [T][4] = (A_t, B_t, C_t, 0).  A step whose C is 0 (DDIM at eta = 0, and t == 0) draws no z: the
// Philox generator bounds this launch.
//
// KNOWN, sampling around observed values (the replacement method).  known [P][F]: a finite value is an
// observation of that element, NaN leaves it to the chain.  After the MODE's update, per element:
//   known element:  x' = La_t * known + Ls_t * z   (t > 0);   x' = known, bit for bit   (t == 0)
// level [S][2] = (La_t, Ls_t) = (sqrt(abar), sqrt(1 - abar)) of the timestep the step arrives at, (1, 0) at t = 0.  z is the step's
// posterior draw at the element's own address -- a replaced element has no other use for it -- so every step with t > 0 draws, also
// where C_t = 0; a quad without an observation has no use for the draw then, and its lanes skip the generator.  The free elements add
// the zero the unconstrained chain adds there (a select on the wave-uniform C_t, not a product with the draw), and an all-NaN `known`
// gives the unconstrained chain's bits.
//
// POST_CLIP, the predicted x0 clipped to per-feature bounds.  x0coef [S][4] = (P_t, Q_t, E_t, F_t); C_t is
// slot 2 of the coef row.  Per element:
//   x0  = fmaf(P, x, Q*eps)                        P = 1/sqrt(abar), Q = -sqrt(1-abar)/sqrt(abar)
//   x0c = fminf(fmaxf(x0, lo[f]), hi[f])           -inf / +inf leave a side free
//   x'  = fmaf(E, x0c, fmaf(F, x, C*z))            the direction term uses the eps the CLIPPED x0 implies, (x - sqrt(abar) x0c)/sqrt(1-abar)
// Row 0 is (P, Q, 1, 0) with C = 0: x' = x0c bit for bit, so every returned element lies inside [lo, hi].  C*z is the select on the
// wave-uniform C.  lo / hi depend on the feature only: loaded next to the x_t quads (2 x 16 float4 per wave tile held from before the
// K loop, the way the bias is, do not fit).
//
// POST_HIST, the DPM-Solver++(2M) multistep update (Lu et al. 2022).  POST_CLIP's deterministic step plus one
// term: the previous step's clipped x0, kept in hist [P][ldh] (ldh = ldx, the state's row stride), which the lane that owns an element
// reads and rewrites in place exactly as it does x.  x0coef [S][4] = (P_t, Q_t, G_t, F_t), hcoef [S] = H_t.  Per element:
//   hp  = hist[p][f];   hist[p][f] = x0c           the clipped network prediction, not the value after the `known` overwrite
//   x'  = fmaf(G, x0c, fmaf(F, x, H*hp))
// LINK (osd_set_output_link), POST_CLIP and POST_HIST only: columns f < n_link of the output are logits of a
// Bernoulli mean.  Right after x0 = fmaf(P, x, Q*eps) (P = 0, Q = 1: the type is OSD_PRED_SAMPLE) they take x0 = sigma(x0); the clamp,
// the update, the history store and the known overwrite follow unchanged.  A 32-column block at or past n_link takes a wave-uniform
// branch around the transcendentals.
// H is wave-uniform: where it is 0 (the first step run, whose history is the zeroed buffer, and t = 0) the read is skipped and hp = 0;
// the store is skipped at t = 0.  Row 0 is (P, Q, 1, 0) with H = 0: x' = x0c bit for bit.  No z: the generator runs only under KNOWN,
// for quads that hold an observation, at t > 0.  coef is not read.
enum PostMode { POST_PLAIN, POST_CLIP, POST_HIST };

struct PosteriorArgs {
  const float* bias;
  const float* xin; int ldx;
  float* xout; int ldo;
  const float* coef;              // dev [T][4] = (A_t, B_t, C_t, 0)
  const int* t_dev; int t_imm;
  const float* z; int ldzz;       // injected noise for draw 0 (t = t_first), [P][F]; null -> Philox
  long long z_step_stride; int t_first;   // draw for step t sits at z + (t_first - t) * stride
  uint64_t seed; uint32_t row_offset;
  float* mut_mask; int mutation_dim;   // written at t == 0 when non-null: (x' > 0.5)
};
struct PosteriorKnownArgs {
  PosteriorArgs p;
  const float* known; int ldk;    // [P][F], row stride ldk; NaN = free
  const float* level;             // dev [S][2] = (La_t, Ls_t)
};
struct PosteriorClipArgs {
  PosteriorArgs p;
  const float* lo; const float* hi;     // dev [F] each
  const float* x0coef;                  // dev [S][4] = (P_t, Q_t, E_t, F_t)
  const float* known; int ldk;          // KNOWN: [P][F], row stride ldk; NaN = free
  const float* level;                   // KNOWN: dev [S][2] = (La_t, Ls_t)
};
struct PosteriorHistArgs {
  PosteriorClipArgs c;
  float* hist; int ldh;                 // [P][ldh]
  const float* hcoef;                   // dev [S] = H_t
};
// LINK: the same with the logistic link on the columns [0, n_link) of the output (osd_set_output_link).  Types of their own, so that the
// kernels without a link keep their argument layout
struct PosteriorClipLinkArgs { PosteriorClipArgs c; int n_link; };
struct PosteriorHistLinkArgs { PosteriorHistArgs h; int n_link; };
// the nested parts of an argument struct: the common fields, the clip fields, and the struct that holds known / ldk / level
__host__ __device__ inline const PosteriorArgs& post_base(const PosteriorArgs& a) { return a; }
__host__ __device__ inline const PosteriorArgs& post_base(const PosteriorKnownArgs& a) { return a.p; }
__host__ __device__ inline const PosteriorArgs& post_base(const PosteriorClipArgs& a) { return a.p; }
__host__ __device__ inline const PosteriorArgs& post_base(const PosteriorHistArgs& a) { return a.c.p; }
__host__ __device__ inline const PosteriorArgs& post_base(const PosteriorClipLinkArgs& a) { return a.c.p; }
__host__ __device__ inline const PosteriorArgs& post_base(const PosteriorHistLinkArgs& a) { return a.h.c.p; }
__host__ __device__ inline const PosteriorClipArgs& post_clip(const PosteriorClipLinkArgs& a) { return a.c; }
__host__ __device__ inline const PosteriorClipArgs& post_clip(const PosteriorHistLinkArgs& a) { return a.h.c; }
__host__ __device__ inline const PosteriorClipArgs& post_known(const PosteriorClipLinkArgs& a) { return a.c; }
__host__ __device__ inline const PosteriorClipArgs& post_known(const PosteriorHistLinkArgs& a) { return a.h.c; }
template <class A> __host__ __device__ inline int post_n_link(const A&) { return 0; }
__host__ __device__ inline int post_n_link(const PosteriorClipLinkArgs& a) { return a.n_link; }
__host__ __device__ inline int post_n_link(const PosteriorHistLinkArgs& a) { return a.n_link; }
__host__ __device__ inline const PosteriorHistArgs& post_hist(const PosteriorHistArgs& a) { return a; }
__host__ __device__ inline const PosteriorHistArgs& post_hist(const PosteriorHistLinkArgs& a) { return a.h; }
__host__ __device__ inline const PosteriorClipArgs& post_clip(const PosteriorClipArgs& a) { return a; }
__host__ __device__ inline const PosteriorClipArgs& post_clip(const PosteriorHistArgs& a) { return a.c; }
__host__ __device__ inline const PosteriorKnownArgs& post_known(const PosteriorKnownArgs& a) { return a; }
__host__ __device__ inline const PosteriorClipArgs& post_known(const PosteriorClipArgs& a) { return a; }
__host__ __device__ inline const PosteriorClipArgs& post_known(const PosteriorHistArgs& a) { return a.c; }

// Quads requested ahead of their use; 0 = every x_t quad of the wave's tile before the first one is used (one latency, not sixteen;
// 64 registers).  The numbers are what fits: the 128 x 128 LDS-DMA kernels sit at 236 - 254 of the 256 VGPRs that two waves per SIMD
// allow.  Measured on that kernel:
//   plain + known: all x_t quads with the known quads beside them do not fit 256 VGPRs; a block's x_t and known quads are 32 registers
//   clip:          a whole block's x, lo, hi are 48 registers
//   hist:          two quads' x, lo, hi, hist are 32
//   clip + known, hist + known (the known quad rides along: 16 and 20 registers a quad): a whole block's 64 spill 31 VGPRs and
//                  half a block's 32 still spill one
// the Bernoulli mean of a logit (LINK), inside [0, 1]: hardware exp2 / rcp as silu_f; exp2 = +inf gives 0
__device__ __forceinline__ float link_sigmoid(float x) {
  return fminf(__builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(x * -1.4426950408889634f)), 1.0f);
}
//   link:          the bias quad rides along as well (EpiPosterior::Pre): clip asks for one quad at a time, two still spill one VGPR
constexpr int post_quads_ahead(PostMode m, bool known) { return m == POST_PLAIN ? (known ? 4 : 0) : known ? 1 : m == POST_CLIP ? 4 : 2; }

template <PostMode MODE, bool KNOWN, bool LINK = false>
struct EpiPosterior {
  static_assert(!LINK || MODE != POST_PLAIN, "POST_PLAIN folds x0 away: it cannot carry a link");
  static constexpr bool COUNTED_STORES = true;     // one x' quad per accumulator quad and, POST_HIST at t > 0, one history quad more: never fewer
  static constexpr bool XBUF = false;
  template <class A> static __device__ __forceinline__ void slice(A&, int) {}
  typedef std::conditional_t<MODE == POST_HIST, std::conditional_t<LINK, PosteriorHistLinkArgs, PosteriorHistArgs>,
                             std::conditional_t<MODE == POST_CLIP, std::conditional_t<LINK, PosteriorClipLinkArgs, PosteriorClipArgs>,
                                                std::conditional_t<KNOWN, PosteriorKnownArgs, PosteriorArgs>>> Args;
  static bool fast_ok(const Args& args, int F) {
    const PosteriorArgs& a = post_base(args);
    bool ok = F % 4 == 0 && al16(a.bias) && al16(a.xin) && al16(a.xout) && a.ldx % 4 == 0 && a.ldo % 4 == 0 &&
              (!a.z || (al16(a.z) && a.ldzz % 4 == 0 && a.z_step_stride % 4 == 0));
    if constexpr (MODE != POST_PLAIN) ok = ok && al16(post_clip(args).lo) && al16(post_clip(args).hi);
    if constexpr (KNOWN) ok = ok && al16(post_known(args).known) && post_known(args).ldk % 4 == 0;
    if constexpr (MODE == POST_HIST) ok = ok && al16(post_hist(args).hist) && post_hist(args).ldh % 4 == 0;
    return ok;
  }
  // LINK: the bias is not held across the K loop; its quads are requested with the x_t quads (32 registers less where the link's
  // branch needs them)
  template <int NFB> struct Pre { float4 bias[LINK ? 1 : NFB][LINK ? 1 : 4]; };
  template <int NFB, bool FAST>
  static __device__ __forceinline__ Pre<NFB> prefetch(const Args& args, int fw, int lane, int F) {
    const PosteriorArgs& a = post_base(args);
    Pre<NFB> r;
    const int h = lane >> 5;
    if constexpr (LINK) { r.bias[0][0] = make_float4(0.f, 0.f, 0.f, 0.f); return r; }
#pragma unroll
    for (int fb = 0; fb < NFB; ++fb)
#pragma unroll
      for (int q = 0; q < 4; ++q) r.bias[fb][q] = ldq<FAST>(a.bias, fw + 32 * fb + 8 * q + 4 * h, F);
    return r;
  }
  // LINK: a wave whose columns start below n_link (uniform) walks its tile with sigma on the unfolded x0 of the columns below n_link; every
  // other wave runs the walk of the form without a link, so the transcendentals are paid only where link columns are
  template <int NFB, int NPB, bool FAST>
  static __device__ __forceinline__ void apply(f32x16 (&acc)[NFB][NPB], const Args& args, const Pre<NFB>& pre, int fw, int pw, int lane, int F, int P) {
    if constexpr (LINK) {
      if (fw < post_n_link(args)) walk<NFB, NPB, FAST, true>(acc, args, pre, fw, pw, lane, F, P);
      else walk<NFB, NPB, FAST, false>(acc, args, pre, fw, pw, lane, F, P);
    } else walk<NFB, NPB, FAST, false>(acc, args, pre, fw, pw, lane, F, P);
  }
  // the quad walk.  LK: the link on the columns below n_link
  template <int NFB, int NPB, bool FAST, bool LK>
  static __device__ __forceinline__ void walk(f32x16 (&acc)[NFB][NPB], const Args& args, const Pre<NFB>& pre, int fw, int pw, int lane, int F, int P) {
    constexpr bool PLAIN = MODE == POST_PLAIN, CLIP = MODE == POST_CLIP, HIST = MODE == POST_HIST;
    constexpr bool ALL = post_quads_ahead(MODE, KNOWN) == 0;
    // LINK: the bias quad rides along with the x_t quads; clip then asks for one quad at a time (two still spill one VGPR)
    constexpr int QB = ALL ? 4 : (LINK && CLIP) ? 1 : post_quads_ahead(MODE, KNOWN);
    const PosteriorArgs& a = post_base(args);
    const int l31 = lane & 31, h = lane >> 5;
    const int t = a.t_dev ? *a.t_dev : a.t_imm;
    // the step's table rows (wave-uniform).  PLAIN: A, B, C;  CLIP: C and (P, Q, E, F);  HIST: (P, Q, G, F) and H
    float cA = 0.f, cB = 0.f, cC = 0.f, cP = 0.f, cQ = 0.f, cE = 0.f, cF = 0.f, cH = 0.f;
    if constexpr (PLAIN) {
      const float* c = a.coef + 4 * t;
      cA = c[0]; cB = c[1]; cC = c[2];
    } else {
      if constexpr (CLIP) cC = a.coef[4 * t + 2];
      const float* c = post_clip(args).x0coef + 4 * t;
      cP = c[0]; cQ = c[1]; cE = c[2]; cF = c[3];
      if constexpr (HIST) cH = post_hist(args).hcoef[t];
    }
    const bool hz = cH != 0.f;           // uniform: H = 0 skips the history read
    float La = 1.f, Ls = 0.f;
    if constexpr (KNOWN) { La = post_known(args).level[2 * t]; Ls = post_known(args).level[2 * t + 1]; }
    const bool cz = cC != 0.f;           // uniform: C = 0 draws no z for the free elements
    const float* zbase = a.z ? a.z + (long long)(a.t_first - t) * a.z_step_stride : nullptr;
    float4 xall[ALL ? NFB : 1][ALL ? NPB : 1][4];
    if constexpr (ALL) {
      OSD_FOR_QUADS(fb, pb, q) {
        const int p = pw + 32 * pb + l31;
        xall[fb][pb][q] = ldq<FAST>(a.xin + (size_t)(p < P ? p : P - 1) * a.ldx, fw + 32 * fb + 8 * q + 4 * h, F);
      }
    }
#pragma unroll
    for (int fb = 0; fb < NFB; ++fb)
#pragma unroll
      for (int pb = 0; pb < NPB; ++pb) {
        const int p = pw + 32 * pb + l31;
        const int pc = p < P ? p : P - 1;
        float* hrow = nullptr;
        if constexpr (HIST) hrow = post_hist(args).hist + (size_t)pc * post_hist(args).ldh;
        float4 xq[4], lq[4], hq[4], pq[4], kq[4], bq[4];
#pragma unroll
        for (int q0 = 0; q0 < 4; q0 += QB) {
          if constexpr (!ALL) {
#pragma unroll
            for (int q = q0; q < q0 + QB; ++q) {
              const int f = fw + 32 * fb + 8 * q + 4 * h;
              xq[q] = ldq<FAST>(a.xin + (size_t)pc * a.ldx, f, F);
              if constexpr (LINK) bq[q] = ldq<FAST>(a.bias, f, F);
              if constexpr (!PLAIN) {
                lq[q] = ldq<FAST>(post_clip(args).lo, f, F);
                hq[q] = ldq<FAST>(post_clip(args).hi, f, F);
              }
              if constexpr (HIST) {
                pq[q] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (hz) pq[q] = ldq<FAST>(hrow, f, F);
              }
              if constexpr (KNOWN) kq[q] = ldq<FAST>(post_known(args).known + (size_t)pc * post_known(args).ldk, f, F);
            }
          }
#pragma unroll
          for (int q = q0; q < q0 + QB; ++q) {
            const int f = fw + 32 * fb + 8 * q + 4 * h;
            const bool ok = p < P && f < F;
            float4 bv;
            if constexpr (LINK) bv = bq[q];
            else bv = pre.bias[fb][q];
            float4 x;
            if constexpr (ALL) x = xall[fb][pb][q];
            else x = xq[q];
            const float e[4] = {acc[fb][pb][4 * q] + bv.x, acc[fb][pb][4 * q + 1] + bv.y, acc[fb][pb][4 * q + 2] + bv.z, acc[fb][pb][4 * q + 3] + bv.w};
            const float xv[4] = {x.x, x.y, x.z, x.w};
            float kv[4] = {0.f, 0.f, 0.f, 0.f};
            // the draw rule.  C = 0 (eta = 0 DDIM steps; t = 0; HIST) draws nothing; the known elements use z at every t > 0, and a
            // quad without an observation skips the generator where C = 0.  cz is uniform: the step's table row
            bool draw = t > 0 && cz;
            if constexpr (KNOWN) {
              kv[0] = kq[q].x; kv[1] = kq[q].y; kv[2] = kq[q].z; kv[3] = kq[q].w;
              const bool any_known = kv[0] == kv[0] || kv[1] == kv[1] || kv[2] == kv[2] || kv[3] == kv[3];
              draw = t > 0 && (cz || any_known);
            }
            float4 zz = make_float4(0.f, 0.f, 0.f, 0.f);
            if (draw) {
              if (zbase) zz = ldq<FAST>(zbase + (size_t)pc * a.ldzz, f, F);
              else zz = randn4(a.seed, a.row_offset + (uint32_t)p, (uint32_t)(f >> 2), (uint32_t)t, TAG_POSTERIOR);
            }
            const float zv[4] = {zz.x, zz.y, zz.z, zz.w};
            float lv[4] = {0.f, 0.f, 0.f, 0.f}, hv[4] = {0.f, 0.f, 0.f, 0.f}, pv[4] = {0.f, 0.f, 0.f, 0.f};
            if constexpr (!PLAIN) {
              lv[0] = lq[q].x; lv[1] = lq[q].y; lv[2] = lq[q].z; lv[3] = lq[q].w;
              hv[0] = hq[q].x; hv[1] = hq[q].y; hv[2] = hq[q].z; hv[3] = hq[q].w;
            }
            if constexpr (HIST) { pv[0] = pq[q].x; pv[1] = pq[q].y; pv[2] = pq[q].z; pv[3] = pq[q].w; }
            float o[4], x0c[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              if constexpr (PLAIN && !KNOWN) o[r] = fmaf(cA, xv[r], fmaf(cB, e[r], cC * zv[r]));
              else if constexpr (PLAIN) o[r] = fmaf(cA, xv[r], fmaf(cB, e[r], cC * (cz ? zv[r] : 0.f)));
              else {
                float x0 = fmaf(cP, xv[r], cQ * e[r]);
                if constexpr (LK) x0 = f + r < post_n_link(args) ? link_sigmoid(x0) : x0;
                x0c[r] = fminf(fmaxf(x0, lv[r]), hv[r]);
                if constexpr (CLIP) o[r] = fmaf(cE, x0c[r], fmaf(cF, xv[r], cC * (cz ? zv[r] : 0.f)));
                else o[r] = fmaf(cE, x0c[r], fmaf(cF, xv[r], cH * pv[r]));      // cE holds G_t
              }
              if constexpr (KNOWN) {
                const float kn = t > 0 ? fmaf(La, kv[r], Ls * zv[r]) : kv[r];
                o[r] = (kv[r] == kv[r]) ? kn : o[r];      // NaN: free
              }
            }
            if (t == 0 && a.mut_mask && ok && f < a.mutation_dim) {
              float* mrow = a.mut_mask + (size_t)p * a.mutation_dim;
#pragma unroll
              for (int r = 0; r < 4; ++r)
                if (f + r < a.mutation_dim) mrow[f + r] = (o[r] > 0.5f) ? 1.0f : 0.0f;
            }
            if (p < P) stq<FAST>(a.xout + (size_t)pc * a.ldo, f, F, make_float4(o[0], o[1], o[2], o[3]));
            if constexpr (HIST)
              if (t > 0 && p < P) stq<FAST>(hrow, f, F, make_float4(x0c[0], x0c[1], x0c[2], x0c[3]));
          }
        }
      }
  }
};

// ---- output_proj fused with the MSE loss (models/diffusion.py:373-377) and its gradient ----
// d = (acc + bias) - noise;  loss += sum d^2 * inv_count;  dout = d * gscale
struct EpiMse {
  static constexpr bool COUNTED_STORES = false;   // dout / pred are optional
  static constexpr bool XBUF = true;              // the noise target comes in, dL/d eps goes out, as full row segments
  template <class A> static __device__ __forceinline__ void slice(A&, int) {}
  struct Args {
    const float* bias; const float* noise; int ldn;
    float* dout; int ldd;         // may be null (validation: loss only)
    float* pred; int ldp;         // may be null
    float* loss;                  // dev float[1], atomically accumulated
    float inv_count; float gscale;
  };
  static bool fast_ok(const Args& a, int F) {
    return F % 4 == 0 && al16(a.bias) && al16(a.noise) && a.ldn % 4 == 0 && (!a.dout || (al16(a.dout) && a.ldd % 4 == 0)) &&
           (!a.pred || (al16(a.pred) && a.ldp % 4 == 0));
  }
  template <int NFB> struct Pre { float4 bias[NFB][4]; };
  template <int NFB, bool FAST>
  static __device__ __forceinline__ Pre<NFB> prefetch(const Args& a, int fw, int lane, int F) {
    Pre<NFB> r;
    const int h = lane >> 5;
#pragma unroll
    for (int fb = 0; fb < NFB; ++fb)
#pragma unroll
      for (int q = 0; q < 4; ++q) r.bias[fb][q] = ldq<FAST>(a.bias, fw + 32 * fb + 8 * q + 4 * h, F);
    return r;
  }
  // xbuf (FAST only): the wave's transposer region; the 32-feature blocks of the noise target are read, and those of dL/d eps
  // written, as full 128-byte row segments (xpose.h) instead of 32 rows x 32 bytes per wave-instruction
  template <int NFB, int NPB, bool FAST>
  static __device__ __forceinline__ void apply(f32x16 (&acc)[NFB][NPB], const Args& a, const Pre<NFB>& pre, int fw, int pw, int lane, int F, int P,
                                               float* xbuf = nullptr) {
    const int l31 = lane & 31, h = lane >> 5;
    float part = 0.f;
    if (FAST && xbuf) {
      const WaveXpose<NPB> xp{xbuf};
      const int rows = P - pw;                         // valid rows of the wave's block (uniform)
#pragma unroll
      for (int fb = 0; fb < NFB; ++fb) {
        const int cols = F - (fw + 32 * fb);            // valid features of this block (uniform)
        if (rows <= 0 || cols <= 0) continue;
        xp.template load_rows<true>(a.noise + (size_t)pw * a.ldn + fw + 32 * fb, a.ldn, lane, rows, cols);
#pragma unroll
        for (int pb = 0; pb < NPB; ++pb)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int fo = 8 * q + 4 * h;
            const int p = 32 * pb + l31;
            const bool prow = p < rows;
            const float4 bv = pre.bias[fb][q];
            const float4 nz = xp.get(pb, q, l31, h);
            const float4 e = make_float4(acc[fb][pb][4 * q] + bv.x, acc[fb][pb][4 * q + 1] + bv.y, acc[fb][pb][4 * q + 2] + bv.z, acc[fb][pb][4 * q + 3] + bv.w);
            if (a.pred && prow) stq<FAST>(a.pred + (size_t)(pw + p) * a.ldp, fw + 32 * fb + fo, F, e);
            float4 d = make_float4(e.x - nz.x, e.y - nz.y, e.z - nz.z, e.w - nz.w);
            if (!prow || fo >= cols) d.x = 0.f;
            if (!prow || fo + 1 >= cols) d.y = 0.f;
            if (!prow || fo + 2 >= cols) d.z = 0.f;
            if (!prow || fo + 3 >= cols) d.w = 0.f;
            part += d.x * d.x + d.y * d.y + d.z * d.z + d.w * d.w;
            xp.put(pb, q, l31, h, make_float4(d.x * a.gscale, d.y * a.gscale, d.z * a.gscale, d.w * a.gscale));
          }
        if (a.dout) xp.template store_rows<true>(a.dout + (size_t)pw * a.ldd + fw + 32 * fb, a.ldd, lane, rows, cols);
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o);
      // one atomic per workgroup (the four waves meet in LDS): same-address float atomics serialise in L2
      __shared__ float wave_part[4];               // 16 bytes: keeps the dynamic LDS base 16-byte aligned
      const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
      if (lane == 0) wave_part[wv] = part;
      __syncthreads();
      if (threadIdx.x == 0) atomicAdd(a.loss, ((wave_part[0] + wave_part[1]) + (wave_part[2] + wave_part[3])) * a.inv_count);
      return;
    }
    OSD_FOR_QUADS(fb, pb, q) {
      const int f = fw + 32 * fb + 8 * q + 4 * h;
      const int p = pw + 32 * pb + l31;
      const int pc = p < P ? p : P - 1;
      const bool prow = p < P;
      const float4 bv = pre.bias[fb][q];
      const float4 nz = ldq<FAST>(a.noise + (size_t)pc * a.ldn, f, F);
      const float4 e = make_float4(acc[fb][pb][4 * q] + bv.x, acc[fb][pb][4 * q + 1] + bv.y, acc[fb][pb][4 * q + 2] + bv.z, acc[fb][pb][4 * q + 3] + bv.w);
      if (a.pred && prow) stq<FAST>(a.pred + (size_t)p * a.ldp, f, F, e);
      float4 d = make_float4(e.x - nz.x, e.y - nz.y, e.z - nz.z, e.w - nz.w);
      if (!prow || f >= F) d.x = 0.f;
      if (!prow || f + 1 >= F) d.y = 0.f;
      if (!prow || f + 2 >= F) d.z = 0.f;
      if (!prow || f + 3 >= F) d.w = 0.f;
      part += d.x * d.x + d.y * d.y + d.z * d.z + d.w * d.w;
      if (a.dout && prow) stq<FAST>(a.dout + (size_t)p * a.ldd, f, F, make_float4(d.x * a.gscale, d.y * a.gscale, d.z * a.gscale, d.w * a.gscale));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o);
    if (lane == 0) atomicAdd(a.loss, part * a.inv_count);
  }
};

// ---- output_proj fused with a configurable eps-loss (osd_set_loss) and its gradient ----
// d = (acc + bias) - noise;  loss += w[t_row] * sum rho(d) * inv_count;  dout = w[t_row] * rho'(d) * gscale
//   kind 0 (l2):     rho = d^2                                         rho' = d               (the host folds the 2 into gscale, as EpiMse)
//   kind 1 (l1):     rho = |d|                                         rho' = sign(d), 0 at 0
//   kind 2 (huber):  rho = 1/2 d^2 if |d| <= delta else delta (|d| - 1/2 delta)   rho' = clamp(d, -delta, delta)
// w = tw[t_index[row]] (one gathered load per row) or 1 when tw is null.  kind is uniform over the launch: a scalar branch around a
// handful of VALU operations per element (tile loops compiled per kind behind one branch were tried: the 128 x 128 LDS-DMA kernel then
// spills 22 VGPRs).  EpiMse's structure otherwise, path for path: the transposer on full row segments when
// FAST, the guarded form elsewhere; padding rows and columns carry d = 0, and rho(0) = rho'(0) = 0 for every kind; one reduction
// per workgroup and one float atomic on the transposer path.
// MASKED (osd_set_loss_mask): a NaN component of the target means "not observed" (k_elem.hip: mask_mark);
// its d is zeroed right after d = e - nz, so it adds rho(0) = 0 to the loss and rho'(0) = 0 to dout -- one compare and one select
// per element, nothing held across the tile.  pred is not written (only the constraint losses read it, and they are refused).
//
// LINK (osd_set_output_link): columns f < n_link are logits of a Bernoulli mean and carry cross-entropy
// instead of rho.  With o = acc + bias and y the target (x0 under OSD_PRED_SAMPLE; inside [0, 1] after a mixup):
//   rho = max(o, 0) - o y + log1p(exp(-|o|))                 d rho / d o = sigma(o) - y = (1 - y) sigma(o) - y sigma(-o)
// from one hardware exp2 (e = exp(-|o|)), one log2 and one rcp per element; the last form has no cancellation at a confident right
// call.  rho(0) = ln 2, so the padding invariant above does not hold in these columns: an element enters the sum and dout only when
// its row < P, its column < F and its target is not NaN (the link form always treats NaN as "not observed": it is the masked form
// too), by an explicit select.  The host folds l2's 2 into gscale; the link columns take it out again (x 0.5, exact).  A 32-column
// block that starts at or past n_link (wave-uniform) runs the code of the form without a link, so the transcendentals are paid only
// where link columns are; a block that holds the boundary selects per element.  pred is not written.
template <bool LINK> struct LossArgsT;
template <> struct LossArgsT<false> {
  EpiMse::Args m;               // bias, noise, dout, pred, loss, inv_count, gscale: EpiMse's meaning
  const float* tw;              // dev [T] per-timestep weights, or null (every row weighs 1)
  const int* t_index;           // dev [P] timestep index of each row, in [0, T); read only when tw is non-null
  int kind; float delta;
};
template <> struct LossArgsT<true> : LossArgsT<false> { int n_link; };   // columns [0, n_link) carry the logistic link
template <bool MASKED, bool LINK = false>
struct EpiLossT {
  static_assert(!LINK || MASKED, "the link form is the masked form as well");
  static constexpr bool COUNTED_STORES = false;   // dout / pred are optional
  static constexpr bool XBUF = true;
  template <class A> static __device__ __forceinline__ void slice(A&, int) {}
  typedef LossArgsT<LINK> Args;
  static bool fast_ok(const Args& a, int F) { return EpiMse::fast_ok(a.m, F); }
  template <int NFB> using Pre = EpiMse::Pre<NFB>;
  template <int NFB, bool FAST>
  static __device__ __forceinline__ Pre<NFB> prefetch(const Args& a, int fw, int lane, int F) {
    return EpiMse::prefetch<NFB, FAST>(a.m, fw, lane, F);
  }
  // LINK: one element of a block that holds link columns.  o the logit (or the output), y the target, link: f < n_link, ok: the element
  // exists and is observed.  Returns the scaled dout; adds the unweighted rho to q
  static __device__ __forceinline__ float link_point(int kind, float delta, float wg, float wgl, float o, float y, bool link, bool ok, float& q) {
    if (link) {
      const float e = __builtin_amdgcn_exp2f(fabsf(o) * -1.4426950408889634f);
      const float r = __builtin_amdgcn_rcpf(1.0f + e);
      const float er = e * r;
      const float sp = o >= 0.f ? r : er, sn = o >= 0.f ? er : r;        // sigma(o), sigma(-o)
      const float rho = fmaf(-o, y, fmaxf(o, 0.f)) + 0.6931471805599453f * __builtin_amdgcn_logf(1.0f + e);
      q += ok ? rho : 0.f;
      return ok ? ((1.0f - y) * sp - y * sn) * wgl : 0.f;
    }
    float d = ok ? o - y : 0.f;
    point(kind, delta, d, q);
    return d * wg;
  }
  // ... and one quad of it: e the outputs, nz the targets, f the quad's first column, cols / prow what exists
  static __device__ __forceinline__ float4 link_quad(int kind, float delta, float w, float gs, int n_link, int f, int fo, int cols, bool prow,
                                                     const float4& e, const float4& nz, float& part) {
    const float wg = w * gs, wgl = w * (kind == 0 ? 0.5f * gs : gs);
    float q = 0.f;
    float4 d;
    d.x = link_point(kind, delta, wg, wgl, e.x, nz.x, f < n_link, prow && fo < cols && nz.x == nz.x, q);
    d.y = link_point(kind, delta, wg, wgl, e.y, nz.y, f + 1 < n_link, prow && fo + 1 < cols && nz.y == nz.y, q);
    d.z = link_point(kind, delta, wg, wgl, e.z, nz.z, f + 2 < n_link, prow && fo + 2 < cols && nz.z == nz.z, q);
    d.w = link_point(kind, delta, wg, wgl, e.w, nz.w, f + 3 < n_link, prow && fo + 3 < cols && nz.w == nz.w, q);
    part += w * q;
    return d;
  }
  // rho(d) into `part`, rho'(d) back into d; d = 0 gives 0 and 0
  static __device__ __forceinline__ void point(int kind, float delta, float& d, float& part) {
    const float ad = fabsf(d);
    if (kind == 0) {
      part += d * d;
    } else if (kind == 1) {
      part += ad;
      d = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
    } else {
      const float c = fminf(ad, delta);
      part += c * (ad - 0.5f * c);
      d = fminf(fmaxf(d, -delta), delta);
    }
  }
  // (rho' * w) * gscale per element rather than a per-row w * gscale kept next to w: the 128 x 128 LDS-DMA tile has no register to spare
  static __device__ __forceinline__ void quad(int kind, float delta, float w, float gs, float4& d, float& part) {
    float q = 0.f;
    point(kind, delta, d.x, q); point(kind, delta, d.y, q); point(kind, delta, d.z, q); point(kind, delta, d.w, q);
    part += w * q;
    d.x = d.x * w * gs; d.y = d.y * w * gs; d.z = d.z * w * gs; d.w = d.w * w * gs;
  }
  // MASKED: d = 0 where the target component is NaN
  static __device__ __forceinline__ void unobserved(const float4& nz, float4& d) {
    d.x = nz.x != nz.x ? 0.f : d.x; d.y = nz.y != nz.y ? 0.f : d.y; d.z = nz.z != nz.z ? 0.f : d.z; d.w = nz.w != nz.w ? 0.f : d.w;
  }
  template <int NFB, int NPB, bool FAST>
  static __device__ __forceinline__ void apply(f32x16 (&acc)[NFB][NPB], const Args& al, const Pre<NFB>& pre, int fw, int pw, int lane, int F, int P,
                                               float* xbuf = nullptr) {
    const EpiMse::Args& a = al.m;
    const int l31 = lane & 31, h = lane >> 5;
    const int kind = al.kind;
    const float delta = al.delta;
    float wrow[NPB];
#pragma unroll
    for (int pb = 0; pb < NPB; ++pb) {
      const int p = pw + 32 * pb + l31;
      wrow[pb] = al.tw ? al.tw[al.t_index[p < P ? p : P - 1]] : 1.0f;
    }
    float part = 0.f;
    if (FAST && xbuf) {
      const WaveXpose<NPB> xp{xbuf};
      const int rows = P - pw;                         // valid rows of the wave's block (uniform)
#pragma unroll
      for (int fb = 0; fb < NFB; ++fb) {
        const int cols = F - (fw + 32 * fb);            // valid features of this block (uniform)
        if (rows <= 0 || cols <= 0) continue;
        xp.template load_rows<true>(a.noise + (size_t)pw * a.ldn + fw + 32 * fb, a.ldn, lane, rows, cols);
#pragma unroll
        for (int pb = 0; pb < NPB; ++pb)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int fo = 8 * q + 4 * h;
            const int p = 32 * pb + l31;
            const bool prow = p < rows;
            const float4 bv = pre.bias[fb][q];
            const float4 nz = xp.get(pb, q, l31, h);
            const float4 e = make_float4(acc[fb][pb][4 * q] + bv.x, acc[fb][pb][4 * q + 1] + bv.y, acc[fb][pb][4 * q + 2] + bv.z, acc[fb][pb][4 * q + 3] + bv.w);
            if constexpr (!MASKED)
              if (a.pred && prow) stq<FAST>(a.pred + (size_t)(pw + p) * a.ldp, fw + 32 * fb + fo, F, e);
            if constexpr (LINK) {
              if (fw + 32 * fb < al.n_link) {          // uniform: the block holds link columns
                xp.put(pb, q, l31, h, link_quad(kind, delta, wrow[pb], a.gscale, al.n_link, fw + 32 * fb + fo, fo, cols, prow, e, nz, part));
                continue;
              }
            }
            float4 d = make_float4(e.x - nz.x, e.y - nz.y, e.z - nz.z, e.w - nz.w);
            if constexpr (MASKED) unobserved(nz, d);
            if (!prow || fo >= cols) d.x = 0.f;
            if (!prow || fo + 1 >= cols) d.y = 0.f;
            if (!prow || fo + 2 >= cols) d.z = 0.f;
            if (!prow || fo + 3 >= cols) d.w = 0.f;
            quad(kind, delta, wrow[pb], a.gscale, d, part);
            xp.put(pb, q, l31, h, d);
          }
        if (a.dout) xp.template store_rows<true>(a.dout + (size_t)pw * a.ldd + fw + 32 * fb, a.ldd, lane, rows, cols);
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o);
      // one atomic per workgroup, as EpiMse
      __shared__ float wave_part[4];               // 16 bytes: keeps the dynamic LDS base 16-byte aligned
      const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
      if (lane == 0) wave_part[wv] = part;
      __syncthreads();
      if (threadIdx.x == 0) atomicAdd(a.loss, ((wave_part[0] + wave_part[1]) + (wave_part[2] + wave_part[3])) * a.inv_count);
      return;
    }
    OSD_FOR_QUADS(fb, pb, q) {
      const int f = fw + 32 * fb + 8 * q + 4 * h;
      const int p = pw + 32 * pb + l31;
      const int pc = p < P ? p : P - 1;
      const bool prow = p < P;
      const float4 bv = pre.bias[fb][q];
      const float4 nz = ldq<FAST>(a.noise + (size_t)pc * a.ldn, f, F);
      const float4 e = make_float4(acc[fb][pb][4 * q] + bv.x, acc[fb][pb][4 * q + 1] + bv.y, acc[fb][pb][4 * q + 2] + bv.z, acc[fb][pb][4 * q + 3] + bv.w);
      if constexpr (!MASKED)
        if (a.pred && prow) stq<FAST>(a.pred + (size_t)p * a.ldp, f, F, e);
      if constexpr (LINK) {
        if (fw + 32 * fb < al.n_link) {          // uniform: the block holds link columns
          const float4 dl = link_quad(kind, delta, wrow[pb], a.gscale, al.n_link, f, f, F, prow, e, nz, part);
          if (a.dout && prow) stq<FAST>(a.dout + (size_t)p * a.ldd, f, F, dl);
          continue;
        }
      }
      float4 d = make_float4(e.x - nz.x, e.y - nz.y, e.z - nz.z, e.w - nz.w);
      if constexpr (MASKED) unobserved(nz, d);
      if (!prow || f >= F) d.x = 0.f;
      if (!prow || f + 1 >= F) d.y = 0.f;
      if (!prow || f + 2 >= F) d.z = 0.f;
      if (!prow || f + 3 >= F) d.w = 0.f;
      quad(kind, delta, wrow[pb], a.gscale, d, part);
      if (a.dout && prow) stq<FAST>(a.dout + (size_t)p * a.ldd, f, F, d);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o);
    if (lane == 0) atomicAdd(a.loss, part * a.inv_count);
  }
};
using EpiLoss = EpiLossT<false>;

// ---- output_proj fused with a PER-ROW squared error against the training target ----
// d = (acc + bias) - target;  part[slot][row] = sum over the wave's features of d^2
// EpiMse's operand paths, path for path -- the transposer on full row segments when FAST, the guarded form elsewhere; padding rows
// and columns carry d = 0 -- without pred, dout or a scalar loss.  No float atomics: a lane holds one row (l31) of each 32-row
// block and a slice of its features, sums them in-lane over fb and q in that order, and meets the other half-wave once (lane^32:
// the sum of the two halves is commutative, so both lanes form the same bits).  The wave's (slot, row) partials -- slot = the wave's
// feature origin / its feature extent, one wave per (slot, row) in the whole grid -- go to part [slots][ld] with ordinary stores, 32
// consecutive floats per instruction; k_rowsq_reduce adds the slots of a row in slot order.  Equal inputs give equal bits.
// Nothing needs zeroing: every (slot < ceil(F / extent), row < P) element is written exactly once per launch.
struct EpiRowSq {
  static constexpr bool COUNTED_STORES = false;   // one store per row and wave, not per accumulator quad
  static constexpr bool XBUF = true;              // the target comes in as full row segments
  template <class A> static __device__ __forceinline__ void slice(A&, int) {}
  struct Args {
    const float* bias; const float* target; int ldn;
    float* part; long long ld;    // [slots][ld], ld >= P
  };
  static bool fast_ok(const Args& a, int F) { return F % 4 == 0 && al16(a.bias) && al16(a.target) && a.ldn % 4 == 0; }
  template <int NFB> using Pre = EpiMse::Pre<NFB>;
  template <int NFB, bool FAST>
  static __device__ __forceinline__ Pre<NFB> prefetch(const Args& a, int fw, int lane, int F) {
    Pre<NFB> r;
    const int h = lane >> 5;
#pragma unroll
    for (int fb = 0; fb < NFB; ++fb)
#pragma unroll
      for (int q = 0; q < 4; ++q) r.bias[fb][q] = ldq<FAST>(a.bias, fw + 32 * fb + 8 * q + 4 * h, F);
    return r;
  }
  template <int NFB, int NPB, bool FAST>
  static __device__ __forceinline__ void apply(f32x16 (&acc)[NFB][NPB], const Args& a, const Pre<NFB>& pre, int fw, int pw, int lane, int F, int P,
                                               float* xbuf = nullptr) {
    const int l31 = lane & 31, h = lane >> 5;
    if (fw >= F || pw >= P) return;                    // uniform over the wave: a slot past the last one, or padding rows only
    float part[NPB];
#pragma unroll
    for (int pb = 0; pb < NPB; ++pb) part[pb] = 0.f;
    if (FAST && xbuf) {
      const WaveXpose<NPB> xp{xbuf};
      const int rows = P - pw;                         // valid rows of the wave's block (uniform)
#pragma unroll
      for (int fb = 0; fb < NFB; ++fb) {
        const int cols = F - (fw + 32 * fb);            // valid features of this block (uniform)
        if (cols <= 0) continue;
        xp.template load_rows<true>(a.target + (size_t)pw * a.ldn + fw + 32 * fb, a.ldn, lane, rows, cols);
#pragma unroll
        for (int pb = 0; pb < NPB; ++pb)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int fo = 8 * q + 4 * h;
            const bool prow = 32 * pb + l31 < rows;
            const float4 bv = pre.bias[fb][q];
            const float4 nz = xp.get(pb, q, l31, h);
            float4 d = make_float4((acc[fb][pb][4 * q] + bv.x) - nz.x, (acc[fb][pb][4 * q + 1] + bv.y) - nz.y,
                                   (acc[fb][pb][4 * q + 2] + bv.z) - nz.z, (acc[fb][pb][4 * q + 3] + bv.w) - nz.w);
            if (!prow || fo >= cols) d.x = 0.f;
            if (!prow || fo + 1 >= cols) d.y = 0.f;
            if (!prow || fo + 2 >= cols) d.z = 0.f;
            if (!prow || fo + 3 >= cols) d.w = 0.f;
            part[pb] += d.x * d.x + d.y * d.y + d.z * d.z + d.w * d.w;
          }
      }
    } else {
      OSD_FOR_QUADS(fb, pb, q) {
        const int f = fw + 32 * fb + 8 * q + 4 * h;
        const int p = pw + 32 * pb + l31;
        const int pc = p < P ? p : P - 1;
        const bool prow = p < P;
        const float4 bv = pre.bias[fb][q];
        const float4 nz = ldq<FAST>(a.target + (size_t)pc * a.ldn, f, F);
        float4 d = make_float4((acc[fb][pb][4 * q] + bv.x) - nz.x, (acc[fb][pb][4 * q + 1] + bv.y) - nz.y,
                               (acc[fb][pb][4 * q + 2] + bv.z) - nz.z, (acc[fb][pb][4 * q + 3] + bv.w) - nz.w);
        if (!prow || f >= F) d.x = 0.f;
        if (!prow || f + 1 >= F) d.y = 0.f;
        if (!prow || f + 2 >= F) d.z = 0.f;
        if (!prow || f + 3 >= F) d.w = 0.f;
        part[pb] += d.x * d.x + d.y * d.y + d.z * d.z + d.w * d.w;
      }
    }
    float* slot = a.part + (long long)(fw / (32 * NFB)) * a.ld;
#pragma unroll
    for (int pb = 0; pb < NPB; ++pb) {
      const float s = part[pb] + swap_halves(part[pb]);
      const int p = pw + 32 * pb + l31;
      if (h == 0 && p < P) slot[p] = s;
    }
  }
};

// ---- output_proj fused with the noise map's solve (osd_noise_map) ----
// Row p of the launch is a (level s, patient i) pair with s > 0.  The chain's step at that level is x' = fmaf(A, y, fmaf(B, out, C z))
// (EpiPosterior<POST_PLAIN>); the map wants the z that makes x' the state y_{s-1}, and takes the step's operations back outermost first:
//   u = fmaf(-A, y_s, y_{s-1})        formed by k_q_sample_map, streamed in where the loss epilogues stream the target
//   z = fmaf(-B, acc + bias, u) / C   here; 1 / C is a correctly rounded per-row reciprocal (k_q_sample_map), the divide a product
// z goes straight to noises_out at the row's own offset (row[p].zoff: level-major in the chain's draw order, so rows of one launch are
// not one stride apart) in place of dL/dout; neither the network output nor a posterior mean is written.  EpiMse's operand paths, path
// for path: the transposer on full row segments when FAST, the guarded form elsewhere.  No atomics, no reduction: a row's z depends on
// the row alone.
struct MapRow { float B, invC; long long zoff; };      // 16 bytes
struct EpiNoiseMap {
  static constexpr bool COUNTED_STORES = false;   // rows beyond P store nothing
  static constexpr bool XBUF = true;              // u comes in, z goes out, as full row segments
  template <class A> static __device__ __forceinline__ void slice(A&, int) {}
  struct Args {
    const float* bias; const float* target; int ldn;
    const MapRow* row;            // dev [P]
    float* z;                     // noises_out
  };
  static bool fast_ok(const Args& a, int F) { return F % 4 == 0 && al16(a.bias) && al16(a.target) && a.ldn % 4 == 0 && al16(a.z); }
  template <int NFB> using Pre = EpiMse::Pre<NFB>;
  template <int NFB, bool FAST>
  static __device__ __forceinline__ Pre<NFB> prefetch(const Args& a, int fw, int lane, int F) {
    Pre<NFB> r;
    const int h = lane >> 5;
#pragma unroll
    for (int fb = 0; fb < NFB; ++fb)
#pragma unroll
      for (int q = 0; q < 4; ++q) r.bias[fb][q] = ldq<FAST>(a.bias, fw + 32 * fb + 8 * q + 4 * h, F);
    return r;
  }
  // explicit operations: both operand paths and both tiles form the same bits whatever the compiler would contract
  static __device__ __forceinline__ float4 solve(const float4& e, const float4& u, float nB, float iC) {
    return make_float4(__fmul_rn(fmaf(nB, e.x, u.x), iC), __fmul_rn(fmaf(nB, e.y, u.y), iC), __fmul_rn(fmaf(nB, e.z, u.z), iC),
                       __fmul_rn(fmaf(nB, e.w, u.w), iC));
  }
  template <int NFB, int NPB, bool FAST>
  static __device__ __forceinline__ void apply(f32x16 (&acc)[NFB][NPB], const Args& a, const Pre<NFB>& pre, int fw, int pw, int lane, int F, int P,
                                               float* xbuf = nullptr) {
    const int l31 = lane & 31, h = lane >> 5;
    if (fw >= F || pw >= P) return;                    // uniform over the wave
    float nB[NPB], iC[NPB];
    long long zo[NPB];
#pragma unroll
    for (int pb = 0; pb < NPB; ++pb) {
      const int p = pw + 32 * pb + l31;
      const MapRow r = a.row[p < P ? p : P - 1];
      nB[pb] = -r.B; iC[pb] = r.invC; zo[pb] = r.zoff;
    }
    if (FAST && xbuf) {
      const WaveXpose<NPB> xp{xbuf};
      const int rows = P - pw;                         // valid rows of the wave's block (uniform)
      const MapRow* const wrow = a.row + pw;
#pragma unroll
      for (int fb = 0; fb < NFB; ++fb) {
        const int cols = F - (fw + 32 * fb);            // valid features of this block (uniform)
        if (cols <= 0) continue;
        xp.template load_rows<true>(a.target + (size_t)pw * a.ldn + fw + 32 * fb, a.ldn, lane, rows, cols);
#pragma unroll
        for (int pb = 0; pb < NPB; ++pb)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float4 bv = pre.bias[fb][q];
            const float4 u = xp.get(pb, q, l31, h);
            const float4 e = make_float4(acc[fb][pb][4 * q] + bv.x, acc[fb][pb][4 * q + 1] + bv.y, acc[fb][pb][4 * q + 2] + bv.z, acc[fb][pb][4 * q + 3] + bv.w);
            xp.put(pb, q, l31, h, solve(e, u, nB[pb], iC[pb]));
          }
        xp.store_rows_at(a.z + fw + 32 * fb, [wrow](int k) { return wrow[k].zoff; }, lane, rows < 32 * NPB ? rows : 32 * NPB, cols);
      }
      return;
    }
    OSD_FOR_QUADS(fb, pb, q) {
      const int f = fw + 32 * fb + 8 * q + 4 * h;
      const int p = pw + 32 * pb + l31;
      const int pc = p < P ? p : P - 1;
      const float4 bv = pre.bias[fb][q];
      const float4 u = ldq<FAST>(a.target + (size_t)pc * a.ldn, f, F);
      const float4 e = make_float4(acc[fb][pb][4 * q] + bv.x, acc[fb][pb][4 * q + 1] + bv.y, acc[fb][pb][4 * q + 2] + bv.z, acc[fb][pb][4 * q + 3] + bv.w);
      if (p < P) stq<FAST>(a.z + zo[pb], f, F, solve(e, u, nB[pb], iC[pb]));
    }
  }
};

// ---- what the four Gram-distance epilogues below share ---------------------------------------------------------------------
// A = the tile's feature side (rows f), B = its patient side (rows p); acc = a_f . b_p.  The squared norms of the A rows ride in
// registers from before the K loop, the layout of the accumulator quads: sq[fb][q] holds rows fw + 32 fb + 8 q + 4 h .. + 3.
template <int NFB> struct GramNorms { float4 sq[NFB][4]; };
template <int NFB, bool FAST>
__device__ __forceinline__ GramNorms<NFB> gram_norms(const float* sq, int fw, int lane, int F) {
  GramNorms<NFB> r;
  const int h = lane >> 5;
#pragma unroll
  for (int fb = 0; fb < NFB; ++fb)
#pragma unroll
    for (int q = 0; q < 4; ++q) r.sq[fb][q] = ldq<FAST>(sq, fw + 32 * fb + 8 * q + 4 * h, F);
  return r;
}
// the expanded squared distance |a|^2 + |b|^2 - 2 a.b, clamped at 0 (it cancels for near copies: callers that report a distance
// recompute it, k_knn_refine)
__device__ __forceinline__ float gram_d2(float sa, float sb, float acc) { return fmaxf(sa + sb - 2.0f * acc, 0.f); }
// FAST reads the A-side norms as aligned quads
inline bool gram_fast_ok(const float* sq, int F) { return F % 4 == 0 && al16(sq); }

// ---- RBF-kernel sum for the MMD metric (utils/validation.py:287-296) -------------------------------
// acc = x_f . y_p;  d2 = |x_f|^2 + |y_p|^2 - 2 acc;  sum += exp(-gamma * max(d2, 0)) over the valid tile
struct EpiRbfSum {
  static constexpr bool COUNTED_STORES = false;   // stores nothing
  static constexpr bool XBUF = false;
  template <class A> static __device__ __forceinline__ void slice(A&, int) {}
  // sum: RBF_SLOTS doubles; a workgroup adds into slot blockIdx.x % RBF_SLOTS (same-address atomics serialise in L2: 153 000
  // tiles of a 50 000 x 50 000 block on ONE address cost ~2 % of the kernel), the host adds the slots up
  static constexpr int RBF_SLOTS = 256;
  // tri: the product is symmetric and only tiles with feature tile <= patient tile run (GemmArgs::tri, 128 x 128 tiles): a tile
  // strictly above the diagonal stands for its mirror image too and counts twice; the diagonal tiles are computed whole
  // (utils/validation.py:286-296 sums the full matrix, diagonal included)
  struct Args { const float* sqa; const float* sqb; float gamma; double* sum; int tri; };
  static bool fast_ok(const Args& a, int F) { return gram_fast_ok(a.sqa, F); }
  template <int NFB> using Pre = GramNorms<NFB>;
  template <int NFB, bool FAST>
  static __device__ __forceinline__ Pre<NFB> prefetch(const Args& a, int fw, int lane, int F) { return gram_norms<NFB, FAST>(a.sqa, fw, lane, F); }
  template <int NFB, int NPB, bool FAST>
  static __device__ __forceinline__ void apply(f32x16 (&acc)[NFB][NPB], const Args& a, const Pre<NFB>& pre, int fw, int pw, int lane, int F, int P) {
    const int l31 = lane & 31, h = lane >> 5;
    float part = 0.f;
#pragma unroll
    for (int pb = 0; pb < NPB; ++pb) {
      const int p = pw + 32 * pb + l31;
      const float sb = a.sqb[p < P ? p : P - 1];
#pragma unroll
      for (int fb = 0; fb < NFB; ++fb)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int f = fw + 32 * fb + 8 * q + 4 * h;
          const float4 sa = pre.sq[fb][q];
          const float sav[4] = {sa.x, sa.y, sa.z, sa.w};
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float d2 = gram_d2(sav[r], sb, acc[fb][pb][4 * q + r]);
            const float k = expf(-a.gamma * d2);
            part += (p < P && f + r < F) ? k : 0.f;
          }
        }
    }
    double dp = (double)part;
    if (a.tri && (fw >> 7) < (pw >> 7)) dp *= 2.0;       // uniform over the workgroup
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) dp += __shfl_xor(dp, o);
    // one atomic per workgroup: a 50 000 x 50 000 Gram block is 153 000 tiles, and same-address atomics serialise in L2
    __shared__ double wave_sum[4];                 // 32 bytes: the dynamic LDS base stays 16-byte aligned
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (lane == 0) wave_sum[wv] = dp;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(a.sum + (blockIdx.x % RBF_SLOTS), (wave_sum[0] + wave_sum[1]) + (wave_sum[2] + wave_sum[3]));
  }
};

// ---- nearest reference row of every query row (the privacy audit) ----------------------------
// A = reference rows (the tile's feature side, f), B = query rows (the patient side, p).  acc = r_f . q_p;
// d2 = max(|r_f|^2 + |q_p|^2 - 2 acc, 0).  Per query the minimum of the unsigned 64-bit key (float_bits(d2) << 32) | f is kept:
// bits of non-negative floats order like the floats, so the minimum key is the minimum distance and ties go to the smallest
// index -- whatever order the workgroups finish in.  f >= F, p >= P and f == exclude[p] never enter.  A lane holds one query and
// 16 * NFB reference rows in increasing f: the running minimum is a 32-bit compare on the distance bits (strict, so the first --
// smallest -- f of a tie stays); the two half-waves that share a query meet through lane^32, and one 64-bit atomicMin per query
// and wave goes out, skipped when the key already stored is not larger (a stale read only costs the atomic it failed to skip).
struct EpiNearest {
  static constexpr bool COUNTED_STORES = false;   // stores nothing but the atomics
  static constexpr bool XBUF = false;
  static constexpr unsigned long long NO_KEY = ~0ull;   // the key array's initial value: no candidate
  template <class A> static __device__ __forceinline__ void slice(A&, int) {}
  struct Args { const float* sqr; const float* sqq; const int* exclude; unsigned long long* keys; };
  static bool fast_ok(const Args& a, int F) { return gram_fast_ok(a.sqr, F); }
  template <int NFB> using Pre = GramNorms<NFB>;
  template <int NFB, bool FAST>
  static __device__ __forceinline__ Pre<NFB> prefetch(const Args& a, int fw, int lane, int F) { return gram_norms<NFB, FAST>(a.sqr, fw, lane, F); }
  template <int NFB, int NPB, bool FAST>
  static __device__ __forceinline__ void apply(f32x16 (&acc)[NFB][NPB], const Args& a, const Pre<NFB>& pre, int fw, int pw, int lane, int F, int P) {
    const int l31 = lane & 31, h = lane >> 5;
#pragma unroll
    for (int pb = 0; pb < NPB; ++pb) {
      const int p = pw + 32 * pb + l31;
      const int pc = p < P ? p : P - 1;
      const float sq = a.sqq[pc];
      const int ex = a.exclude ? a.exclude[pc] : -1;
      unsigned best = 0xffffffffu;                 // above the bits of every non-negative float, +inf included
      int best_f = 0;
#pragma unroll
      for (int fb = 0; fb < NFB; ++fb)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int f = fw + 32 * fb + 8 * q + 4 * h;
          const float4 sr = pre.sq[fb][q];
          const float srv[4] = {sr.x, sr.y, sr.z, sr.w};
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float d2 = gram_d2(srv[r], sq, acc[fb][pb][4 * q + r]);
            const unsigned bits = (f + r < F && f + r != ex) ? __float_as_uint(d2) : 0xffffffffu;
            if (bits < best) { best = bits; best_f = f + r; }
          }
        }
      unsigned long long key = best == 0xffffffffu ? NO_KEY : ((unsigned long long)best << 32) | (unsigned)best_f;
      const unsigned long long other = __shfl_xor(key, 32);
      key = other < key ? other : key;
      if (h == 0 && p < P && key != NO_KEY) {
        unsigned long long* slot = a.keys + p;
        if (key < __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(slot, key);
      }
    }
  }
};

// ---- the k nearest reference rows of every query row (precision / recall / density / coverage) ----------
// EpiNearest's operands, distance and key.  keys [P][k], all-ones on entry, ends as the k smallest keys of every query in ascending
// order, whatever order the workgroups, waves and lanes run in:
//   filter   slot k-1 is the query's current k-th best.  It only ever decreases (every write below is an atomicMin) and ends as the
//            k-th smallest key, so a candidate whose key is not below ANY value read from it is not among the k smallest and is
//            dropped.  A stale read can only cost an insertion that was not needed.
//   insert   a lane carries its key through the slots s = 0 .. k-1:  old = atomicMin(slot[s], key);  key = max(old, key);  it stops
//            when it carries NO_KEY (the slot was empty) and drops what it carries past slot k-1.
//   why      each atomic leaves the multiset {slot values} + {carried keys} unchanged, and a carried key only moves forward.  Keys of
//            one query are distinct (they hold the index).  Every inserted key visits slot 0, so slot 0 ends as the minimum m0 of
//            them.  Every other key K leaves slot 0 exactly once: either it met a smaller value there and was carried on at once, or it
//            was stored and the smaller key that later displaced it (one must: the slot ends as m0 < K) carried it on.  So slot 1
//            sees every inserted key but m0 and ends as their minimum; by induction slot s ends as the s-th smallest.  The inserted
//            keys are a superset of the k smallest of all candidates (the filter drops nothing that belongs to them).
// The hot path per element is the distance and one integer minimum; per accumulator quad one signed compare of the quad's smallest
// distance bits with the threshold (the upper half of the key last read from slot k-1; -1 for a row beyond P, so nothing passes; a
// candidate that is out of range or excluded carries INT_MAX, above every float's bits and above the largest threshold).  A quad that
// passes walks its four elements in a rolled loop -- sixteen copies of the insertion code per wave tile, not sixty-four -- and the
// lane refreshes its threshold after every insertion, so of the candidates a lane holds it inserts the running k best only.
// f_base: the launch's reference rows are rows f_base.. of the caller's (the host seeds the thresholds with a first launch over the
// leading rows: 64 workgroups of an XCD start on one query tile together and would otherwise all see empty lists).
struct EpiKnn {
  static constexpr bool COUNTED_STORES = false;   // stores nothing but the atomics
  static constexpr bool XBUF = false;
  static constexpr unsigned long long NO_KEY = ~0ull;
  static constexpr int MAX_K = 16;
  template <class A> static __device__ __forceinline__ void slice(A&, int) {}
  struct Args { const float* sqr; const float* sqq; const int* exclude; unsigned long long* keys; int k; int f_base; };
  static bool fast_ok(const Args& a, int F) { return gram_fast_ok(a.sqr, F); }
  template <int NFB> using Pre = GramNorms<NFB>;
  template <int NFB, bool FAST>
  static __device__ __forceinline__ Pre<NFB> prefetch(const Args& a, int fw, int lane, int F) { return gram_norms<NFB, FAST>(a.sqr, fw, lane, F); }
  // the signed threshold a quad's smallest distance bits are compared with
  static __device__ __forceinline__ int threshold(unsigned long long kth, bool prow) {
    const unsigned hi = (unsigned)(kth >> 32);
    return prow ? (int)(hi < 0x7ffffffeu ? hi : 0x7ffffffeu) : -1;
  }
  template <int NFB, int NPB, bool FAST>
  static __device__ __forceinline__ void apply(f32x16 (&acc)[NFB][NPB], const Args& a, const Pre<NFB>& pre, int fw, int pw, int lane, int F, int P) {
    const int l31 = lane & 31, h = lane >> 5;
    const int k = a.k;
#pragma unroll
    for (int pb = 0; pb < NPB; ++pb) {
      const int p = pw + 32 * pb + l31;
      const bool prow = p < P;
      const int pc = prow ? p : P - 1;
      const float sq = a.sqq[pc];
      const int ex = a.exclude ? a.exclude[pc] - a.f_base : -1;
      unsigned long long* const slots = a.keys + (size_t)pc * k;
      unsigned long long kth = __hip_atomic_load(slots + (k - 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      int thr = threshold(kth, prow);
#pragma unroll
      for (int fb = 0; fb < NFB; ++fb)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int f = fw + 32 * fb + 8 * q + 4 * h;
          const float4 sr = pre.sq[fb][q];
          const float srv[4] = {sr.x, sr.y, sr.z, sr.w};
          int b[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float d2 = gram_d2(srv[r], sq, acc[fb][pb][4 * q + r]);
            b[r] = (f + r < F && f + r != ex) ? (int)__float_as_uint(d2) : 0x7fffffff;
          }
          const int m01 = b[0] < b[1] ? b[0] : b[1], m23 = b[2] < b[3] ? b[2] : b[3];
          if ((m01 < m23 ? m01 : m23) <= thr) {
#pragma unroll 1
            for (int r = 0; r < 4; ++r) {
              const int br = r == 0 ? b[0] : r == 1 ? b[1] : r == 2 ? b[2] : b[3];
              if (br > thr) continue;
              unsigned long long key = ((unsigned long long)(unsigned)br << 32) | (unsigned)(a.f_base + f + r);
              if (key >= kth) continue;            // equal distance bits, larger index
              for (int s = 0; s < k; ++s) {
                const unsigned long long old = atomicMin(slots + s, key);
                key = old > key ? old : key;
                if (key == NO_KEY) break;
              }
              kth = __hip_atomic_load(slots + (k - 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              thr = threshold(kth, prow);
            }
          }
        }
    }
  }
};

// ---- how many reference rows lie inside a per-row radius ---------------------------------------------
// EpiNearest's operands and distance.  Per query p two counts over the reference rows f < F:
//   in_ref[p]   = #{f : d2(p, f) <= r2_ref[f]}       the reference row's own radius
//   in_query[p] = #{f : d2(p, f) <= r2_query[p]}     the query row's radius
// `<=` on floats: a +inf radius holds every row, a negative or NaN one none.  A NULL radius array counts as -1 everywhere and its
// output is not touched; r2_ref rides in registers from before the K loop beside the reference norms (-1 for f >= F).  A lane holds
// one query and 16 * NFB reference rows; the two half-waves that share a query meet through lane^32 and one integer atomicAdd per
// query, count and wave goes out, skipped when the count is zero.  Integer sums: the result does not depend on the order.
struct EpiBallCount {
  static constexpr bool COUNTED_STORES = false;   // stores nothing but the atomics
  static constexpr bool XBUF = false;
  template <class A> static __device__ __forceinline__ void slice(A&, int) {}
  struct Args { const float* sqr; const float* sqq; const float* r2_ref; const float* r2_query; int* in_ref; int* in_query; };
  static bool fast_ok(const Args& a, int F) { return gram_fast_ok(a.sqr, F) && al16(a.r2_ref); }
  template <int NFB> struct Pre { GramNorms<NFB> n; float4 r2[NFB][4]; };
  template <int NFB, bool FAST>
  static __device__ __forceinline__ Pre<NFB> prefetch(const Args& a, int fw, int lane, int F) {
    Pre<NFB> r;
    const int h = lane >> 5;
#pragma unroll
    for (int fb = 0; fb < NFB; ++fb)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int f = fw + 32 * fb + 8 * q + 4 * h;
        r.n.sq[fb][q] = ldq<FAST>(a.sqr, f, F);           // gram_norms, interleaved with the radii
        float4 t = make_float4(-1.f, -1.f, -1.f, -1.f);
        if (a.r2_ref) {                            // uniform
          t = ldq<FAST>(a.r2_ref, f, F);
          t.x = f < F ? t.x : -1.f; t.y = f + 1 < F ? t.y : -1.f; t.z = f + 2 < F ? t.z : -1.f; t.w = f + 3 < F ? t.w : -1.f;
        }
        r.r2[fb][q] = t;
      }
    return r;
  }
  template <int NFB, int NPB, bool FAST>
  static __device__ __forceinline__ void apply(f32x16 (&acc)[NFB][NPB], const Args& a, const Pre<NFB>& pre, int fw, int pw, int lane, int F, int P) {
    const int l31 = lane & 31, h = lane >> 5;
#pragma unroll
    for (int pb = 0; pb < NPB; ++pb) {
      const int p = pw + 32 * pb + l31;
      const int pc = p < P ? p : P - 1;
      const float sq = a.sqq[pc];
      const float rq = a.r2_query ? a.r2_query[pc] : -1.f;
      int cr = 0, cq = 0;
#pragma unroll
      for (int fb = 0; fb < NFB; ++fb)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int f = fw + 32 * fb + 8 * q + 4 * h;
          const float4 sr = pre.n.sq[fb][q], rr = pre.r2[fb][q];
          const float srv[4] = {sr.x, sr.y, sr.z, sr.w};
          const float rrv[4] = {rr.x, rr.y, rr.z, rr.w};
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float d2 = gram_d2(srv[r], sq, acc[fb][pb][4 * q + r]);
            const bool valid = FAST ? f < F : f + r < F;        // FAST: F % 4 == 0, a quad is inside or outside as a whole
            cr += d2 <= rrv[r] ? 1 : 0;
            cq += (valid && d2 <= rq) ? 1 : 0;
          }
        }
      cr += __shfl_xor(cr, 32);
      cq += __shfl_xor(cq, 32);
      if (h == 0 && p < P) {
        if (cr) atomicAdd(a.in_ref + p, cr);       // cr, cq stay 0 where the radius array is NULL
        if (cq) atomicAdd(a.in_query + p, cq);
      }
    }
  }
};

}  // namespace osd
