// corr.hip -- second-order structure of a whole cohort on the device:
//   osd_val_centered_gram   G[i][j] = sum_r (X[r][i] - c[i]) (X[r][j] - c[j]) for all D x D column pairs, in double
//   osd_val_corr_compare    two such matrices compared as correlation matrices, block pair by block pair, without storing either
//
// The Gram kernel is a sibling of wgrad_item (wgrad_group.h): operands [rows][features], 32-row K stages moved by LDS-DMA into a
// linear [32][128] image that ds_read_b32 reads conflict-free, 128 x 128 tiles of v_mfma_f32_32x32x2_f32.  What differs:
//   * one workgroup of EIGHT waves per CU (64 x 32 of the tile each; the double sums below make registers the limit), and a
//     staging ring four stages deep, not two;
//   * A and B are two column windows (i0.., j0..) of the SAME matrix; only tiles with j0 >= i0 are computed (the reduction mirrors
//     them), and a diagonal tile stages one window and reads it as both operands;
//   * the centre is subtracted in registers after the fragment read: in the 32x32x2 MFMA a lane's A column and B column are fixed
//     over the whole K loop, so each centre is one register and one v_sub per operand per MFMA -- no centred copy of X;
//   * rows beyond the cohort in the last stage are MASKED AFTER centring (a zero row would otherwise add c_i c_j); their loads are
//     clamped to the last valid row;
//   * an fp32 accumulator run covers at most OSD_COV_SLAB_ROWS rows, then it is folded into double sums the workgroup keeps in
//     registers (32 doubles per lane) and writes once, to the slab of its work item (tile x row slice);
//   * the row slices of a tile are summed in a fixed order by cov_gram_reduce: no floating-point atomics, same inputs, same bits.
#include <limits.h>
#include <math.h>
#include <string.h>
#include <type_traits>
#include <vector>
#include "gemm_glds.h"
#include "handle.h"
#include "val_common.h"

namespace osd {
namespace {

constexpr int COV_BK = 32;
constexpr int COV_TILE = 128;
constexpr int COV_RUN_STAGES = OSD_COV_SLAB_ROWS / COV_BK;
constexpr int COV_NBUF = 4;                                         // K stages in LDS: one being read, up to three in flight
constexpr int COV_LDS_BYTES = COV_NBUF * 2 * COV_BK * COV_TILE * 4; // each an (A, B) pair of [32][128] fp32 images: 128 KiB
constexpr int COV_MAX_SLICES = 8;
constexpr int COV_SLAB_ELEMS = COV_TILE * COV_TILE;
constexpr int COV_WAVES = 8;                                        // 2 x 4 waves of 64 (A side) x 32 (B side)
constexpr int COV_THREADS = 64 * COV_WAVES;
static_assert(OSD_COV_SLAB_ROWS % COV_BK == 0 && COV_RUN_STAGES >= 1, "an accumulator run is a whole number of K stages");

struct CovArgs {
  const float* X;          // [rows][ld], 16-byte aligned, ld % 4 == 0, columns [0, Dq) readable
  const float* c;          // dev [nt * 128]: the centres, zero beyond D
  double* slab;            // [n_tri * S][128][128]: item (tile, slice) at (tile * S + slice) * 128 * 128, element [j - j0][i - i0]
  long long ld;
  int rows, D, Dq;         // Dq = roundup(D, 4)
  int nt, S, rows_per;     // tiles per dimension, row slices, rows per slice (a multiple of 32)
};

// upper-triangular tile number -> (ti, tj), tj >= ti, row-major
__device__ __host__ inline void tri_decode(int tile, int nt, int& ti, int& tj) {
  int i = 0, rem = tile;
  while (rem >= nt - i) { rem -= nt - i; ++i; }
  ti = i; tj = i + rem;
}

// One work item per workgroup, one workgroup of eight waves per CU (128 KiB of LDS): two waves per SIMD, each with a 64 x 32 share of
// the tile -- 32 fp32 accumulators and 32 double sums (64 VGPRs) per lane.
__global__ __launch_bounds__(COV_THREADS, 1) void cov_gram_kernel(CovArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int TILE = COV_BK * COV_TILE;
  auto buf_a = [&](int stage_no) { return smem + (stage_no & (COV_NBUF - 1)) * 2 * TILE; };      // its B image follows at + TILE

  const int item = blockIdx.x;
  const int tile = item / a.S, slice = item - tile * a.S;
  int ti, tj;
  tri_decode(tile, a.nt, ti, tj);
  const bool diag = ti == tj;                                // uniform: one staged window serves both operands
  const int i0 = ti * COV_TILE, j0 = tj * COV_TILE;
  const long long r0l = (long long)slice * a.rows_per;
  const int r0 = r0l < a.rows ? (int)r0l : a.rows;
  const int r1 = min(a.rows, r0 + a.rows_per);               // (rows < INT_MAX / 2: no overflow)
  const int nst = (r1 - r0 + COV_BK - 1) / COV_BK;           // 0 for a slice beyond the cohort: the item writes zeros

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wf = (wave >> 2) * 64, wp = (wave & 3) * 32;
  const int l31 = lane & 31, h = lane >> 5;

  // staging: piece q = 8 j + wave moves rows 2 q, 2 q + 1 of the stage; a lane carries 4 columns of one row.  Columns beyond the
  // extent re-read valid data (never stored); rows beyond the cohort re-read its last row (masked after centring).
  const int a_col = min(i0 + 4 * l31, a.Dq - 4);
  const int b_col = min(j0 + 4 * l31, a.Dq - 4);
  const int last_row = a.rows - 1;
  auto stage = [&](int k, float* As) {
    const unsigned la = __builtin_amdgcn_readfirstlane(lds_addr(As) + (unsigned)wave * 1024u);
    const unsigned lb = __builtin_amdgcn_readfirstlane(lds_addr(As + TILE) + (unsigned)wave * 1024u);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int m = min(r0 + k + 2 * (COV_WAVES * j + wave) + h, last_row);
      const float* row = a.X + (size_t)m * (size_t)a.ld;
      glds16(row + a_col, __builtin_amdgcn_readfirstlane(la + (unsigned)j * 8192u));
      if (!diag) glds16(row + b_col, __builtin_amdgcn_readfirstlane(lb + (unsigned)j * 8192u));
    }
  };

  // the lane's centres: its A columns i0 + wf + 32 fb + l31 and its B column j0 + wp + l31 (c is padded to whole tiles)
  float ca[2], cb;
#pragma unroll
  for (int fb = 0; fb < 2; ++fb) ca[fb] = a.c[i0 + wf + 32 * fb + l31];
  cb = a.c[j0 + wp + l31];
  // the centres are used here, before the first LDS-DMA: hipcc then waits for these three loads now and not with a vmcnt inside the K
  // loop, where its count (which leaves out the asm DMAs) would drain the stages in flight
  asm volatile("" : "+v"(ca[0]), "+v"(ca[1]), "+v"(cb));

  f32x16 acc[2];
  double dacc[2][16];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc[i][r] = 0.f; dacc[i][r] = 0.0; }

  // 32 rows of one stage; MASKED: only the first nv rows exist
  auto compute = [&](const float* Ac, const float* Bc, int nv, auto masked) {
    constexpr bool MASKED = decltype(masked)::value;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float av[2][4], bv[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int m = 8 * i + 2 * e + h;
        const bool live = !MASKED || m < nv;
#pragma unroll
        for (int fb = 0; fb < 2; ++fb) {
          const float v = Ac[m * 128 + wf + 32 * fb + l31] - ca[fb];
          av[fb][e] = live ? v : 0.f;
        }
        const float v = Bc[m * 128 + wp + l31] - cb;
        bv[e] = live ? v : 0.f;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int fb = 0; fb < 2; ++fb) acc[fb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[fb][e], bv[e], acc[fb], 0, 0, 0);
    }
  };

  // The one workgroup of a CU has nobody to hide its staging latency behind, so three stages stay in flight: stage kt + 3 is issued
  // when stage kt is about to be read, into the buffer stage kt - 1 was read from (every wave has left it: the barrier).  A wave
  // issues 2 (diagonal tile) or 4 LDS-DMA pieces per stage and they complete in order, so "at most 2 stages' pieces outstanding"
  // proves that this wave's pieces of stage kt have landed; the barrier then publishes every wave's.
  for (int p = 0; p < COV_NBUF - 1 && p < nst; ++p) stage(p * COV_BK, buf_a(p));
  for (int kt = 0; kt < nst; ++kt) {
    const int ahead = min(nst - kt - 1, COV_NBUF - 2);       // stages issued behind stage kt (uniform)
    if (ahead == 2) {
      if (diag) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    } else if (ahead == 1) {
      if (diag) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    if (kt + COV_NBUF - 1 < nst) stage((kt + COV_NBUF - 1) * COV_BK, buf_a(kt + COV_NBUF - 1));
    const float* Ac = buf_a(kt);
    const float* Bc = diag ? Ac : Ac + TILE;
    const int nv = r1 - r0 - kt * COV_BK;                    // rows of this stage that exist (uniform)
    if (nv >= COV_BK) compute(Ac, Bc, COV_BK, std::false_type{});
    else compute(Ac, Bc, nv, std::true_type{});
    if ((kt + 1) % COV_RUN_STAGES == 0 || kt + 1 == nst) {   // end of an accumulator run: fold it into the double sums
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) { dacc[i][r] += (double)acc[i][r]; acc[i][r] = 0.f; }
    }
  }

  // slab[jl][il]: register quad q of block fb holds A-side columns il .. il + 3 of B-side column jl
  double* out = a.slab + (size_t)item * COV_SLAB_ELEMS;
#pragma unroll
  for (int fb = 0; fb < 2; ++fb)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int il = wf + 32 * fb + 8 * q + 4 * h;
      const int jl = wp + l31;
      double* o = out + jl * COV_TILE + il;
#pragma unroll
      for (int t = 0; t < 4; ++t) o[t] = dacc[fb][4 * q + t];
    }
}

// G[i][j] = G[j][i] = sum over the tile's slices, slice 0 first.  One workgroup per tile, 32 x 32 sub-tiles through LDS so that both
// orientations are written along rows of G.  A diagonal tile was computed whole: its upper triangle (and diagonal) is what is kept.
__global__ __launch_bounds__(256) void cov_gram_reduce(const double* __restrict__ slab, int S, int nt, int D, double* __restrict__ G) {
  __shared__ double sub[32][33];
  int ti, tj;
  tri_decode(blockIdx.x, nt, ti, tj);
  const bool diag = ti == tj;
  const int i0 = ti * COV_TILE, j0 = tj * COV_TILE;
  const double* base = slab + (size_t)blockIdx.x * S * COV_SLAB_ELEMS;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int sj = 0; sj < 4; ++sj)
    for (int si = 0; si < 4; ++si) {
      if (i0 + 32 * si >= D || j0 + 32 * sj >= D) continue;                  // uniform
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int jl = 32 * sj + ty + 8 * rr, il = 32 * si + tx;
        const double* p = base + jl * COV_TILE + il;
        double v = p[0];
        for (int s = 1; s < S; ++s) v += p[(size_t)s * COV_SLAB_ELEMS];
        sub[ty + 8 * rr][tx] = v;                                            // [j][i]
        const int i = i0 + il, j = j0 + jl;
        if (i < D && j < D && (!diag || i < j)) G[(size_t)j * D + i] = v;
      }
      __syncthreads();
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int il = 32 * si + ty + 8 * rr, jl = 32 * sj + tx;
        const int i = i0 + il, j = j0 + jl;
        if (i < D && j < D && (!diag || i <= j)) G[(size_t)i * D + j] = sub[tx][ty + 8 * rr];
      }
      __syncthreads();
    }
}

// dst[r][c] = src[r][c] for c < D, 0 for D <= c < Dq: the aligned copy of an X that 16-byte staging cannot read in place
__global__ void cov_pad_copy(const float* __restrict__ src, long long ld, long long rows, int D, int Dq, float* __restrict__ dst) {
  const long long total = rows * Dq;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long r = i / Dq;
    const int c = (int)(i - r * Dq);
    dst[i] = c < D ? src[r * ld + c] : 0.f;
  }
}

// ---- correlation comparison -----------------------------------------------------------------------------------------------------
// diagonals of both matrices; live[i] = 0 for a constant column (G[i][i] <= 0, or NaN, in either matrix)
__global__ void corr_diag(const double* __restrict__ Gr, const double* __restrict__ Gs, int D, double* dr, double* ds, int* live,
                          unsigned long long* n_const) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= D) return;
  const double x = Gr[(size_t)i * D + i], y = Gs[(size_t)i * D + i];
  const bool ok = x > 0 && y > 0;
  dr[i] = x; ds[i] = y; live[i] = ok ? 1 : 0;
  if (!ok) atomicAdd(n_const, 1ull);
}

struct CorrSlot {             // one block pair; [3] holds the bits of a non-negative double (ordered as integers)
  unsigned long long pairs;
  double sum_abs, sum_sq;
  unsigned long long max_bits, strong, agree;
  double strong_abs;
};
static_assert(sizeof(CorrSlot) == OSD_CORR_STATS * 8, "seven 8-byte figures per block pair");

__device__ __forceinline__ int sgn(double x) { return (x > 0) - (x < 0); }

// blockIdx.y = block pair (a <= b, row-major); a wavefront per row i of block a, lanes over the columns j > i of block b
__global__ __launch_bounds__(256) void corr_compare_kernel(const double* __restrict__ Gr, const double* __restrict__ Gs, int D,
                                                           const int* __restrict__ bounds, int nb, const double* __restrict__ dr,
                                                           const double* __restrict__ ds, const int* __restrict__ live, double strong,
                                                           CorrSlot* slots) {
  int ba, bb;
  tri_decode(blockIdx.y, nb, ba, bb);
  const int ilo = bounds[ba], ihi = bounds[ba + 1], jlo = bounds[bb], jhi = bounds[bb + 1];
  const auto [lane, wave, nw] = wave_rows<int>();
  unsigned long long n = 0, ns = 0, na = 0;
  double s1 = 0.0, s2 = 0.0, mx = 0.0, s3 = 0.0;
  for (int i = ilo + wave; i < ihi; i += nw) {
    if (!live[i]) continue;                                  // uniform over the wave
    const double di_r = dr[i], di_s = ds[i];
    const double* gr = Gr + (size_t)i * D;
    const double* gs = Gs + (size_t)i * D;
    for (int j = max(jlo, i + 1) + lane; j < jhi; j += 64) {
      if (!live[j]) continue;
      const double rr = gr[j] / sqrt(di_r * dr[j]);
      const double rs = gs[j] / sqrt(di_s * ds[j]);
      const double d = rs - rr, ad = fabs(d);
      ++n; s1 += ad; s2 += d * d; mx = ad > mx ? ad : mx;
      if (fabs(rr) >= strong) { ++ns; na += sgn(rs) == sgn(rr) ? 1 : 0; s3 += ad; }
    }
  }
  wave_sum(n, ns, na, s1, s2, s3);
  wave_max(mx);
  if (lane == 0 && n > 0) {
    CorrSlot* s = slots + blockIdx.y;
    atomicAdd(&s->pairs, n); atomicAdd(&s->strong, ns); atomicAdd(&s->agree, na);
    atomicAdd(&s->sum_abs, s1); atomicAdd(&s->sum_sq, s2); atomicAdd(&s->strong_abs, s3);
    atomicMax(&s->max_bits, (unsigned long long)__double_as_longlong(mx));
  }
}

// Row slices of a tile, from the tile count and the CU count alone (the workspace is n_tri * S slabs whatever the number of rows).
// The kernel holds one workgroup per CU, so a launch of n_tri * S items runs in ceil(n_tri * S / cus) rounds of 1 / S of a tile's
// rows each: the smallest S <= COV_MAX_SLICES whose rounds / S is within 5 % of the best (136 tiles on 256 CUs: S = 5, three
// rounds of a fifth, against one round of everything at S = 1 with 120 CUs idle).
int cov_slices(int n_tri, int cus) {
  if (cus < 1) cus = 1;
  double cost[COV_MAX_SLICES + 1], best = 1e30;
  for (int s = 1; s <= COV_MAX_SLICES; ++s) {
    cost[s] = (double)(((long long)n_tri * s + cus - 1) / cus) / s;
    if (cost[s] < best) best = cost[s];
  }
  for (int s = 1; s <= COV_MAX_SLICES; ++s)
    if (cost[s] <= 1.05 * best) return s;
  return 1;
}

}  // namespace
}  // namespace osd

using namespace osd;

extern "C" {

int osd_val_centered_gram(void* stream, int device, const float* X, int64_t rows, int ld, int D, const float* center_host, double* G_dev) {
  if (!X || !center_host || !G_dev || rows < 1 || D < 1 || ld < D || rows > INT_MAX / 2 - 64 || D > 32768) {
    set_error("bad argument (rows >= 1, 1 <= D <= 32768, ld >= D)");
    return OSD_EINVAL;
  }
  OSD_HIP(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  int cus = 0;
  OSD_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
  OSD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(cov_gram_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, COV_LDS_BYTES));
  const int nt = (D + COV_TILE - 1) / COV_TILE, n_tri = nt * (nt + 1) / 2;
  const int Dq = (D + 3) / 4 * 4;
  CovArgs a{};
  a.rows = (int)rows; a.D = D; a.Dq = Dq; a.nt = nt;
  a.S = cov_slices(n_tri, cus);
  a.rows_per = (int)(((rows + a.S - 1) / a.S + COV_BK - 1) / COV_BK * COV_BK);
  ValBuf cen, slab, pad;
  OSD_TRY(cen.alloc((size_t)nt * COV_TILE * sizeof(float)));
  OSD_TRY(slab.alloc((size_t)n_tri * a.S * COV_SLAB_ELEMS * sizeof(double)));
  OSD_HIP(hipMemsetAsync(cen.get(), 0, (size_t)nt * COV_TILE * sizeof(float), s));
  OSD_HIP(hipMemcpyAsync(cen.get(), center_host, (size_t)D * sizeof(float), hipMemcpyHostToDevice, s));
  a.c = (const float*)cen.get();
  a.slab = (double*)slab.get();
  if ((reinterpret_cast<uintptr_t>(X) & 15) == 0 && ld % 4 == 0 && ld >= Dq) {
    a.X = X; a.ld = ld;
  } else {                                                   // 16-byte LDS-DMA cannot read this X in place
    OSD_TRY(pad.alloc((size_t)rows * Dq * sizeof(float)));
    OSD_HIP(launched(cov_pad_copy, 2048, 256, 0, s, X, (long long)ld, (long long)rows, D, Dq, pad.as<float>()));
    a.X = (const float*)pad.get(); a.ld = Dq;
  }
  OSD_HIP(launched(cov_gram_kernel, dim3((unsigned)(n_tri * a.S)), dim3(COV_THREADS), COV_LDS_BYTES, s, a));
  OSD_HIP(launched(cov_gram_reduce, dim3((unsigned)n_tri), dim3(256), 0, s, slab.as<const double>(), a.S, nt, D, G_dev));
  OSD_HIP(hipStreamSynchronize(s));
  return OSD_OK;
}

int osd_val_corr_compare(void* stream, int device, const double* G_real, const double* G_synth, int D, const int32_t* bounds_host,
                         int n_blocks, double strong, double* out_host) {
  if (!G_real || !G_synth || !bounds_host || !out_host || D < 1 || n_blocks < 1 || n_blocks > D || !(strong == strong)) {
    set_error("bad argument");
    return OSD_EINVAL;
  }
  bool sorted = bounds_host[0] == 0 && bounds_host[n_blocks] == D;
  for (int b = 0; sorted && b < n_blocks; ++b) sorted = bounds_host[b] < bounds_host[b + 1];
  if (!sorted) { set_error("block bounds must be 0 = b_0 < b_1 < ... < b_n = D"); return OSD_EINVAL; }
  if (n_blocks > 1024) { set_error("at most 1024 column blocks"); return OSD_EINVAL; }
  OSD_HIP(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  const int n_pairs = n_blocks * (n_blocks + 1) / 2;
  ValBuf diag, flags, bnd, res;
  OSD_TRY(diag.alloc((size_t)2 * D * sizeof(double)));
  OSD_TRY(flags.alloc((size_t)D * sizeof(int)));
  OSD_TRY(bnd.alloc((size_t)(n_blocks + 1) * sizeof(int)));
  OSD_TRY(res.alloc(sizeof(unsigned long long) + (size_t)n_pairs * sizeof(CorrSlot)));
  unsigned long long* n_const = (unsigned long long*)res.get();
  CorrSlot* slots = (CorrSlot*)(n_const + 1);
  double* dr = (double*)diag.get(); double* ds = dr + D;
  OSD_HIP(hipMemsetAsync(res.get(), 0, sizeof(unsigned long long) + (size_t)n_pairs * sizeof(CorrSlot), s));
  OSD_HIP(hipMemcpyAsync(bnd.get(), bounds_host, (size_t)(n_blocks + 1) * sizeof(int), hipMemcpyHostToDevice, s));
  OSD_HIP(launched(corr_diag, dim3((unsigned)((D + 255) / 256)), dim3(256), 0, s, G_real, G_synth, D, dr, ds, flags.as<int>(), n_const));
  // up to 256 wavefronts walk the rows of a block; one set of atomics per wavefront and block pair
  int gx = (D / n_blocks + 3) / 4;
  gx = gx < 1 ? 1 : (gx > 64 ? 64 : gx);
  OSD_HIP(launched(corr_compare_kernel, dim3((unsigned)gx, (unsigned)n_pairs), dim3(256), 0, s, G_real, G_synth, D, bnd.as<const int>(),
                   n_blocks, dr, ds, flags.as<const int>(), strong, slots));
  std::vector<unsigned long long> raw((size_t)1 + (size_t)n_pairs * OSD_CORR_STATS);
  OSD_HIP(read_back(s, raw.data(), res.get(), raw.size() * 8));
  out_host[0] = (double)raw[0];
  for (int p = 0; p < n_pairs; ++p) {
    CorrSlot c;
    memcpy(&c, raw.data() + 1 + (size_t)p * OSD_CORR_STATS, sizeof(c));
    double mx;
    memcpy(&mx, &c.max_bits, 8);
    double* o = out_host + 1 + (size_t)p * OSD_CORR_STATS;
    o[0] = (double)c.pairs; o[1] = c.sum_abs; o[2] = c.sum_sq; o[3] = mx; o[4] = (double)c.strong; o[5] = (double)c.agree; o[6] = c.strong_abs;
  }
  return OSD_OK;
}

}  // extern "C"
