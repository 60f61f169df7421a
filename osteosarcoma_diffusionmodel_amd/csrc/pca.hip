// pca.hip -- the two skinny products of a block subspace iteration over a device-resident cohort.  With
// u_rc = ((double) x_rc - center_c) * scale_c (scale NULL: 1) and everything after the load in double:
//   osd_val_pca_project      Z[r][j] = sum_c u_rc V[c][j]  and  norm2[r] = sum_c u_rc^2
//   osd_val_pca_backproject  W[c][j] = sum_r u_rc Z[r][j]
// One iteration is one call of each: X is read twice, as osd_val_cox_eval reads it.
//
// Both kernels keep the long axis of the OUTPUT on the lanes and the l directions in a lane's registers, and read the small matrix
// (V, Z) through wave-uniform addresses, so its values arrive in scalar registers and every inner step is one double FMA per
// direction with no cross-lane traffic:
//   project      an item is 64 consecutive rows (a lane owns a row) times a slab of columns, one wavefront.  The slab is walked in
//                tiles of 32 columns: the tile is loaded coalesced (16 bytes a lane on the ALIGNED path, dwords otherwise) into
//                registers one tile ahead, passes through LDS (row stride 33: no bank conflict), and the lane adds its row's terms
//                in COLUMN order.  pca_project_combine adds the slabs in slab order.
//   backproject  an item is a block of consecutive rows times a slab of 128 columns, one wavefront; a lane owns two columns (an
//                adjacent pair on the ALIGNED path, lane and lane + 64 otherwise), loads them coalesced two row groups ahead,
//                requests Z's next row while this row's FMAs run, and adds the rows' terms in ROW order.
//                pca_backproject_reduce adds the blocks: PCA_PARTS contiguous runs of blocks in block order, the runs in run order.
// No floating-point atomics, no workgroup waits for another, every sum has one fixed order; the partition depends on (rows, D, l)
// and the load path only: the same inputs give the same bits on every call.
//
// Vector FMAs in double, not v_mfma_f64_16x16x4_f64.  On this part the double matrix rate equals the double vector rate (the
// public peak figures of the two are the same), so the matrix instruction can only save issue slots, and it pays for them with l
// padded to 16 or 32: at the default l = 18 that is 32 / 18 = 1.8 times the FMAs of a loop that is already level with the two
// reads of X (4 n D l FLOPs against 8 n D bytes: at l = 18 the FMAs of a pair take about as long as its bytes).  Here l is padded
// to the next even number only (LP; the pad columns of V and Z are zeros in a workspace copy, made only when l is odd), and the
// u = (x - c) s preparation costs three double operations per element beside the l FMAs.  Measured, the
// kernels sit at neither bound: they are paced by the scalar fetch around each run of FMAs, which the matrix form would not remove.
#include <stdint.h>
#include <mutex>
#include "handle.h"
#include "val_common.h"

namespace osd {
namespace {

constexpr int PCA_MAX_DIRS = OSD_PCA_MAX_DIRS;
constexpr int PCA_MAX_D = 32768;
constexpr int PCA_MAX_DEVICES = 64;
constexpr int PCA_T = 64;                // an item is one wavefront
constexpr int PJ_ROWS = 64;              // project: rows of an item, one per lane
constexpr int PJ_COLS = 32;              // project: columns of a tile
constexpr int PJ_STRIDE = PJ_COLS + 1;   // floats between two rows of the LDS tile
constexpr int PJ_PER = PJ_ROWS * PJ_COLS / PCA_T;      // values of a tile a lane loads
constexpr int BP_PER = 2;                // backproject: columns of a lane
constexpr int BP_SLAB = PCA_T * BP_PER;
constexpr int BP_U = 4;                  // backproject: rows of a load group; two groups are in flight
constexpr int BP_Z_AHEAD_MAX = 18;       // backproject: up to this LP, Z's next row is requested one row ahead (two rows fit the scalar registers)
constexpr int PCA_TARGET_ITEMS = 8192;   // items a call aims at: twice the wavefronts that are resident at four per SIMD
constexpr int PCA_PARTS = 16;            // runs of blocks of the backproject reduction
static_assert(PCA_MAX_DIRS % 2 == 0, "l is padded to an even number");

struct PcaArgs {
  const float* X; const double* center; const double* scale;
  const double* M;               // project: V [D][LP]; backproject: Z [rows][LP]
  double* part;                  // project: [slabs][rows][LP]; backproject: [blocks][D][LP]
  double* n2part;                // project: [slabs][rows], or null
  long long ld, rows, rows_per;  // rows_per: rows of a backproject item, a multiple of BP_U
  int D, slab_cols;              // slab_cols: columns of a project slab, a multiple of PJ_COLS
};

// dst [n][LP] = src [n][l] with zeros in the pad columns
__global__ __launch_bounds__(256) void pca_pad(const double* __restrict__ src, double* __restrict__ dst, long long n, int l, int LP) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n * LP) return;
  const long long r = i / LP;
  const int j = (int)(i - r * LP);
  dst[i] = j < l ? src[r * l + j] : 0.0;
}

template <int LP, bool ALIGNED>
__global__ __launch_bounds__(PCA_T) void pca_project_kernel(PcaArgs a) {
  __shared__ float tile[PJ_ROWS * PJ_STRIDE];
  const int lane = threadIdx.x;
  const long long r0 = (long long)blockIdx.x * PJ_ROWS;      // r0 < rows: the host launches no empty item
  const int cbeg = (int)blockIdx.y * a.slab_cols, cend = min(a.D, cbeg + a.slab_cols);
  const double* __restrict__ V = a.M;
  const double* __restrict__ center = a.center;
  const double* __restrict__ scale = a.scale;

  // The tile's values of this lane, one tile ahead.  A row beyond the cohort re-reads the last one (its result is not stored);
  // a column beyond the slab is never read from LDS.
  float pre[PJ_PER];
  auto fetch = [&](int c0) {
    if (ALIGNED) {
      const int q = (lane & 7) * 4;
#pragma unroll
      for (int i = 0; i < PJ_PER / 4; ++i) {
        const long long row = min(r0 + 8 * i + (lane >> 3), a.rows - 1);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c0 + q < cend) v = *reinterpret_cast<const float4*>(a.X + (size_t)row * (size_t)a.ld + c0 + q);   // ld >= roundup(D, 4): inside the row
        pre[4 * i] = v.x; pre[4 * i + 1] = v.y; pre[4 * i + 2] = v.z; pre[4 * i + 3] = v.w;
      }
    } else {
      const int col = c0 + (lane & 31);
#pragma unroll
      for (int i = 0; i < PJ_PER; ++i) {
        const long long row = min(r0 + 2 * i + (lane >> 5), a.rows - 1);
        pre[i] = col < cend ? a.X[(size_t)row * (size_t)a.ld + col] : 0.f;
      }
    }
  };
  auto stash = [&]() {
    if (ALIGNED) {
      const int q = (lane & 7) * 4;
#pragma unroll
      for (int i = 0; i < PJ_PER / 4; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) tile[(8 * i + (lane >> 3)) * PJ_STRIDE + q + e] = pre[4 * i + e];
    } else {
#pragma unroll
      for (int i = 0; i < PJ_PER; ++i) tile[(2 * i + (lane >> 5)) * PJ_STRIDE + (lane & 31)] = pre[i];
    }
  };

  double z[LP], n2 = 0.0;
#pragma unroll
  for (int j = 0; j < LP; ++j) z[j] = 0.0;
  fetch(cbeg);
  for (int c0 = cbeg; c0 < cend; c0 += PJ_COLS) {
    __syncthreads();                                         // the previous tile has been read
    stash();
    __syncthreads();
    if (c0 + PJ_COLS < cend) fetch(c0 + PJ_COLS);
    const int nc = min(PJ_COLS, cend - c0);
    for (int cc = 0; cc < nc; ++cc) {                        // the lane's row, in column order
      const int col = c0 + cc;                               // wave-uniform: centre, scale and V's row arrive in scalar registers
      const double s = scale ? scale[col] : 1.0;
      const double u = ((double)tile[lane * PJ_STRIDE + cc] - center[col]) * s;
      n2 = fma(u, u, n2);
      const double* __restrict__ v = V + (size_t)col * LP;
#pragma unroll
      for (int j = 0; j < LP; ++j) z[j] = fma(u, v[j], z[j]);
    }
  }
  const long long row = r0 + lane;
  if (row >= a.rows) return;
  const size_t at = (size_t)blockIdx.y * (size_t)a.rows + (size_t)row;
#pragma unroll
  for (int j = 0; j < LP; ++j) a.part[at * LP + j] = z[j];
  if (a.n2part) a.n2part[at] = n2;
}

// Z[r][j] = the sum over the slabs of part[s][r][j], in slab order; norm2 likewise
__global__ __launch_bounds__(256) void pca_project_combine(const double* __restrict__ part, const double* __restrict__ n2part, int slabs,
                                                           long long rows, int LP, int l, double* __restrict__ Z,
                                                           double* __restrict__ norm2) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * l) return;
  const long long r = i / l;
  const int j = (int)(i - r * l);
  double t = 0.0;
  for (int s = 0; s < slabs; ++s) t += part[((size_t)s * (size_t)rows + (size_t)r) * LP + j];
  Z[i] = t;
  if (j == 0 && norm2) {
    double q = 0.0;
    for (int s = 0; s < slabs; ++s) q += n2part[(size_t)s * (size_t)rows + (size_t)r];
    norm2[r] = q;
  }
}

template <bool ALIGNED>
__device__ __forceinline__ int bp_col(int slab, int lane, int e) {
  return slab * BP_SLAB + (ALIGNED ? BP_PER * lane + e : lane + PCA_T * e);
}

template <int LP, bool ALIGNED>
__global__ __launch_bounds__(PCA_T) void pca_backproject_kernel(PcaArgs a) {
  const int lane = threadIdx.x, slab = blockIdx.y;
  const long long blk = blockIdx.x;
  const long long r0 = blk * a.rows_per, r1 = min(a.rows, r0 + a.rows_per);    // r0 < r1: the host launches no empty block
  const double* __restrict__ Zp = a.M;
  double c[BP_PER], s[BP_PER], w[BP_PER][LP];
  bool in[BP_PER];
#pragma unroll
  for (int e = 0; e < BP_PER; ++e) {
    const int col = bp_col<ALIGNED>(slab, lane, e);
    in[e] = col < a.D;
    c[e] = in[e] ? a.center[col] : 0.0;
    s[e] = !in[e] ? 0.0 : a.scale ? a.scale[col] : 1.0;
#pragma unroll
    for (int j = 0; j < LP; ++j) w[e][j] = 0.0;
  }
  // Two buffers of BP_U rows: the loads of the next group are in flight while this group's arithmetic runs.  A row beyond the block
  // re-reads the block's last one and is not used; a column beyond D reads as 0.
  struct Group { float x[BP_U][BP_PER]; };
  auto fetch = [&](Group& g, long long g0) {
#pragma unroll
    for (int r = 0; r < BP_U; ++r) {
      const float* p = a.X + (size_t)min(g0 + r, r1 - 1) * (size_t)a.ld;
      if (ALIGNED) {
        float2 v = make_float2(0.f, 0.f);
        if (in[0]) v = *reinterpret_cast<const float2*>(p + bp_col<true>(slab, lane, 0));     // ld >= roundup(D, 4): inside the row
        g.x[r][0] = v.x; g.x[r][1] = in[1] ? v.y : 0.f;
      } else {
#pragma unroll
        for (int e = 0; e < BP_PER; ++e) g.x[r][e] = in[e] ? p[bp_col<false>(slab, lane, e)] : 0.f;
      }
    }
  };
  // Z's row: wave-uniform, so it arrives in scalar registers.  Its latency is a round trip per row unless the next row is
  // requested before this row's FMAs: zn holds that next row (a row beyond the block re-reads the block's last one).
  constexpr bool Z_AHEAD = LP <= BP_Z_AHEAD_MAX;
  double zn[LP];
  auto zfetch = [&](long long row) {
    const double* __restrict__ zr = Zp + (size_t)min(row, r1 - 1) * LP;
#pragma unroll
    for (int j = 0; j < LP; ++j) zn[j] = zr[j];
  };
  auto consume = [&](const Group& g, long long g0) {
#pragma unroll
    for (int r = 0; r < BP_U; ++r) {
      const long long row = g0 + r;
      if (row >= r1) break;                                  // uniform: the whole wavefront leaves together
      double zc[LP];
      if (Z_AHEAD) {
#pragma unroll
        for (int j = 0; j < LP; ++j) zc[j] = zn[j];
        zfetch(row + 1);
      } else {
        const double* __restrict__ zr = Zp + (size_t)row * LP;
#pragma unroll
        for (int j = 0; j < LP; ++j) zc[j] = zr[j];
      }
      double u[BP_PER];
#pragma unroll
      for (int e = 0; e < BP_PER; ++e) u[e] = ((double)g.x[r][e] - c[e]) * s[e];
#pragma unroll
      for (int j = 0; j < LP; ++j)
#pragma unroll
        for (int e = 0; e < BP_PER; ++e) w[e][j] = fma(u[e], zc[j], w[e][j]);
    }
  };
  Group ga, gb;
  if (Z_AHEAD) zfetch(r0);
  fetch(ga, r0);
  for (long long g0 = r0; g0 < r1; g0 += 2 * BP_U) {
    if (g0 + BP_U < r1) fetch(gb, g0 + BP_U);
    consume(ga, g0);
    if (g0 + BP_U >= r1) break;
    if (g0 + 2 * BP_U < r1) fetch(ga, g0 + 2 * BP_U);
    consume(gb, g0 + BP_U);
  }
#pragma unroll
  for (int e = 0; e < BP_PER; ++e) {
    if (!in[e]) continue;
    const size_t at = ((size_t)blk * (size_t)a.D + (size_t)bp_col<ALIGNED>(slab, lane, e)) * LP;
#pragma unroll
    for (int j = 0; j < LP; ++j) a.part[at + j] = w[e][j];
  }
}

// W[c][j] = the sum over the blocks of part[b][c][j]: wave w adds the w-th run of `chunk` blocks in block order, wave 0 the runs in
// run order.  A lane of a wave owns one (c, j).
__global__ __launch_bounds__(PCA_T * PCA_PARTS) void pca_backproject_reduce(const double* __restrict__ part, long long blocks, long long chunk,
                                                                            int D, int LP, int l, double* __restrict__ W) {
  __shared__ double run[PCA_PARTS][PCA_T];
  const int cx = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long long i = (long long)blockIdx.x * PCA_T + cx, n = (long long)D * l;
  const long long b0 = min(blocks, (long long)w * chunk), b1 = min(blocks, b0 + chunk);
  double t = 0.0;
  if (i < n) {
    const long long col = i / l;
    const size_t at = (size_t)col * LP + (size_t)(i - col * l), step = (size_t)D * LP;
    for (long long b = b0; b < b1; ++b) t += part[(size_t)b * step + at];
  }
  run[w][cx] = t;
  __syncthreads();
  if (w != 0 || i >= n) return;
  for (int q = 1; q < PCA_PARTS; ++q) t += run[q][cx];
  W[i] = t;
}

// One grow-only workspace per device, held for the length of a call: a fit calls the pair once per iteration.
struct PcaWorkspace {
  std::mutex mu;
  DevBuf<char> buf;
};
PcaWorkspace* const g_pca_ws = new PcaWorkspace[PCA_MAX_DEVICES];     // never destroyed: no hipFree from a static destructor at process exit

inline size_t pca_up256(size_t v) { return (v + 255) / 256 * 256; }

template <int LP>
hipError_t pca_launch_lp(bool project, bool aligned, dim3 grid, hipStream_t s, const PcaArgs& a) {
  if (project) return launched(aligned ? pca_project_kernel<LP, true> : pca_project_kernel<LP, false>, grid, dim3(PCA_T), 0, s, a);
  return launched(aligned ? pca_backproject_kernel<LP, true> : pca_backproject_kernel<LP, false>, grid, dim3(PCA_T), 0, s, a);
}

hipError_t pca_launch(int LP, bool project, bool aligned, dim3 grid, hipStream_t s, const PcaArgs& a) {
  switch (LP) {
    case 2: return pca_launch_lp<2>(project, aligned, grid, s, a);
    case 4: return pca_launch_lp<4>(project, aligned, grid, s, a);
    case 6: return pca_launch_lp<6>(project, aligned, grid, s, a);
    case 8: return pca_launch_lp<8>(project, aligned, grid, s, a);
    case 10: return pca_launch_lp<10>(project, aligned, grid, s, a);
    case 12: return pca_launch_lp<12>(project, aligned, grid, s, a);
    case 14: return pca_launch_lp<14>(project, aligned, grid, s, a);
    case 16: return pca_launch_lp<16>(project, aligned, grid, s, a);
    case 18: return pca_launch_lp<18>(project, aligned, grid, s, a);
    case 20: return pca_launch_lp<20>(project, aligned, grid, s, a);
    case 22: return pca_launch_lp<22>(project, aligned, grid, s, a);
    case 24: return pca_launch_lp<24>(project, aligned, grid, s, a);
    case 26: return pca_launch_lp<26>(project, aligned, grid, s, a);
    case 28: return pca_launch_lp<28>(project, aligned, grid, s, a);
    case 30: return pca_launch_lp<30>(project, aligned, grid, s, a);
    default: return pca_launch_lp<32>(project, aligned, grid, s, a);
  }
}

// what both entry points refuse, before anything touches the device
int pca_check(const void* X, const void* center, const void* M, const void* out, int64_t rows, int ld, int D, int l, int device) {
  if (!X || !center || !M || !out || l < 1 || l > PCA_MAX_DIRS || D < l || D > PCA_MAX_D || ld < D || rows < 1 || rows > INT32_MAX ||
      device < 0 || device >= PCA_MAX_DEVICES) {
    set_error("bad argument (1 <= l <= %d, l <= D <= %d, ld >= D, 1 <= rows < 2^31, the matrices and the centre given)", PCA_MAX_DIRS,
              PCA_MAX_D);
    return OSD_EINVAL;
  }
  return OSD_OK;
}

inline bool pca_aligned(const float* X, int ld, int D) {
  return (reinterpret_cast<uintptr_t>(X) & 15) == 0 && ld % 4 == 0 && ld >= (D + 3) / 4 * 4;
}

}  // namespace
}  // namespace osd

using namespace osd;

extern "C" {

int osd_val_pca_project(void* stream, int device, const float* X, int64_t rows, int ld, int D, const double* center,
                        const double* scale, const double* V, int l, double* Z_dev, double* norm2_dev) {
  OSD_TRY(pca_check(X, center, V, Z_dev, rows, ld, D, l, device));
  OSD_HIP(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  const int LP = (l + 1) / 2 * 2;
  const bool aligned = pca_aligned(X, ld, D);
  // the partition: a function of (rows, D, l) alone
  const long long row_blocks = ((long long)rows + PJ_ROWS - 1) / PJ_ROWS;
  const int tiles = (D + PJ_COLS - 1) / PJ_COLS;
  long long want = (PCA_TARGET_ITEMS + row_blocks - 1) / row_blocks;
  if (want > D / (4 * LP)) want = D / (4 * LP);              // the slabs' partial scores stay below half of X's bytes
  if (want > tiles) want = tiles;
  if (want < 1) want = 1;
  const int slab_cols = (int)((tiles + want - 1) / want) * PJ_COLS;
  const int slabs = (D + slab_cols - 1) / slab_cols;

  PcaWorkspace& ws = g_pca_ws[device];
  std::lock_guard<std::mutex> hold(ws.mu);
  const size_t v_bytes = LP != l ? pca_up256((size_t)D * LP * sizeof(double)) : 0;
  const size_t part_bytes = pca_up256((size_t)slabs * (size_t)rows * LP * sizeof(double));
  const size_t n2_bytes = norm2_dev ? pca_up256((size_t)slabs * (size_t)rows * sizeof(double)) : 0;
  OSD_TRY(ws.buf.reserve((int64_t)(v_bytes + part_bytes + n2_bytes)));
  double* vp = (double*)ws.buf.get();
  if (LP != l)
    OSD_HIP(launched(pca_pad, dim3((unsigned)(((long long)D * LP + 255) / 256)), dim3(256), 0, s, V, vp, (long long)D, l, LP));

  PcaArgs a{};
  a.X = X; a.center = center; a.scale = scale; a.M = LP != l ? vp : V;
  a.part = (double*)(ws.buf.get() + v_bytes);
  a.n2part = norm2_dev ? (double*)(ws.buf.get() + v_bytes + part_bytes) : nullptr;
  a.ld = ld; a.rows = rows; a.rows_per = PJ_ROWS; a.D = D; a.slab_cols = slab_cols;
  OSD_HIP(pca_launch(LP, true, aligned, dim3((unsigned)row_blocks, (unsigned)slabs), s, a));
  OSD_HIP(launched(pca_project_combine, dim3((unsigned)(((long long)rows * l + 255) / 256)), dim3(256), 0, s, (const double*)a.part,
                   (const double*)a.n2part, slabs, (long long)rows, LP, l, Z_dev, norm2_dev));
  OSD_HIP(hipStreamSynchronize(s));
  return OSD_OK;
}

int osd_val_pca_backproject(void* stream, int device, const float* X, int64_t rows, int ld, int D, const double* center,
                            const double* scale, const double* Z_dev, int l, double* W_dev) {
  OSD_TRY(pca_check(X, center, Z_dev, W_dev, rows, ld, D, l, device));
  OSD_HIP(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  const int LP = (l + 1) / 2 * 2;
  const bool aligned = pca_aligned(X, ld, D);
  // the partition: a function of (rows, D, l) alone
  const unsigned slabs = (unsigned)((D + BP_SLAB - 1) / BP_SLAB);
  long long blocks = (PCA_TARGET_ITEMS + slabs - 1) / slabs;
  const long long most = ((long long)rows + PJ_ROWS - 1) / PJ_ROWS;            // a block is not shorter than 64 rows
  if (blocks > most) blocks = most;
  if (blocks > rows / (4 * LP)) blocks = rows / (4 * LP);    // the blocks' partial sums stay below half of X's bytes
  if (blocks < 1) blocks = 1;
  const long long rows_per = (((long long)rows + blocks - 1) / blocks + BP_U - 1) / BP_U * BP_U;
  blocks = ((long long)rows + rows_per - 1) / rows_per;
  const long long chunk = (blocks + PCA_PARTS - 1) / PCA_PARTS;

  PcaWorkspace& ws = g_pca_ws[device];
  std::lock_guard<std::mutex> hold(ws.mu);
  const size_t z_bytes = LP != l ? pca_up256((size_t)rows * LP * sizeof(double)) : 0;
  const size_t part_bytes = pca_up256((size_t)blocks * (size_t)D * LP * sizeof(double));
  OSD_TRY(ws.buf.reserve((int64_t)(z_bytes + part_bytes)));
  double* zp = (double*)ws.buf.get();
  if (LP != l)
    OSD_HIP(launched(pca_pad, dim3((unsigned)(((long long)rows * LP + 255) / 256)), dim3(256), 0, s, Z_dev, zp, (long long)rows, l, LP));

  PcaArgs a{};
  a.X = X; a.center = center; a.scale = scale; a.M = LP != l ? zp : Z_dev;
  a.part = (double*)(ws.buf.get() + z_bytes);
  a.ld = ld; a.rows = rows; a.rows_per = rows_per; a.D = D;
  OSD_HIP(pca_launch(LP, false, aligned, dim3((unsigned)blocks, slabs), s, a));
  OSD_HIP(launched(pca_backproject_reduce, dim3((unsigned)(((long long)D * l + PCA_T - 1) / PCA_T)), dim3(PCA_T * PCA_PARTS), 0, s,
                   (const double*)a.part, blocks, chunk, D, LP, l, W_dev));
  OSD_HIP(hipStreamSynchronize(s));
  return OSD_OK;
}

}  // extern "C"
