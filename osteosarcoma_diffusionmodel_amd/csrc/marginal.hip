// marginal.hip -- per-feature two-sample statistics over EVERY column of two device-resident cohorts:
//   osd_val_marginals   per feature the exact integer KS extremes, the Wasserstein-1 distance by quantile coupling, and the number
//                       of synthetic values below / above the real column's range.
//
// The columns go through in chunks, so the workspace is bounded whatever D is.  Per chunk and cohort:
//   marg_transpose   the [rows, chunk] column slice of the row-major matrix (any ld, any base alignment: dword loads only) through a
//                    64 x 64 LDS tile into column-major segments -- the global reads run along a row, the writes along a segment
//   segsort.h        the four stable 8-bit passes, as osd_val_ks_extremes runs them: the segments come back sorted in place
// then one pass over both cohorts' sorted segments:
//   marg_stats       workgroup (x, f) owns elements [x R, (x + 1) R) of BOTH sorted columns of feature f (R = MARG_RUN).
//                    KS: an element v that is the last of its value contributes d(v) = #{a <= v} n2 - #{b <= v} n1; its own count is
//                    its index + 1, the other cohort's count is an upper bound.  The upper bounds of a run's first and last value
//                    enclose every count the run can ask for: that window of the other cohort is staged in LDS and searched there
//                    (MARG_WINDOW floats; a wider window -- heavy ties, or cohorts of very different length -- is searched in
//                    global memory, between the same two ends).
//                    W1: element i of the LONGER cohort meets partners floor(i nS / nL) .. floor(((i + 1) nS - 1) / nL) of the
//                    shorter one, at most two, with the exact integer weight min((i + 1) nS, (j + 1) nL) - max(i nS, j nL);
//                    |difference| and the products in double, summed per lane in index order, over the wavefront by the xor
//                    butterfly, over the four wavefronts in order.
//                    One slot per workgroup for the sum and the two extremes: no atomic of any kind.
//   marg_finish      one wavefront per feature: the slots in a fixed order, and the two range counts from searches at the ends.
// The partition of a feature's elements depends on (n1, n2) alone, so the results have the same bits at every chunk size.
#include <limits.h>
#include <stdint.h>
#include <string.h>
#include <vector>
#include <hip/hip_runtime.h>
#include "handle.h"
#include "val_common.h"

// segsort.h defines its kernels at namespace scope and validate.hip instantiates them already: this translation unit's copies live
// in a namespace of their own, so that the two objects link.
namespace osd { namespace marg {
#include "segsort.h"
} }

namespace osd {
namespace {

namespace seg = marg::osd;

constexpr int MARG_TILE = 64;              // rows and columns of a transposed tile
constexpr int MARG_THREADS = 256;
constexpr int MARG_ITEMS = 4;              // elements of a run per lane
constexpr int MARG_RUN = MARG_THREADS * MARG_ITEMS;
constexpr int MARG_WINDOW = 4096;          // floats of the other cohort a workgroup stages in LDS
constexpr int MARG_MAX_CHUNK = 32768;      // columns of a chunk: the sort's grid.y
// auto chunk: the transposed and the sorted buffer of both cohorts together, 2 x 4 (n1 + n2) bytes per column, stay within this
// (the Infinity Cache's size; measured at 125 000 + 125 000 rows x 2000: 31.4 ms at 128 and at 256 columns, 244 and 488 MiB, against
// 35.2 ms at 64 and 40.0 ms at 512 -- DESIGN.md section 3.28), in whole tiles of the transposing gather
constexpr int64_t MARG_AUTO_BYTES = 256ll << 20;

// dst[c][r] = src[r][c0 + c] for c < cols
__global__ __launch_bounds__(MARG_THREADS) void marg_transpose(const float* __restrict__ src, long long ld, long long rows, int cols,
                                                               float* __restrict__ dst) {
  __shared__ float tile[MARG_TILE][MARG_TILE + 1];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const long long r0 = (long long)blockIdx.x * MARG_TILE;
  const int c0 = (int)blockIdx.y * MARG_TILE;
  if (c0 + tx < cols)
    for (int y = ty; y < MARG_TILE; y += MARG_THREADS / 64)
      if (r0 + y < rows) tile[y][tx] = src[(r0 + y) * ld + c0 + tx];
  __syncthreads();
  if (r0 + tx < rows)
    for (int y = ty; y < MARG_TILE; y += MARG_THREADS / 64)
      if (c0 + y < cols) dst[(long long)(c0 + y) * rows + r0 + tx] = tile[tx][y];
}

// the first index in [lo, hi) whose value exceeds v, else hi (p ascending)
__device__ __forceinline__ long long marg_upper(const float* __restrict__ p, long long lo, long long hi, float v) {
  while (lo < hi) { const long long mid = (lo + hi) >> 1; if (p[mid] <= v) lo = mid + 1; else hi = mid; }
  return lo;
}
__device__ __forceinline__ int marg_upper_lds(const float* w, int n, float v) {
  int lo = 0, hi = n;
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (w[mid] <= v) lo = mid + 1; else hi = mid; }
  return lo;
}

struct MargArgs {
  const float* a; const float* b;          // sorted segments [chunk][n1], [chunk][n2]
  long long n1, n2;
  int blocks;                              // workgroups of a feature: ceil(max(n1, n2) / MARG_RUN)
  long long* pmax; long long* pmin;        // [chunk][blocks]
  double* psum;                            // [chunk][blocks]
};

// The KS half for the run [i0, i1) of the sorted column x (nx values, the counts weighted wx) against the column y (ny values,
// weighted wy): d = sign (cnt_x wx - cnt_y wy) at every last-of-its-value element.  i0 < i1 <= nx.
template <int SIGN>
__device__ __forceinline__ void marg_ks_run(const float* __restrict__ x, long long nx, long long i0, long long i1, const float* __restrict__ y,
                                            long long ny, long long wx, long long wy, float* win, long long* ends, long long& mx,
                                            long long& mn) {
  if (threadIdx.x == 0) ends[0] = marg_upper(y, 0, ny, x[i0]);
  if (threadIdx.x == 64) ends[1] = marg_upper(y, 0, ny, x[i1 - 1]);
  __syncthreads();
  const long long lo = ends[0], hi = ends[1];                  // lo <= hi: x ascending
  const bool staged = hi - lo <= MARG_WINDOW;                  // the same in the whole workgroup
  if (staged)
    for (int k = threadIdx.x; k < (int)(hi - lo); k += MARG_THREADS) win[k] = y[lo + k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < MARG_ITEMS; ++k) {
    const long long i = i0 + k * MARG_THREADS + threadIdx.x;
    if (i >= i1) continue;
    const float v = x[i];
    if (i + 1 < nx && x[i + 1] == v) continue;                 // a later element carries this value
    const long long cy = staged ? lo + marg_upper_lds(win, (int)(hi - lo), v) : marg_upper(y, lo, hi, v);
    const long long d = SIGN * ((i + 1) * wx - cy * wy);
    mx = d > mx ? d : mx;
    mn = d < mn ? d : mn;
  }
  __syncthreads();                                             // win and ends are free again
}

// sum over the run [i0, i1) of the longer column l (nl values) of |l_i - s_j| w_ij against the shorter column s (ns <= nl values)
__device__ __forceinline__ double marg_w1_run(const float* __restrict__ l, long long nl, long long i0, long long i1, const float* __restrict__ s,
                                              long long ns) {
  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < MARG_ITEMS; ++k) {
    const long long i = i0 + k * MARG_THREADS + threadIdx.x;
    if (i >= i1) continue;
    const double v = (double)l[i];
    const long long p0 = i * ns, p1 = p0 + ns;                 // [i ns, (i + 1) ns): this element's share of the n1 n2 grid
    const long long j0 = p0 / nl, j1 = (p1 - 1) / nl;          // j0 <= j1 <= ns - 1, at most two partners
    for (long long j = j0; j <= j1; ++j) {
      const long long q0 = j * nl, q1 = q0 + nl;
      const long long w = (p1 < q1 ? p1 : q1) - (p0 > q0 ? p0 : q0);
      acc += fabs(v - (double)s[j]) * (double)w;
    }
  }
  return acc;
}

__global__ __launch_bounds__(MARG_THREADS) void marg_stats(MargArgs g) {
  __shared__ float win[MARG_WINDOW];
  __shared__ long long ends[2];
  __shared__ long long rmax[MARG_THREADS / 64], rmin[MARG_THREADS / 64];
  __shared__ double rsum[MARG_THREADS / 64];
  const long long f = blockIdx.y;
  const float* a = g.a + f * g.n1;
  const float* b = g.b + f * g.n2;
  const long long i0 = (long long)blockIdx.x * MARG_RUN;
  const long long a1 = min(g.n1, i0 + MARG_RUN), b1 = min(g.n2, i0 + MARG_RUN);
  long long mx = LLONG_MIN, mn = LLONG_MAX;
  // every condition below is the same in the whole workgroup: the barriers inside marg_ks_run are met by all or by none
  if (i0 < g.n1) marg_ks_run<1>(a, g.n1, i0, a1, b, g.n2, g.n2, g.n1, win, ends, mx, mn);
  if (i0 < g.n2) marg_ks_run<-1>(b, g.n2, i0, b1, a, g.n1, g.n1, g.n2, win, ends, mx, mn);
  double sum = g.n1 >= g.n2 ? marg_w1_run(a, g.n1, i0, a1, b, g.n2) : marg_w1_run(b, g.n2, i0, b1, a, g.n1);
  wave_max(mx);
  wave_min(mn);
  wave_sum(sum);
  const int wv = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { rmax[wv] = mx; rmin[wv] = mn; rsum[wv] = sum; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < MARG_THREADS / 64; ++w) {
      mx = rmax[w] > mx ? rmax[w] : mx;
      mn = rmin[w] < mn ? rmin[w] : mn;
      sum += rsum[w];
    }
    const long long slot = f * g.blocks + blockIdx.x;
    g.pmax[slot] = mx; g.pmin[slot] = mn; g.psum[slot] = sum;
  }
}

// One wavefront per feature.  out: five arrays of `chunk` 8-byte values -- dmax, dmin (long long), the W1 sum (double), below, above
__global__ __launch_bounds__(64) void marg_finish(MargArgs g, int chunk, long long* out) {
  const int f = blockIdx.x, lane = threadIdx.x;
  long long mx = LLONG_MIN, mn = LLONG_MAX;
  double sum = 0.0;
  for (int k = lane; k < g.blocks; k += 64) {                   // lane order, then the butterfly: fixed by (n1, n2)
    const long long slot = (long long)f * g.blocks + k;
    mx = g.pmax[slot] > mx ? g.pmax[slot] : mx;
    mn = g.pmin[slot] < mn ? g.pmin[slot] : mn;
    sum += g.psum[slot];
  }
  wave_max(mx);
  wave_min(mn);
  wave_sum(sum);
  const float* a = g.a + (long long)f * g.n1;
  const float* b = g.b + (long long)f * g.n2;
  if (lane == 0) {
    out[f] = mx;
    out[chunk + f] = mn;
    ((double*)out)[2 * chunk + f] = sum;
    const float first = a[0];                                  // below: #{b < a_0}, a lower bound
    long long lo = 0, hi = g.n2;
    while (lo < hi) { const long long mid = (lo + hi) >> 1; if (b[mid] < first) lo = mid + 1; else hi = mid; }
    out[3 * chunk + f] = lo;
  }
  if (lane == 1) out[4 * chunk + f] = g.n2 - marg_upper(b, 0, g.n2, a[g.n1 - 1]);      // above: #{b > a_last}
}

// the four passes of segsort.h over `nf` segments of n keys, ping-pong between buf0 and buf1: sorted floats back in buf0
int marg_sort(hipStream_t s, float* buf0, float* buf1, long long n, int nf, int* cnt) {
  const int wps = (int)((n + seg::SEG_CHUNK - 1) / seg::SEG_CHUNK);
  uint32_t* a = (uint32_t*)buf0; uint32_t* b = (uint32_t*)buf1;
  const dim3 grid((unsigned)((wps + seg::SEG_WAVES - 1) / seg::SEG_WAVES), (unsigned)nf), block(64 * seg::SEG_WAVES);
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 8 * pass;
    OSD_HIP(launched(pass == 0 ? seg::k_seg_count<true> : seg::k_seg_count<false>, grid, block, 0, s, (const uint32_t*)a, n, wps, shift, cnt));
    OSD_HIP(launched(seg::k_seg_scan, dim3((unsigned)nf), dim3(256), 0, s, cnt, wps));
    OSD_HIP(launched(pass == 0 ? seg::k_seg_scatter<true, false> : pass == 3 ? seg::k_seg_scatter<false, true> : seg::k_seg_scatter<false, false>,
                     grid, block, 0, s, (const uint32_t*)a, b, n, wps, shift, (const int*)cnt));
    uint32_t* t = a; a = b; b = t;
  }
  return OSD_OK;
}

struct PhaseClock {                        // optional: milliseconds of the three phases, summed over the chunks
  double* ms;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  explicit PhaseClock(double* out) : ms(out) {}
  ~PhaseClock() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
  hipError_t init() {
    if (!ms) return hipSuccess;
    ms[0] = ms[1] = ms[2] = 0.0;
    for (hipEvent_t& e : ev) { const hipError_t r = hipEventCreate(&e); if (r != hipSuccess) return r; }
    return hipSuccess;
  }
  hipError_t mark(int i, hipStream_t s) { return ms ? hipEventRecord(ev[i], s) : hipSuccess; }
  hipError_t add() {                       // after the stream has drained
    if (!ms) return hipSuccess;
    for (int i = 0; i < 3; ++i) {
      float t = 0.f;
      const hipError_t r = hipEventElapsedTime(&t, ev[i], ev[i + 1]);
      if (r != hipSuccess) return r;
      ms[i] += t;
    }
    return hipSuccess;
  }
};

int marg_auto_chunk(int64_t n1, int64_t n2, int D) {
  int64_t c = MARG_AUTO_BYTES / (8 * (n1 + n2));
  if (c >= D) return D;
  if (c >= MARG_TILE) c -= c % MARG_TILE;
  return (int)(c < 1 ? 1 : c);
}

int marginals(void* stream, int device, const float* real, int64_t n1, int ld_real, const float* synth, int64_t n2, int ld_synth, int D,
              int chunk_cols, int64_t* ks_dmax, int64_t* ks_dmin, double* w1, int64_t* below, int64_t* above, double* phase_ms) {
  if (!real || !synth || !ks_dmax || !ks_dmin || !w1 || !below || !above) { set_error("bad argument (NULL pointer)"); return OSD_EINVAL; }
  if (n1 < 1 || n2 < 1 || D < 1 || ld_real < D || ld_synth < D || chunk_cols < 0) {
    set_error("bad argument (n1, n2, D >= 1, ld_real, ld_synth >= D, chunk_cols >= 0)");
    return OSD_EINVAL;
  }
  if (n1 > (1ll << 53) / n2) { set_error("n1 * n2 exceeds 2^53: the integer weights would not convert to double exactly"); return OSD_EINVAL; }
  const int64_t nmax = n1 > n2 ? n1 : n2;
  if (nmax > 2000000000ll) { set_error("too many rows for one segmented sort"); return OSD_EINVAL; }
  int64_t chunk = chunk_cols ? chunk_cols : marg_auto_chunk(n1, n2, D);
  if (chunk > D) chunk = D;
  if (chunk > MARG_MAX_CHUNK) chunk = MARG_MAX_CHUNK;
  if (chunk > 2000000000ll / nmax) chunk = 2000000000ll / nmax;          // segsort's keys per sort; >= 1 by the check above
  OSD_HIP(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;

  const int64_t blocks = (nmax + MARG_RUN - 1) / MARG_RUN;
  const int wps = (int)((nmax + seg::SEG_CHUNK - 1) / seg::SEG_CHUNK);
  ValBuf keys, counts, slots, res;
  OSD_TRY(keys.alloc((size_t)(2 * (n1 + n2) * chunk) * sizeof(float)));
  OSD_TRY(counts.alloc((size_t)chunk * 256 * (size_t)wps * sizeof(int)));
  OSD_TRY(slots.alloc((size_t)(3 * chunk * blocks) * 8));
  OSD_TRY(res.alloc((size_t)(5 * chunk) * 8));
  float* ca = keys.as<float>(); float* ta = ca + n1 * chunk;
  float* cb = ta + n1 * chunk;  float* tb = cb + n2 * chunk;
  MargArgs g{};
  g.a = ca; g.b = cb; g.n1 = n1; g.n2 = n2; g.blocks = (int)blocks;
  g.pmax = slots.as<long long>(); g.pmin = g.pmax + chunk * blocks; g.psum = (double*)(g.pmin + chunk * blocks);
  std::vector<long long> host((size_t)(5 * chunk));
  PhaseClock clock(phase_ms);
  OSD_HIP(clock.init());

  for (int64_t c0 = 0; c0 < D; c0 += chunk) {
    const int c = (int)(D - c0 < chunk ? D - c0 : chunk);
    const unsigned cy = (unsigned)((c + MARG_TILE - 1) / MARG_TILE);
    OSD_HIP(clock.mark(0, s));
    OSD_HIP(launched(marg_transpose, dim3((unsigned)((n1 + MARG_TILE - 1) / MARG_TILE), cy), MARG_THREADS, 0, s, real + c0, (long long)ld_real,
                     (long long)n1, c, ca));
    OSD_HIP(launched(marg_transpose, dim3((unsigned)((n2 + MARG_TILE - 1) / MARG_TILE), cy), MARG_THREADS, 0, s, synth + c0, (long long)ld_synth,
                     (long long)n2, c, cb));
    OSD_HIP(clock.mark(1, s));
    OSD_TRY(marg_sort(s, ca, ta, (long long)n1, c, counts.as<int>()));
    OSD_TRY(marg_sort(s, cb, tb, (long long)n2, c, counts.as<int>()));
    OSD_HIP(clock.mark(2, s));
    OSD_HIP(launched(marg_stats, dim3((unsigned)blocks, (unsigned)c), MARG_THREADS, 0, s, g));
    OSD_HIP(launched(marg_finish, dim3((unsigned)c), 64, 0, s, g, (int)chunk, res.as<long long>()));
    OSD_HIP(clock.mark(3, s));
    OSD_HIP(read_back(s, host.data(), res.get(), (size_t)(5 * chunk) * 8));
    OSD_HIP(clock.add());
    const double scale = (double)n1 * (double)n2;
    for (int f = 0; f < c; ++f) {
      ks_dmax[c0 + f] = host[f];
      ks_dmin[c0 + f] = host[chunk + f];
      double sum;
      memcpy(&sum, &host[2 * chunk + f], sizeof(double));
      w1[c0 + f] = sum / scale;
      below[c0 + f] = host[3 * chunk + f];
      above[c0 + f] = host[4 * chunk + f];
    }
  }
  return OSD_OK;
}

}  // namespace
}  // namespace osd

using namespace osd;

extern "C" {

int osd_val_marginals(void* stream, int device, const float* real, int64_t n1, int ld_real, const float* synth, int64_t n2, int ld_synth,
                      int D, int chunk_cols, int64_t* ks_dmax, int64_t* ks_dmin, double* w1, int64_t* below, int64_t* above) {
  return marginals(stream, device, real, n1, ld_real, synth, n2, ld_synth, D, chunk_cols, ks_dmax, ks_dmin, w1, below, above, nullptr);
}

int osd_val_marginals_timed(void* stream, int device, const float* real, int64_t n1, int ld_real, const float* synth, int64_t n2,
                            int ld_synth, int D, int chunk_cols, int64_t* ks_dmax, int64_t* ks_dmin, double* w1, int64_t* below,
                            int64_t* above, double* phase_ms) {
  if (!phase_ms) { set_error("bad argument (NULL pointer)"); return OSD_EINVAL; }
  return marginals(stream, device, real, n1, ld_real, synth, n2, ld_synth, D, chunk_cols, ks_dmax, ks_dmin, w1, below, above, phase_ms);
}

int osd_val_marginals_auto_chunk(int64_t n1, int64_t n2, int D) {
  if (n1 < 1 || n2 < 1 || D < 1) { set_error("bad argument"); return OSD_EINVAL; }
  return marg_auto_chunk(n1, n2, D);
}

}  // extern "C"
