// marginal.hip -- per-feature two-sample statistics over EVERY column of two device-resident cohorts:
//   osd_val_marginals   per feature the exact integer KS extremes, the Wasserstein-1 distance by quantile coupling, and the number
//                       of synthetic values below / above the real column's range.
//
// The columns go through in chunks, so the workspace is bounded whatever D is.  The chunked driver's state, the tile transposer
// (col_tiles<false>), the binary searches and the phase timer are the shared ones of val_columns.h; per chunk and cohort
//   col_tiles<false>   the [rows, chunk] column slice of the row-major matrix into column-major segments
//   seg_sort           segsort.h's four stable 8-bit passes: the segments come back sorted in place
// then one pass over both cohorts' sorted segments:
//   marg_stats       workgroup (x, f) owns elements [x R, (x + 1) R) of BOTH sorted columns of feature f (R = COL_RUN).
//                    KS: an element v that is the last of its value contributes d(v) = #{a <= v} n2 - #{b <= v} n1; its own count is
//                    its index + 1, the other cohort's count is an upper bound.  The upper bounds of a run's first and last value
//                    enclose every count the run can ask for: that window of the other cohort is staged in LDS and searched there
//                    (COL_WINDOW floats; a wider window -- heavy ties, or cohorts of very different length -- is searched in
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
#include "val_columns.h"

namespace osd {
namespace {

// auto chunk: the transposed and the sorted buffer of both cohorts together, 2 x 4 (n1 + n2) bytes per column, stay within this
// (the Infinity Cache's size; measured at 125 000 + 125 000 rows x 2000: 31.4 ms at 128 and at 256 columns, 244 and 488 MiB, against
// 35.2 ms at 64 and 40.0 ms at 512 -- DESIGN.md section 3.28), in whole tiles of the transposing gather
constexpr int64_t MARG_AUTO_BYTES = 256ll << 20;

struct MargArgs {
  const float* a; const float* b;          // sorted segments [chunk][n1], [chunk][n2]
  long long n1, n2;
  int blocks;                              // workgroups of a feature: ceil(max(n1, n2) / COL_RUN)
  long long* pmax; long long* pmin;        // [chunk][blocks]
  double* psum;                            // [chunk][blocks]
};

// The KS half for the run [i0, i1) of the sorted column x (nx values, the counts weighted wx) against the column y (ny values,
// weighted wy): d = sign (cnt_x wx - cnt_y wy) at every last-of-its-value element.  i0 < i1 <= nx.
template <int SIGN>
__device__ __forceinline__ void marg_ks_run(const float* __restrict__ x, long long nx, long long i0, long long i1, const float* __restrict__ y,
                                            long long ny, long long wx, long long wy, float* win, long long* ends, long long& mx,
                                            long long& mn) {
  if (threadIdx.x == 0) ends[0] = upper_bound(y, 0ll, ny, x[i0]);
  if (threadIdx.x == 64) ends[1] = upper_bound(y, 0ll, ny, x[i1 - 1]);
  __syncthreads();
  const long long lo = ends[0], hi = ends[1];                  // lo <= hi: x ascending
  const bool staged = hi - lo <= COL_WINDOW;                   // the same in the whole workgroup
  if (staged)
    for (int k = threadIdx.x; k < (int)(hi - lo); k += COL_THREADS) win[k] = y[lo + k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < COL_ITEMS; ++k) {
    const long long i = i0 + k * COL_THREADS + threadIdx.x;
    if (i >= i1) continue;
    const float v = x[i];
    if (i + 1 < nx && x[i + 1] == v) continue;                 // a later element carries this value
    const long long cy = staged ? lo + upper_bound(win, 0, (int)(hi - lo), v) : upper_bound(y, lo, hi, v);
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
  for (int k = 0; k < COL_ITEMS; ++k) {
    const long long i = i0 + k * COL_THREADS + threadIdx.x;
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

__global__ __launch_bounds__(COL_THREADS) void marg_stats(MargArgs g) {
  __shared__ float win[COL_WINDOW];
  __shared__ long long ends[2];
  __shared__ long long rmax[COL_THREADS / 64], rmin[COL_THREADS / 64];
  __shared__ double rsum[COL_THREADS / 64];
  const long long f = blockIdx.y;
  const float* a = g.a + f * g.n1;
  const float* b = g.b + f * g.n2;
  const long long i0 = (long long)blockIdx.x * COL_RUN;
  const long long a1 = min(g.n1, i0 + COL_RUN), b1 = min(g.n2, i0 + COL_RUN);
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
    for (int w = 1; w < COL_THREADS / 64; ++w) {
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
    out[3 * chunk + f] = lower_bound(b, 0ll, g.n2, a[0]);       // below: #{b < a_0}
  }
  if (lane == 1) out[4 * chunk + f] = g.n2 - upper_bound(b, 0ll, g.n2, a[g.n1 - 1]);      // above: #{b > a_last}
}

int marg_auto_chunk(int64_t n1, int64_t n2, int D) {
  int64_t c = MARG_AUTO_BYTES / (8 * (n1 + n2));
  if (c >= D) return D;
  if (c >= COL_TILE) c -= c % COL_TILE;
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
  if (n1 > 2000000000ll || n2 > 2000000000ll) { set_error("too many rows for one segmented sort"); return OSD_EINVAL; }
  OSD_HIP(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;

  ColumnChunks cc;
  OSD_TRY(cc.init(n1, n2, D, chunk_cols ? chunk_cols : marg_auto_chunk(n1, n2, D)));
  const int64_t chunk = cc.chunk, blocks = cc.blocks;
  ValBuf slots, res;
  OSD_TRY(slots.alloc((size_t)(3 * chunk * blocks) * 8));
  OSD_TRY(res.alloc((size_t)(5 * chunk) * 8));
  MargArgs g{};
  g.a = cc.ca; g.b = cc.cb; g.n1 = n1; g.n2 = n2; g.blocks = (int)blocks;
  g.pmax = slots.as<long long>(); g.pmin = g.pmax + chunk * blocks; g.psum = (double*)(g.pmin + chunk * blocks);
  std::vector<long long> host((size_t)(5 * chunk));
  PhaseClock<3, double> clock(phase_ms);                       // transpose, sort, statistics: summed over the chunks
  OSD_HIP(clock.init());

  for (int64_t c0 = 0; c0 < D; c0 += chunk) {
    const int c = (int)(D - c0 < chunk ? D - c0 : chunk);
    const unsigned cy = (unsigned)((c + COL_TILE - 1) / COL_TILE);
    OSD_HIP(clock.mark(0, s));
    OSD_HIP(launched(col_tiles<false>, dim3((unsigned)((n1 + COL_TILE - 1) / COL_TILE), cy), COL_THREADS, 0, s, real + c0, (long long)ld_real,
                     (long long)n1, c, nullptr, 0ll, 0ll, cc.ca, nullptr));
    OSD_HIP(launched(col_tiles<false>, dim3((unsigned)((n2 + COL_TILE - 1) / COL_TILE), cy), COL_THREADS, 0, s, synth + c0, (long long)ld_synth,
                     (long long)n2, c, nullptr, 0ll, 0ll, cc.cb, nullptr));
    OSD_HIP(clock.mark(1, s));
    OSD_TRY(cc.sort(s, c));
    OSD_HIP(clock.mark(2, s));
    OSD_HIP(launched(marg_stats, dim3((unsigned)blocks, (unsigned)c), COL_THREADS, 0, s, g));
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
