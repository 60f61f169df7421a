// val_columns.h -- what the validator's sort-based statistics share (marginal.hip, diffexp.hip; the searches and the phase timer also
// gsea.hip, pathway.hip and validate.hip): the tile transposer that turns a column slice of a row-major matrix into column-major
// segments, the binary searches over ascending data, the optional phase timer, and the chunked driver's state for two groups of
// column segments that segsort.h sorts.  The statistics themselves -- kernels, result layouts, host unpacking -- stay in their files.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "handle.h"
#include "segsort.h"
#include "val_common.h"

namespace osd {

constexpr int COL_TILE = 64;               // rows and columns of a transposed tile
constexpr int COL_THREADS = 256;
constexpr int COL_ITEMS = 4;               // elements of a run per lane
constexpr int COL_RUN = COL_THREADS * COL_ITEMS;       // elements of a sorted column a workgroup of the statistics kernels owns
constexpr int COL_WINDOW = 4096;           // floats of the other group a workgroup stages in LDS
constexpr int COL_MAX_CHUNK = 32768;       // columns of a chunk: the sort's grid.y

// The [rows, cols] slice src[r][c] of a row-major matrix (any ld, any base alignment: dword loads only) through a 64 x 64 LDS tile into
// column-major segments: the global reads run along a row, the writes along a segment.  grid (ceil(rows / 64), ceil(cols / 64)).
// Unmapped: row r of column c goes to dstA[c][r]; slot_of, na, nb and dstB are not read.  Mapped: slot_of[r] (made by the host: -1 or
// in [0, na + nb)) sends row r to dstA[c][slot] (na rows a segment), to dstB[c][slot - na] (nb rows) or nowhere.
template <bool MAPPED>
__global__ __launch_bounds__(COL_THREADS) void col_tiles(const float* __restrict__ src, long long ld, long long rows, int cols,
                                                         const int* __restrict__ slot_of, long long na, long long nb,
                                                         float* __restrict__ dstA, float* __restrict__ dstB) {
  __shared__ float tile[COL_TILE][COL_TILE + 1];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const long long r0 = (long long)blockIdx.x * COL_TILE;
  const int c0 = (int)blockIdx.y * COL_TILE;
  if (c0 + tx < cols)
    for (int y = ty; y < COL_TILE; y += COL_THREADS / 64)
      if (r0 + y < rows) tile[y][tx] = src[(r0 + y) * ld + c0 + tx];
  __syncthreads();
  if constexpr (MAPPED) {
    if (r0 + tx >= rows) return;
    const long long slot = slot_of[r0 + tx];
    if (slot < 0) return;
    const bool is_a = slot < na;
    float* dst = is_a ? dstA + slot : dstB + (slot - na);
    const long long n = is_a ? na : nb;
    for (int y = ty; y < COL_TILE; y += COL_THREADS / 64)
      if (c0 + y < cols) dst[(long long)(c0 + y) * n] = tile[tx][y];
  } else {
    if (r0 + tx < rows)
      for (int y = ty; y < COL_TILE; y += COL_THREADS / 64)
        if (c0 + y < cols) dstA[(long long)(c0 + y) * rows + r0 + tx] = tile[tx][y];
  }
}

// p ascending (global memory or LDS).  lower_bound: the first index in [lo, hi) whose value is not below v, else hi; upper_bound: the
// first whose value exceeds v, else hi.  With lo = 0 they are #{p < v} and #{p <= v}.
template <class I, class T> __device__ __forceinline__ I lower_bound(const T* p, I lo, I hi, T v) {
  while (lo < hi) { const I mid = (lo + hi) >> 1; if (p[mid] < v) lo = mid + 1; else hi = mid; }
  return lo;
}
template <class I, class T> __device__ __forceinline__ I upper_bound(const T* p, I lo, I hi, T v) {
  while (lo < hi) { const I mid = (lo + hi) >> 1; if (p[mid] <= v) lo = mid + 1; else hi = mid; }
  return lo;
}

// Optional: milliseconds of N consecutive phases between N + 1 events into ms (float or double; NULL: every call is a no-op).
// mark(i) opens phase i (and closes phase i - 1); add(), once the stream has drained, adds every phase to ms, so a driver that
// goes through chunks ends with the sums and one that marks once with the times themselves.
template <int N, class T> struct PhaseClock {
  T* ms;
  hipEvent_t ev[N + 1] = {};
  explicit PhaseClock(T* out) : ms(out) {}
  ~PhaseClock() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
  hipError_t init() {
    if (!ms) return hipSuccess;
    for (int i = 0; i < N; ++i) ms[i] = 0;
    for (hipEvent_t& e : ev) { const hipError_t r = hipEventCreate(&e); if (r != hipSuccess) return r; }
    return hipSuccess;
  }
  hipError_t mark(int i, hipStream_t s) { return ms ? hipEventRecord(ev[i], s) : hipSuccess; }
  hipError_t add() {
    if (!ms) return hipSuccess;
    for (int i = 0; i < N; ++i) {
      float t = 0.f;
      const hipError_t r = hipEventElapsedTime(&t, ev[i], ev[i + 1]);
      if (r != hipSuccess) return r;
      ms[i] += t;
    }
    return hipSuccess;
  }
};

// The state of a driver that takes D columns through in chunks, each chunk as two groups of column-major segments (na and nb rows
// a column) that are sorted in place.  keys holds, per group, the segments and the sort's second buffer: ca, ta, cb, tb.
struct ColumnChunks {
  int64_t na = 0, nb = 0, chunk = 0;       // chunk: columns at a time, the same for every chunk but the last
  int64_t blocks = 0;                      // workgroups of a column in the statistics kernels: ceil(max(na, nb) / COL_RUN)
  ValBuf keys, counts;
  float *ca = nullptr, *ta = nullptr, *cb = nullptr, *tb = nullptr;

  // want: the caller's chunk (> 0), clamped to D, to the sort's grid and to segsort's 2e9 keys per sort (1 <= na, nb <= 2e9)
  int init(int64_t na_, int64_t nb_, int D, int64_t want) {
    na = na_; nb = nb_;
    const int64_t nmax = na > nb ? na : nb;
    chunk = want;
    if (chunk > D) chunk = D;
    if (chunk > COL_MAX_CHUNK) chunk = COL_MAX_CHUNK;
    if (chunk > 2000000000ll / nmax) chunk = 2000000000ll / nmax;
    blocks = (nmax + COL_RUN - 1) / COL_RUN;
    OSD_TRY(keys.alloc((size_t)(2 * (na + nb) * chunk) * sizeof(float)));
    OSD_TRY(counts.alloc(seg_count_bytes(nmax, (int)chunk)));
    ca = keys.as<float>(); ta = ca + na * chunk;
    cb = ta + na * chunk;  tb = cb + nb * chunk;
    return OSD_OK;
  }
  // both groups of a chunk of c columns: sorted floats back in ca and cb
  int sort(hipStream_t s, int c) {
    OSD_TRY(seg_sort(s, ca, ta, (long long)na, c, counts.as<int>()));
    return seg_sort(s, cb, tb, (long long)nb, c, counts.as<int>());
  }
};

}  // namespace osd
