// cluster.hip -- per-label column sums of a device-resident cohort, in double and bit-reproducible:
//   osd_val_label_sums   sums[k][c] = sum over the rows with label k of X[r][c], the rows' count, and the per-label sum of a row value
// the update half of a Lloyd iteration (the assignment half is osd_val_nearest) and the per-subtype mean of any matrix.
//
// A work item is a contiguous block of rows times a slice of 64 columns, one wavefront, one lane per column.  The item's per-label
// accumulators are [K][64] doubles in LDS; a workgroup is LS_WAVES(K) such items side by side on the same rows, its LDS [K][T]
// doubles, and a lane only ever touches the K addresses of its own column: no barrier, no atomic.  The label of a row is the same
// in the whole wavefront (a scalar load and a scalar branch), so a row is one dword load per lane, one convert, and a plain
// read-modify-write  acc[label][lane] += (double)x  in row order.  The rows are loaded LS_ROWS at a time into one of two register
// sets: the next set's loads are in flight while this set's rows go through the LDS.  Each item then writes its [K][64] slab (nobody
// else touches it), and label_sums_reduce adds the row blocks' slabs as glm_reduce does: part p adds blocks p, p + 16, ... in that
// order, then the parts are added in part order.  Every addition is a double addition of a converted float, the order depends on
// (rows, D, K) alone -- there is ONE load path, by dwords, for every base address and every ld >= D -- so the same inputs give the
// same bits, and integer data below 2^53 in total is summed exactly.
// Lane k of the first wavefront of the first column block counts label k's rows of its row block and adds their row values.
#include <stdint.h>
#include <mutex>
#include "handle.h"
#include "val_common.h"

namespace osd {
namespace {

constexpr int LS_MAX_K = 64;
constexpr int LS_MAX_D = 8192;
constexpr int LS_MAX_BLOCKS = 256;       // row blocks of a call; at most the lanes of a label_sums_reduce workgroup
constexpr int LS_ROWS = 8;               // rows of a register set
constexpr int LS_RED_PARTS = 16;
constexpr int LS_MAX_DEVICES = 64;
static_assert(LS_MAX_BLOCKS <= 64 * LS_RED_PARTS, "label_sums_reduce stages one row block per lane");

// wavefronts of a workgroup: K x 64 doubles of LDS each, at most 64 KB together
constexpr int ls_waves(int K) { return K <= 32 ? 4 : 2; }
// rows of a row block: at least 16 K, so that the slabs ([blocks][K][D] doubles) stay below an eighth of the bytes of X
inline int64_t ls_rows_per(int64_t rows, int K) {
  const int64_t least = 16 * (int64_t)K, even = (rows + LS_MAX_BLOCKS - 1) / LS_MAX_BLOCKS;
  return least > even ? least : even;
}

struct LabelSumArgs {
  const float* X; const int32_t* labels; const float* value;
  double* slab;            // [blocks][K][D]
  long long* count_slab;   // [blocks][K]
  double* value_slab;      // [blocks][K]
  long long ld, rows, rows_per;
  int D, K;
};

__global__ __launch_bounds__(256) void label_sums_kernel(LabelSumArgs a) {
  extern __shared__ double acc[];                            // [K][T]
  const int tid = threadIdx.x, T = blockDim.x, lane = tid & 63;
  const int D = a.D, K = a.K;
  const int col = (int)blockIdx.x * T + tid;
  const bool in = col < D;
  const bool counter = blockIdx.x == 0 && tid < 64;          // the whole wavefront or none of it
  if (col - lane >= D && !counter) return;                   // a wavefront beyond the last column
  const long long blk = blockIdx.y;
  const long long r0 = blk * a.rows_per;
  const long long r1 = min(a.rows, r0 + a.rows_per);         // r0 < r1: the host launches no empty block
  for (int k = 0; k < K; ++k) acc[k * T + tid] = 0.0;
  long long cnt = 0;
  double vsum = 0.0;

  // Loads are unconditional, so that LS_ROWS of them are in flight together: a lane beyond D reads column D - 1 and never stores
  // its sums; a row beyond the block re-reads the block's last row and is not added.
  const int lcol = min(col, D - 1);
  auto load = [&](float (&xb)[LS_ROWS], int (&lb)[LS_ROWS], long long gr) {
#pragma unroll
    for (int i = 0; i < LS_ROWS; ++i) {
      const long long row = min(gr + i, r1 - 1);
      xb[i] = a.X[(size_t)row * (size_t)a.ld + lcol];
      lb[i] = a.labels[row];                                 // the same in the whole workgroup: a scalar load
    }
  };
  auto process = [&](const float (&xb)[LS_ROWS], const int (&lb)[LS_ROWS], long long gr) {
#pragma unroll
    for (int i = 0; i < LS_ROWS; ++i) {
      if (gr + i >= r1) break;                               // the same in the whole workgroup, as is the next line
      const int lab = lb[i];
      if ((unsigned)lab >= (unsigned)K) continue;            // a row outside [0, K) adds to nothing
      double* p = acc + lab * T + tid;
      *p = *p + (double)xb[i];
      if (counter && lab == lane) {
        ++cnt;
        if (a.value) vsum += (double)a.value[gr + i];
      }
    }
  };

  float x0[LS_ROWS], x1[LS_ROWS];
  int l0[LS_ROWS], l1[LS_ROWS];
  load(x0, l0, r0);
  for (long long gr = r0; gr < r1; gr += 2 * LS_ROWS) {
    const bool second = gr + LS_ROWS < r1;
    if (second) load(x1, l1, gr + LS_ROWS);
    process(x0, l0, gr);
    if (second) {
      if (gr + 2 * LS_ROWS < r1) load(x0, l0, gr + 2 * LS_ROWS);
      process(x1, l1, gr + LS_ROWS);
    }
  }

  if (in)
    for (int k = 0; k < K; ++k) a.slab[((size_t)blk * K + k) * (size_t)D + col] = acc[k * T + tid];
  if (counter && lane < K) {
    a.count_slab[(size_t)blk * K + lane] = cnt;
    if (a.value) a.value_slab[(size_t)blk * K + lane] = vsum;
  }
}

// sums[k][col] = the row blocks' slabs added: 64 columns x 16 parts per workgroup, part p adds blocks p, p + 16, ... in that order,
// then the parts are added in part order.  Workgroup (0, k) also adds label k's counts and value sums in block order.
__global__ __launch_bounds__(64 * LS_RED_PARTS) void label_sums_reduce(const double* __restrict__ slab, const long long* __restrict__ count_slab,
                                                                       const double* __restrict__ value_slab, int blocks, int K, int D,
                                                                       double* __restrict__ sums, long long* __restrict__ counts,
                                                                       double* __restrict__ value_sums) {
  __shared__ double part[LS_RED_PARTS][64];
  const int cx = threadIdx.x & 63, p = threadIdx.x >> 6;
  const int k = blockIdx.y, col = blockIdx.x * 64 + cx;
  double s = 0.0;
  if (col < D) {
#pragma unroll 8                                             // eight loads in flight, added in the same order
    for (int b = p; b < blocks; b += LS_RED_PARTS) s += slab[((size_t)b * K + k) * (size_t)D + col];
  }
  part[p][cx] = s;
  __syncthreads();
  if (p == 0 && col < D) {
    double t = part[0][cx];
    for (int q = 1; q < LS_RED_PARTS; ++q) t += part[q][cx];
    sums[(size_t)k * D + col] = t;
  }
  if (blockIdx.x == 0) {                                       // the same in the whole workgroup
    // one load per lane into LDS, then one lane adds in block order: a lane that walked the slab itself would wait for every load
    __shared__ long long cn[LS_MAX_BLOCKS];
    __shared__ double vv[LS_MAX_BLOCKS];
    const int t = threadIdx.x;
    if (t < blocks) {
      cn[t] = count_slab[(size_t)t * K + k];
      vv[t] = value_sums ? value_slab[(size_t)t * K + k] : 0.0;
    }
    __syncthreads();
    if (t == 0) {
      long long n = 0;
      double v = 0.0;
      for (int b = 0; b < blocks; ++b) { n += cn[b]; v += vv[b]; }
      counts[k] = n;
      if (value_sums) value_sums[k] = v;
    }
  }
}

// One grow-only workspace per device, held for the length of a call: a k-means fit calls osd_val_label_sums once per iteration.
struct Workspace {
  std::mutex mu;
  DevBuf<char> buf;
};
Workspace* const g_ws = new Workspace[LS_MAX_DEVICES];       // never destroyed: no hipFree from a static destructor at process exit

}  // namespace
}  // namespace osd

using namespace osd;

extern "C" {

int osd_val_label_sums(void* stream, int device, const float* X, int64_t rows, int ld, int D, const int32_t* labels, int K,
                       const float* value, double* sums_dev, int64_t* counts_dev, double* value_sums_dev) {
  if (!X || !labels || !sums_dev || !counts_dev || rows < 1 || D < 1 || D > LS_MAX_D || ld < D || K < 1 || K > LS_MAX_K || device < 0 ||
      device >= LS_MAX_DEVICES) {
    set_error("bad argument (rows >= 1, 1 <= D <= 8192, ld >= D, 1 <= K <= 64, labels, sums and counts not NULL)");
    return OSD_EINVAL;
  }
  if ((value == nullptr) != (value_sums_dev == nullptr)) {
    set_error("bad argument (value and value_sums_dev: both or neither)");
    return OSD_EINVAL;
  }
  OSD_HIP(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;

  // the partition: a function of (rows, D, K) alone
  const int64_t rows_per = ls_rows_per(rows, K);
  const unsigned blocks = (unsigned)((rows + rows_per - 1) / rows_per);
  const unsigned T = 64u * (unsigned)ls_waves(K);
  LabelSumArgs a{};
  a.X = X; a.labels = labels; a.value = value;
  a.ld = ld; a.rows = rows; a.rows_per = rows_per; a.D = D; a.K = K;

  Workspace& ws = g_ws[device];
  std::lock_guard<std::mutex> hold(ws.mu);
  const size_t slab_bytes = (size_t)blocks * K * D * sizeof(double), small_bytes = (size_t)blocks * K * 8;
  OSD_TRY(ws.buf.reserve((int64_t)(slab_bytes + 2 * small_bytes)));
  a.slab = (double*)ws.buf.get();
  a.count_slab = (long long*)(ws.buf.get() + slab_bytes);
  a.value_slab = (double*)(ws.buf.get() + slab_bytes + small_bytes);

  OSD_HIP(launched(label_sums_kernel, dim3((unsigned)((D + T - 1) / T), blocks), dim3(T), (size_t)K * T * sizeof(double), s, a));
  OSD_HIP(launched(label_sums_reduce, dim3((unsigned)((D + 63) / 64), (unsigned)K), dim3(64 * LS_RED_PARTS), 0, s, (const double*)a.slab,
                   (const long long*)a.count_slab, (const double*)a.value_slab, (int)blocks, K, D, sums_dev, (long long*)counts_dev,
                   value_sums_dev));
  OSD_HIP(hipStreamSynchronize(s));
  return OSD_OK;
}

}  // extern "C"
