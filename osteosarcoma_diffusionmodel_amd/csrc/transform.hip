// transform.hip -- per-feature maps between data units and model units, forward and inverse:
//   osd_xf_apply   dst[r][f] = map_f(src[r][f]), map_f one of identity, standard (centre and scale) and quantile_normal (a monotone
//                  piecewise-linear map between the column's knots and one shared table of normal levels)
//
// A workgroup owns a strip of XF_STRIP = 32 columns (one 128-byte line per row) and a chunk of rows.  It stages the strip's knots in
// LDS once, transposed to [Q][32]: lane c of a 32-lane group reads word q * 32 + c, bank c, whatever q its own search has reached, so
// a knot read never has a bank conflict (ds_read_b32 banks by dword address mod 32 within each half of a wavefront, and the two
// halves of a wavefront are two rows of the same 32 columns).  The level table is shared by all columns and is searched by the
// inverse map with a different index per lane: entry i sits at word i + (i >> 5), which sends the midpoints of the first five
// search steps (multiples of Q / 2^d, at Q = 1024 all on one bank) to different banks.  The 1024 lanes of a workgroup are 32 rows of
// the strip; a lane takes XF_ILP rows at a time, runs their searches side by side (independent chains of dependent LDS reads) while
// the loads of its next XF_ILP rows are in flight, and stores them: one read and one write of the matrix.  An output is a function
// of its own input and of its column's tables alone: no atomics, nothing shared between workgroups, no dependence on the launch
// geometry, and src == dst works because an element is read and written by the same lane.
#include <stdint.h>
#include <vector>
#include "handle.h"
#include "val_common.h"

namespace osd {
namespace {

constexpr int XF_STRIP = 32;             // columns of a workgroup: 128 bytes of a row
constexpr int XF_THREADS = 1024;         // 32 rows x 32 columns
constexpr int XF_ROWS = XF_THREADS / XF_STRIP;
constexpr int XF_ILP = 8;                // rows a lane searches side by side (and as many loads in flight for the next set)
constexpr int XF_MAX_Q = 1024;
constexpr int XF_MIN_ROWS_PER = 512;     // rows of a chunk, at least: the strip's tables are Q rows' worth of reads
constexpr int XF_TARGET_WGS = 2048;      // about eight workgroups per CU over the whole call
constexpr int XF_MAX_DEVICES = 64;
constexpr int XF_KIND_IDENTITY = 0, XF_KIND_STANDARD = 1, XF_KIND_QUANTILE = 2;

__host__ __device__ constexpr int xf_level_slot(int i) { return i + (i >> 5); }
// words of the level table, a whole number of 32-word rows: the knot image behind it keeps bank = column, and the row below a column's
// first knot -- where the knot search starts from -- is an LDS address like any other
__host__ __device__ constexpr int xf_level_words(int Q) { return (xf_level_slot(Q - 1) + XF_STRIP) / XF_STRIP * XF_STRIP; }
constexpr size_t xf_lds_bytes(int Q) { return ((size_t)Q * XF_STRIP + (size_t)xf_level_words(Q)) * sizeof(float); }
constexpr size_t XF_MAX_LDS = xf_lds_bytes(XF_MAX_Q);
static_assert(XF_MAX_LDS <= 160 * 1024, "the tables of one strip must fit the CU's LDS");

struct XfArgs {
  const float* src; float* dst;
  const int32_t* kind; const float* knots; const float* levels; const float* center; const float* scale;
  long long ld_src, ld_dst, rows, rows_per;
  int D, Q;
};

// #{i : tab[slot(i)] < x} (UPPER: <= x) over a non-decreasing table of Q entries, XF_ILP searches side by side.  The trip count
// depends on Q alone: no divergence.  slot maps an index to its word.
template <bool UPPER, class Slot>
__device__ __forceinline__ void xf_count(const float* tab, int Q, Slot slot, const float (&x)[XF_ILP], int (&n)[XF_ILP]) {
  int base[XF_ILP];
#pragma unroll
  for (int u = 0; u < XF_ILP; ++u) base[u] = 0;
  int len = Q;
  while (len > 1) {
    const int half = len >> 1;
#pragma unroll
    for (int u = 0; u < XF_ILP; ++u) {
      const float v = tab[slot(base[u] + half - 1)];
      base[u] += (UPPER ? v <= x[u] : v < x[u]) ? half : 0;
    }
    len -= half;
  }
#pragma unroll
  for (int u = 0; u < XF_ILP; ++u) {
    const float v = tab[slot(base[u])];
    n[u] = base[u] + ((UPPER ? v <= x[u] : v < x[u]) ? 1 : 0);
  }
}

// The same count over this lane's column of the [Q][32] knot image, col = kn + c.  The search carries the LDS address of the row
// BELOW its lower end, so the probe of a step is that address plus the step: one add, then the compare, a select and an add for the
// move -- the issue rate of these vector instructions, not the LDS array, bounds the kernel.  The row below
// the first knot lies in the level table (xf_level_words >= 32) and is never read.
template <bool UPPER>
__device__ __forceinline__ void xf_count_knots(const float* col, int Q, const float (&x)[XF_ILP], int (&n)[XF_ILP]) {
  using lds_float = __attribute__((address_space(3))) const float;      // a 32-bit LDS address: the adds below are dword adds
  lds_float* const below = (lds_float*)col - XF_STRIP;
  lds_float* p[XF_ILP];
#pragma unroll
  for (int u = 0; u < XF_ILP; ++u) p[u] = below;
  int len = Q;
  while (len > 1) {
    const int half = len >> 1;
    const int step = half * XF_STRIP;
#pragma unroll
    for (int u = 0; u < XF_ILP; ++u) {
      const float v = p[u][step];                            // knot base + half - 1
      p[u] += (UPPER ? v <= x[u] : v < x[u]) ? step : 0;
    }
    len -= half;
  }
#pragma unroll
  for (int u = 0; u < XF_ILP; ++u) {
    const float v = p[u][XF_STRIP];
    n[u] = (int)(p[u] - below) / XF_STRIP + ((UPPER ? v <= x[u] : v < x[u]) ? 1 : 0);
  }
}

// FeatureTransform.forward_host (transform.py) restates the forward rule, this clamp included, in NumPy float32 for map_bounds, and
// tests hold the two bit-equal: change them together.
__device__ __forceinline__ float xf_lerp(float a, float b, float t) {
  const float y = a + t * (b - a);
  return fminf(fmaxf(y, a), b);          // a + fl(b - a) can pass b by an ulp: the result stays inside its bracket
}

template <bool INVERSE>
__global__ __launch_bounds__(XF_THREADS) void xf_kernel(XfArgs a) {
  extern __shared__ float xf_lds[];
  const int Q = a.Q, D = a.D;
  float* lv = xf_lds;                                        // levels, entry i at xf_level_slot(i)
  float* kn = xf_lds + xf_level_words(Q);                    // [Q][32]
  const int tid = threadIdx.x, c = tid & (XF_STRIP - 1), rsub = tid >> 5;
  const int col = (int)blockIdx.x * XF_STRIP + c;
  const bool in = col < D;
  const int kind = in ? a.kind[col] : XF_KIND_IDENTITY;
  const bool quant = kind == XF_KIND_QUANTILE;

  if (__syncthreads_or(quant)) {
    // 32 lanes = the 32 columns of one q (conflict-free stores); the 32 lane groups of the workgroup take 32 consecutive q, one
    // 128-byte line per column per pass.  With Q a multiple of 4 a lane fetches four consecutive q of its column at once.
    const float* kc = a.knots + (size_t)(in ? col : 0) * (size_t)Q;
    if ((Q & 3) == 0 && (reinterpret_cast<uintptr_t>(a.knots) & 15) == 0) {
      for (int q = rsub * 4; q < Q; q += XF_ROWS * 4) {
        if (quant) {
          const float4 v = *reinterpret_cast<const float4*>(kc + q);
          kn[(q + 0) * XF_STRIP + c] = v.x;
          kn[(q + 1) * XF_STRIP + c] = v.y;
          kn[(q + 2) * XF_STRIP + c] = v.z;
          kn[(q + 3) * XF_STRIP + c] = v.w;
        }
      }
    } else {
      for (int q = rsub; q < Q; q += XF_ROWS)
        if (quant) kn[q * XF_STRIP + c] = kc[q];
    }
    for (int i = tid; i < Q; i += XF_THREADS) lv[xf_level_slot(i)] = a.levels[i];
    __syncthreads();
  }

  const float ctr = kind == XF_KIND_STANDARD ? a.center[col] : 0.0f;
  const float scl = kind == XF_KIND_STANDARD ? a.scale[col] : 1.0f;
  const long long r0 = (long long)blockIdx.y * a.rows_per;
  const long long r1 = min(a.rows, r0 + a.rows_per);
  const auto knot_slot = [c](int i) { return i * XF_STRIP + c; };
  const auto level_slot = [](int i) { return xf_level_slot(i); };
  // the clamps' values: the ends of the level table and of this lane's column
  const float z_first = quant ? lv[xf_level_slot(0)] : 0.0f, z_last = quant ? lv[xf_level_slot(Q - 1)] : 0.0f;
  const float k_first = quant ? kn[knot_slot(0)] : 0.0f, k_last = quant ? kn[knot_slot(Q - 1)] : 0.0f;

  // the next XF_ILP rows are loaded before this set is searched: their latency hides under the LDS reads.  A lane reads an element
  // before it writes it and no other lane touches it, so in place stays safe.
  float xn[XF_ILP];
  const auto load = [&](long long r) {
#pragma unroll
    for (int u = 0; u < XF_ILP; ++u) {
      const long long row = r + (long long)u * XF_ROWS;
      xn[u] = in && row < r1 ? a.src[(size_t)row * (size_t)a.ld_src + col] : 0.0f;
    }
  };
  load(r0 + rsub);
  for (long long r = r0 + rsub; r < r1; r += XF_ROWS * XF_ILP) {
    float x[XF_ILP], y[XF_ILP];
    bool live[XF_ILP];
#pragma unroll
    for (int u = 0; u < XF_ILP; ++u) {
      live[u] = in && r + (long long)u * XF_ROWS < r1;
      x[u] = xn[u];
    }
    load(r + XF_ROWS * XF_ILP);
    if (quant) {
      // a row past the end of the chunk holds the placeholder 0: its lane searches for it in its own column's words -- in bounds --
      // and the result is never stored (a lane past column D is an identity lane and never comes here)
      if (!INVERSE) {
        int lb[XF_ILP], ub[XF_ILP];
        xf_count_knots<false>(kn + c, Q, x, lb);
        // x equals k[lb]: a knot or a plateau of knots lb .. ub - 1.  Zero-inflated columns make that the common case, so the wavefront
        // runs the second search for all of its rows side by side as soon as one lane needs it (NaN compares unequal)
        bool tie[XF_ILP], any_tie = false;
#pragma unroll
        for (int u = 0; u < XF_ILP; ++u) {
          tie[u] = lb[u] < Q && kn[knot_slot(min(lb[u], Q - 1))] == x[u];
          any_tie |= tie[u];
        }
        if (__any(any_tie)) {
          xf_count_knots<true>(kn + c, Q, x, ub);
        } else {
#pragma unroll
          for (int u = 0; u < XF_ILP; ++u) ub[u] = lb[u];
        }
        // every lane reads what either case needs (indices clamped into the tables), all rows' reads side by side, and the case
        // is a select: no divergence, and what the case not taken computes -- 0 / 0 on a plateau -- is dropped
        float k0[XF_ILP], k1[XF_ILP], z0[XF_ILP], z1[XF_ILP], za[XF_ILP], zb[XF_ILP];
#pragma unroll
        for (int u = 0; u < XF_ILP; ++u) {
          const int j = min(max(lb[u] - 1, 0), Q - 2), s = lb[u] + ub[u];
          k0[u] = kn[knot_slot(j)];
          k1[u] = kn[knot_slot(j + 1)];
          z0[u] = lv[xf_level_slot(j)];
          z1[u] = lv[xf_level_slot(j + 1)];
          za[u] = lv[xf_level_slot(min(max((s - 1) >> 1, 0), Q - 1))];      // a tie has ub >= lb + 1: both mid-rank indices lie in
          zb[u] = lv[xf_level_slot(min(s >> 1, Q - 1))];                    // [lb, ub - 1] without the clamps
        }
#pragma unroll
        for (int u = 0; u < XF_ILP; ++u) {
          const float xv = x[u];
          const float t = (xv - k0[u]) / (k1[u] - k0[u]);
          float out = tie[u] ? 0.5f * (za[u] + zb[u]) : xf_lerp(z0[u], z1[u], t);
          out = !tie[u] && lb[u] == 0 ? z_first : out;       // ub == 0
          out = lb[u] == Q ? z_last : out;
          y[u] = xv != xv ? xv : out;
        }
      } else {
        int ub[XF_ILP];
        xf_count<true>(lv, Q, level_slot, x, ub);
        float k0[XF_ILP], k1[XF_ILP], z0[XF_ILP], z1[XF_ILP];
#pragma unroll
        for (int u = 0; u < XF_ILP; ++u) {
          const int j = min(max(ub[u] - 1, 0), Q - 2);       // zl[j] <= z < zl[j + 1] wherever neither clamp below applies
          z0[u] = lv[xf_level_slot(j)];
          z1[u] = lv[xf_level_slot(j + 1)];
          k0[u] = kn[knot_slot(j)];
          k1[u] = kn[knot_slot(j + 1)];
        }
#pragma unroll
        for (int u = 0; u < XF_ILP; ++u) {
          const float zv = x[u];
          const float t = (zv - z0[u]) / (z1[u] - z0[u]);
          float out = xf_lerp(k0[u], k1[u], t);
          out = zv <= z_first ? k_first : out;
          out = ub[u] >= Q ? k_last : out;                   // z >= zl[Q - 1]
          y[u] = zv != zv ? zv : out;
        }
      }
    } else if (kind == XF_KIND_STANDARD) {
#pragma unroll
      for (int u = 0; u < XF_ILP; ++u) y[u] = INVERSE ? x[u] * scl + ctr : (x[u] - ctr) / scl;
    } else {
#pragma unroll
      for (int u = 0; u < XF_ILP; ++u) y[u] = x[u];
    }
#pragma unroll
    for (int u = 0; u < XF_ILP; ++u) {
      const long long row = r + (long long)u * XF_ROWS;
      if (live[u]) a.dst[(size_t)row * (size_t)a.ld_dst + col] = y[u];
    }
  }
}

// more than 64 KiB of dynamic LDS needs the function attribute, and the attribute is per device
bool g_xf_attr[XF_MAX_DEVICES] = {};

}  // namespace
}  // namespace osd

using namespace osd;

extern "C" {

int osd_xf_apply(void* stream, int device, const float* src, int64_t ld_src, float* dst, int64_t ld_dst, int64_t rows, int D,
                 const int32_t* kind_dev, const float* knots_dev, int Q, const float* levels_dev, const float* center_dev,
                 const float* scale_dev, int inverse) {
  if (!src || !dst || !kind_dev || !knots_dev || !levels_dev || !center_dev || !scale_dev) {
    set_error("bad argument (src, dst, kind, knots, levels, center and scale not NULL)");
    return OSD_EINVAL;
  }
  if (Q < 2 || Q > XF_MAX_Q || D < 1 || rows < 0 || ld_src < D || ld_dst < D || device < 0 || device >= XF_MAX_DEVICES) {
    set_error("bad argument (2 <= Q <= %d, D >= 1, rows >= 0, ld_src >= D, ld_dst >= D)", XF_MAX_Q);
    return OSD_EINVAL;
  }
  if (rows == 0) return OSD_OK;
  OSD_HIP(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  // the kinds choose the code path of a column: an unknown one is refused before anything is launched
  std::vector<int32_t> kinds((size_t)D);
  OSD_HIP(read_back(s, kinds.data(), kind_dev, (size_t)D * sizeof(int32_t)));
  for (int f = 0; f < D; ++f)
    if (kinds[f] != XF_KIND_IDENTITY && kinds[f] != XF_KIND_STANDARD && kinds[f] != XF_KIND_QUANTILE) {
      set_error("bad argument (kind[%d] = %d: 0 identity, 1 standard, 2 quantile_normal)", f, (int)kinds[f]);
      return OSD_EINVAL;
    }
  if (!g_xf_attr[device]) {
    OSD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(xf_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)XF_MAX_LDS));
    OSD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(xf_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)XF_MAX_LDS));
    g_xf_attr[device] = true;
  }
  const int64_t strips = ((int64_t)D + XF_STRIP - 1) / XF_STRIP;
  const int64_t chunks_wanted = (XF_TARGET_WGS + strips - 1) / strips;
  int64_t rows_per = (rows + chunks_wanted - 1) / chunks_wanted;
  if (rows_per < XF_MIN_ROWS_PER) rows_per = XF_MIN_ROWS_PER;
  if ((rows + rows_per - 1) / rows_per > 65535) rows_per = (rows + 65534) / 65535;
  const int64_t chunks = (rows + rows_per - 1) / rows_per;
  XfArgs a{};
  a.src = src; a.dst = dst; a.kind = kind_dev; a.knots = knots_dev; a.levels = levels_dev; a.center = center_dev; a.scale = scale_dev;
  a.ld_src = ld_src; a.ld_dst = ld_dst; a.rows = rows; a.rows_per = rows_per; a.D = D; a.Q = Q;
  const dim3 grid((unsigned)strips, (unsigned)chunks);
  if (inverse) {
    OSD_HIP(launched(xf_kernel<true>, grid, dim3(XF_THREADS), xf_lds_bytes(Q), s, a));
  } else {
    OSD_HIP(launched(xf_kernel<false>, grid, dim3(XF_THREADS), xf_lds_bytes(Q), s, a));
  }
  return OSD_OK;
}

}  // extern "C"
