// cox.hip -- the survival half of the validator:
//   osd_val_cox_plan_create / _destroy   the descending-time order of a cohort, its tie groups and event flags, made once per fit
//   osd_val_cox_eval                     Breslow partial likelihood of eta = w . u, u = (x - center) * scale: loss, gradient, scores
//   osd_val_concordance                  Harrell's pair counts of a risk score, exact
//
// The partial likelihood couples every row to its risk set, so one read of X cannot give the gradient: a call is TWO reads of X with
// 1-D work between them.
//   a. cox_eta_kernel: eta_i in fp32 with glm_kernel's arithmetic (glm.hip) -- d = x - center, w' = w * scale, the per-lane order
//      (row, column quad, element), the wave butterfly, the waves added in wave order -- and both of its load paths, so a score is the
//      bits osd_val_glm_eval gives for the same weights and a zero bias.
//   b. in double, rows in descending-time order p: m = max eta; e_p = exp(eta_p - m); P = inclusive prefix sums of e; S_p = P at the
//      END of p's tie group (Breslow); the loss terms delta_p (eta_p - m - log S_p) and q_p = delta_p / S_p; C = inclusive suffix sums
//      of q; c_p = C at the START of p's tie group; r_p = -delta_p + e_p c_p, rounded to fp32 and scattered back to the row's place.
//      A scan is three launches -- per-block sums, one workgroup that scans the sums, apply -- so NO WORKGROUP EVER WAITS FOR
//      ANOTHER inside a kernel: nothing looks back, nothing can spin.
//   c. cox_grad_kernel: g[col] += r_j d_j,col in fp32 over runs of at most OSD_GLM_RUN_ROWS rows, each run folded into the item's own
//      double slab; cox_reduce adds the slabs in a fixed order and applies the factor scale once, in double.
// No floating-point atomics anywhere: every sum has one fixed order, the same inputs give the same bits, and the partition into items
// depends on (rows, D) and the load path alone.
//
// Column ownership of (a) and (c) is glm_kernel's: ALIGNED (base 16-byte aligned, ld % 4 == 0, ld >= roundup(D, 4)) a lane owns the
// column quads tid + T j and loads 16 bytes; otherwise it owns the columns tid + T m and loads dwords, each checked against D --
// in place, never through a padded copy.  Neither pass keeps a row across a barrier, so four rows per group fit every width class.
#include <limits.h>
#include <math.h>
#include <cmath>
#include <stdint.h>
#include <algorithm>
#include <mutex>
#include <numeric>
#include <vector>
#include "cox_plan.h"
#include "handle.h"
#include "val_common.h"

namespace osd {
namespace {

constexpr int COX_MAX_ITEMS = 768;       // workgroups of a pass, as osd_val_glm_eval's
constexpr int COX_MIN_ITEM_ROWS = 16;    // an item writes D doubles: not for fewer rows than this
constexpr int COX_MAX_WAVES = 8;
constexpr int COX_R = 4;                 // rows of a group
constexpr int COX_RED_PARTS = 16;
constexpr int SCAN_T = 256, SCAN_PER = 4, SCAN_BLOCK = SCAN_T * SCAN_PER;      // a scan block: 256 lanes x 4 consecutive elements
constexpr int COX_MAX_PARTS = 1024;      // partial maxima of eta
static_assert(OSD_GLM_RUN_ROWS % COX_R == 0, "a run is a whole number of groups");

struct CoxPassArgs {
  const float* X; const float* center; const float* scale; const float* w;
  float* eta;              // (a): [rows], out
  const float* resid;      // (c): [rows], in
  double* slab;            // (c): [items][Dl]
  long long ld, rows, rows_per;    // rows_per: rows of an item, a multiple of the group
  int D, Dl;
};

template <int NV, bool ALIGNED>
__device__ __forceinline__ int cox_col(int tid, int T, int j, int e) {
  return ALIGNED ? 4 * (tid + T * j) + e : tid + T * (4 * j + e);
}

// rows gr .. gr + R - 1 of the item [.., r1): a row beyond the item re-reads its last row (the caller gives it weight 0 or drops it)
template <int NV, bool ALIGNED>
__device__ __forceinline__ void cox_load(const CoxPassArgs& a, float (&xb)[COX_R][NV][4], long long gr, long long r1, int tid, int T) {
#pragma unroll
  for (int r = 0; r < COX_R; ++r) {
    const long long row = min(gr + r, r1 - 1);
    const float* p = a.X + (size_t)row * (size_t)a.ld;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      if (ALIGNED) {
        const int q = 4 * (tid + T * j);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (q < a.D) v = *reinterpret_cast<const float4*>(p + q);
        xb[r][j][0] = v.x; xb[r][j][1] = v.y; xb[r][j][2] = v.z; xb[r][j][3] = v.w;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int col = cox_col<NV, ALIGNED>(tid, T, j, e);
          xb[r][j][e] = col < a.D ? p[col] : 0.f;
        }
      }
    }
  }
}

// (a) eta[row] = sum_col w'[col] (x[row][col] - center[col]): glm_kernel's steps 1 to 3 for one head without a bias
template <int NV, int TMAX, bool ALIGNED>
__global__ __launch_bounds__(TMAX) void cox_eta_kernel(CoxPassArgs a) {
  constexpr int R = COX_R;
  __shared__ float part[2][COX_MAX_WAVES][R];
  const int tid = threadIdx.x, T = blockDim.x;
  const int lane = tid & 63, wave = tid >> 6, nw = T >> 6;
  const long long r0 = (long long)blockIdx.x * a.rows_per;
  const long long r1 = min(a.rows, r0 + a.rows_per);         // r0 < r1: the host launches no empty item
  float c[NV][4], w[NV][4];
#pragma unroll
  for (int j = 0; j < NV; ++j)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int col = cox_col<NV, ALIGNED>(tid, T, j, e);
      const bool in = col < a.D;
      c[j][e] = in ? a.center[col] : 0.f;
      w[j][e] = in ? a.w[col] * a.scale[col] : 0.f;
    }
  int par = 0;
  for (long long gr = r0; gr < r1; gr += R, par ^= 1) {      // the same trip count in the whole workgroup
    float xb[R][NV][4];
    cox_load<NV, ALIGNED>(a, xb, gr, r1, tid, T);
    float p[R];
#pragma unroll
    for (int r = 0; r < R; ++r) p[r] = 0.f;
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int j = 0; j < NV; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float d = xb[r][j][e] - c[j][e];
          p[r] += w[j][e] * d;
        }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      float v = p[r];
      wave_sum(v);
      if (lane == 0) part[par][wave][r] = v;
    }
    __syncthreads();                                         // part[par] is next written two groups on, behind the next barrier
    if (tid < R) {
      float z = part[par][0][tid];
      for (int q = 1; q < nw; ++q) z += part[par][q][tid];
      const long long row = gr + tid;
      if (row < r1) a.eta[row] = z;
    }
  }
}

// (c) the item's column sums of resid[row] (x[row][col] - center[col]): glm_kernel's step 4 and its fold
template <int NV, int TMAX, bool ALIGNED>
__global__ __launch_bounds__(TMAX) void cox_grad_kernel(CoxPassArgs a) {
  constexpr int R = COX_R;
  const int tid = threadIdx.x, T = blockDim.x;
  const long long item = blockIdx.x;
  const long long r0 = item * a.rows_per;
  const long long r1 = min(a.rows, r0 + a.rows_per);
  const long long n_rows = r1 - r0;
  float c[NV][4], g[NV][4];
#pragma unroll
  for (int j = 0; j < NV; ++j)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int col = cox_col<NV, ALIGNED>(tid, T, j, e);
      c[j][e] = col < a.D ? a.center[col] : 0.f;
      g[j][e] = 0.f;
    }
  int folds = 0;
  long long done = 0;
  for (long long gr = r0; gr < r1; gr += R) {
    float xb[R][NV][4];
    cox_load<NV, ALIGNED>(a, xb, gr, r1, tid, T);
    float f[R];
#pragma unroll
    for (int r = 0; r < R; ++r) f[r] = gr + r < r1 ? a.resid[gr + r] : 0.f;      // 0 for a row beyond the item
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int j = 0; j < NV; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float d = xb[r][j][e] - c[j][e];
          g[j][e] += f[r] * d;
        }
    done += R;
    if (done % OSD_GLM_RUN_ROWS == 0 || done >= n_rows) {    // end of an fp32 run: into the item's own double slab
#pragma unroll
      for (int j = 0; j < NV; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int col = cox_col<NV, ALIGNED>(tid, T, j, e);
          if (col < a.D) {
            double* s = a.slab + (size_t)item * (size_t)a.Dl + col;
            *s = (folds ? *s : 0.0) + (double)g[j][e];
          }
          g[j][e] = 0.f;
        }
      ++folds;
    }
  }
}

// grad[col] = scale[col] * sum over the items: 64 columns x 16 parts per workgroup, part p adds items p, p + 16, ... in that order,
// then the parts are added in part order
__global__ __launch_bounds__(64 * COX_RED_PARTS) void cox_reduce(const double* __restrict__ slab, int items, int D, int Dl,
                                                                 const float* __restrict__ scale, double* __restrict__ grad) {
  __shared__ double part[COX_RED_PARTS][64];
  const int cx = threadIdx.x & 63, p = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + cx;
  double s = 0.0;
  if (col < D)
    for (int it = p; it < items; it += COX_RED_PARTS) s += slab[(size_t)it * (size_t)Dl + col];
  part[p][cx] = s;
  __syncthreads();
  if (p == 0 && col < D) {
    double t = part[0][cx];
    for (int q = 1; q < COX_RED_PARTS; ++q) t += part[q][cx];
    const float sc = scale[col];
    grad[col] = sc == 0.f ? 0.0 : t * (double)sc;            // a dropped column: exactly zero
  }
}

// ---- the 1-D work between the two passes -----------------------------------------------------------------------------------------
// Inclusive scan of the workgroup's SCAN_BLOCK values, lane tid owning elements 4 tid .. 4 tid + 3: in the lane, then up the wave,
// then the waves in wave order.  v becomes the inclusive prefix, ex what precedes the lane's first element; returns the workgroup's
// total.  One barrier; the caller puts another between two uses of the same wsum.
__device__ __forceinline__ double block_scan(double (&v)[SCAN_PER], double (&wsum)[SCAN_T / 64], double& ex) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int e = 1; e < SCAN_PER; ++e) v[e] += v[e - 1];
  double t = v[SCAN_PER - 1];
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double u = __shfl_up(t, o);
    if (lane >= o) t += u;
  }
  double prev = __shfl_up(t, 1);
  if (lane == 0) prev = 0.0;
  if (lane == 63) wsum[wave] = t;
  __syncthreads();
  double off = 0.0, total = 0.0;
#pragma unroll
  for (int q = 0; q < SCAN_T / 64; ++q) {
    if (q < wave) off += wsum[q];
    total += wsum[q];
  }
  ex = off + prev;
#pragma unroll
  for (int e = 0; e < SCAN_PER; ++e) v[e] = ex + v[e];
  return total;
}

__global__ __launch_bounds__(256) void cox_max_part(const float* __restrict__ eta, long long n, float* __restrict__ pmax) {
  __shared__ float wmax[4];
  float v = -INFINITY;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) v = fmaxf(v, eta[i]);
  wave_max(v);
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) pmax[blockIdx.x] = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
}

__global__ __launch_bounds__(256) void cox_max_final(const float* __restrict__ pmax, int parts, double* __restrict__ m) {
  __shared__ float wmax[4];
  float v = -INFINITY;
  for (int i = threadIdx.x; i < parts; i += 256) v = fmaxf(v, pmax[i]);
  wave_max(v);
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) *m = (double)fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
}

struct CoxStageArgs {
  const float* eta;            // [n], rows in their own order
  const int* order;            // [n]: the row at position p
  const int* gend;             // [n]: last position of p's tie group
  const unsigned char* ev;     // [n]: event flag of position p
  const double* m;
  const double* P;             // stage 1: prefix sums of e
  double* out;                 // stage 0: e[p]; stage 1: q[p]
  double* bsum;                // [blocks]: the block's sum of out, in scan order
  double* lpart;               // stage 1: [blocks], the block's sum of delta (eta - m - log S)
  long long n;
};

// STAGE 0: e_p = exp(eta_p - m), scanned forwards.  STAGE 1: q_p = delta_p / S_p and the loss terms, scanned BACKWARDS (scan index i
// is position n - 1 - i).  Writes the values and the block's sum; the scan itself is cox_scan_sums + cox_scan_apply.
template <int STAGE>
__global__ __launch_bounds__(SCAN_T) void cox_stage(CoxStageArgs a) {
  __shared__ double wsum[SCAN_T / 64], wsum2[SCAN_T / 64];
  double v[SCAN_PER], lt[SCAN_PER];
  const double m = *a.m;
#pragma unroll
  for (int e = 0; e < SCAN_PER; ++e) {
    const long long i = (long long)blockIdx.x * SCAN_BLOCK + threadIdx.x * SCAN_PER + e;
    v[e] = 0.0; lt[e] = 0.0;
    if (i < a.n) {
      const long long p = STAGE == 0 ? i : a.n - 1 - i;
      if (STAGE == 0) {
        v[e] = exp((double)a.eta[a.order[p]] - m);
      } else if (a.ev[p]) {
        const double S = a.P[a.gend[p]];
        v[e] = 1.0 / S;
        lt[e] = (double)a.eta[a.order[p]] - m - log(S);
      }
      a.out[p] = v[e];
    }
  }
  double ex;
  const double total = block_scan(v, wsum, ex);
  if (threadIdx.x == 0) a.bsum[blockIdx.x] = total;
  if (STAGE == 1) {
    const double ltotal = block_scan(lt, wsum2, ex);
    if (threadIdx.x == 0) a.lpart[blockIdx.x] = ltotal;
  }
}

// bsum[b] becomes the sum of the blocks before b: one workgroup walks the list in chunks of SCAN_BLOCK with a carry
__global__ __launch_bounds__(SCAN_T) void cox_scan_sums(double* __restrict__ bsum, long long blocks) {
  __shared__ double wsum[SCAN_T / 64];
  double carry = 0.0;
  for (long long base = 0; base < blocks; base += SCAN_BLOCK) {
    double v[SCAN_PER], ex;
#pragma unroll
    for (int e = 0; e < SCAN_PER; ++e) {
      const long long i = base + threadIdx.x * SCAN_PER + e;
      v[e] = i < blocks ? bsum[i] : 0.0;
    }
    const double total = block_scan(v, wsum, ex);
    // exclusive: the inclusive prefix of the element before (the lane's first: what precedes the lane)
#pragma unroll
    for (int e = 0; e < SCAN_PER; ++e) {
      const long long i = base + threadIdx.x * SCAN_PER + e;
      if (i < blocks) bsum[i] = carry + (e == 0 ? ex : v[e - 1]);
    }
    carry += total;
    __syncthreads();
  }
}

// out[p] = (sum of the blocks before) + the inclusive prefix of in inside the block; rev: scan index i is position n - 1 - i
__global__ __launch_bounds__(SCAN_T) void cox_scan_apply(const double* __restrict__ in, double* __restrict__ out,
                                                         const double* __restrict__ bsum, long long n, int rev) {
  __shared__ double wsum[SCAN_T / 64];
  double v[SCAN_PER];
#pragma unroll
  for (int e = 0; e < SCAN_PER; ++e) {
    const long long i = (long long)blockIdx.x * SCAN_BLOCK + threadIdx.x * SCAN_PER + e;
    v[e] = i < n ? in[rev ? n - 1 - i : i] : 0.0;
  }
  double ex;
  block_scan(v, wsum, ex);
  const double base = bsum[blockIdx.x];
#pragma unroll
  for (int e = 0; e < SCAN_PER; ++e) {
    const long long i = (long long)blockIdx.x * SCAN_BLOCK + threadIdx.x * SCAN_PER + e;
    if (i < n) out[rev ? n - 1 - i : i] = base + v[e];
  }
}

// r_p = -delta_p + e_p c_p, c_p the suffix sum at the START of p's tie group; to fp32, to the row's own place
__global__ __launch_bounds__(256) void cox_resid(const double* __restrict__ e, const double* __restrict__ Cs, const int* __restrict__ gstart,
                                                 const unsigned char* __restrict__ ev, const int* __restrict__ order, long long n,
                                                 float* __restrict__ resid) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const double r = (ev[p] ? -1.0 : 0.0) + e[p] * Cs[gstart[p]];
  resid[order[p]] = (float)r;
}

// ---- concordance ------------------------------------------------------------------------------------------------------------------
// A lane owns one i; the (t_j, risk_j) of a chunk go through LDS, read at one address by the whole wave.  A lane meets each j once,
// so its 32-bit counters hold below n = 2^32; the wave and the workgroup add in 64 bits into the workgroup's own slab.
__global__ __launch_bounds__(OSD_CONC_I_TILE) void conc_kernel(const float* __restrict__ t, const float* __restrict__ ev,
                                                               const float* __restrict__ risk, long long n,
                                                               unsigned long long* __restrict__ slab) {
  __shared__ float2 tj[OSD_CONC_J_CHUNK];
  __shared__ unsigned long long wpart[OSD_CONC_I_TILE / 64][3];
  const int tid = threadIdx.x;
  const long long i = (long long)blockIdx.x * OSD_CONC_I_TILE + tid;
  const bool live = i < n && ev[i] != 0.f;                   // only an event opens a comparable pair
  const float ti = live ? t[i] : 0.f, ri = live ? risk[i] : 0.f;
  unsigned comp = 0, conc = 0, disc = 0;
  for (long long j0 = 0; j0 < n; j0 += OSD_CONC_J_CHUNK) {
    __syncthreads();
    for (int k = tid; k < OSD_CONC_J_CHUNK; k += OSD_CONC_I_TILE) {
      const long long j = j0 + k;
      tj[k] = j < n ? make_float2(t[j], risk[j]) : make_float2(-INFINITY, 0.f);      // past the end: later than nothing
    }
    __syncthreads();
    if (live) {
#pragma unroll 8
      for (int k = 0; k < OSD_CONC_J_CHUNK; ++k) {
        const float2 v = tj[k];
        const unsigned c = ti < v.x ? 1u : 0u;
        comp += c;
        conc += c & (ri > v.y ? 1u : 0u);
        disc += c & (ri < v.y ? 1u : 0u);
      }
    }
  }
  unsigned long long a = comp, b = conc, d = disc;
  wave_sum(a, b, d);
  if ((tid & 63) == 0) { wpart[tid >> 6][0] = a; wpart[tid >> 6][1] = b; wpart[tid >> 6][2] = d; }
  __syncthreads();
  if (tid < 3) {
    unsigned long long s = 0;
    for (int q = 0; q < OSD_CONC_I_TILE / 64; ++q) s += wpart[q][tid];
    slab[(size_t)blockIdx.x * 3 + tid] = s;
  }
}

// One grow-only workspace per device (cox_plan.h): a fit calls osd_val_cox_eval hundreds of times.
CoxWorkspace* const g_cox_ws = new CoxWorkspace[COX_MAX_DEVICES];  // never destroyed: no hipFree from a static destructor at process exit

template <int NV, int TMAX>
hipError_t cox_launch2(bool grad, bool aligned, unsigned items, unsigned T, hipStream_t s, const CoxPassArgs& a) {
  if (grad)
    return launched(aligned ? cox_grad_kernel<NV, TMAX, true> : cox_grad_kernel<NV, TMAX, false>, dim3(items), dim3(T), 0, s, a);
  return launched(aligned ? cox_eta_kernel<NV, TMAX, true> : cox_eta_kernel<NV, TMAX, false>, dim3(items), dim3(T), 0, s, a);
}

hipError_t cox_launch(int NV, bool grad, bool aligned, unsigned items, unsigned T, hipStream_t s, const CoxPassArgs& a) {
  switch (NV) {
    case 1: return cox_launch2<1, 256>(grad, aligned, items, T, s, a);
    case 2: return cox_launch2<2, 512>(grad, aligned, items, T, s, a);
    case 3: return cox_launch2<3, 512>(grad, aligned, items, T, s, a);
    default: return cox_launch2<4, 512>(grad, aligned, items, T, s, a);
  }
}

}  // namespace

}  // namespace osd

using namespace osd;

extern "C" {

int osd_val_cox_plan_create(int device, void* stream, const double* time_host, const double* event_host, int64_t rows, void** plan) {
  if (plan) *plan = nullptr;
  if (!plan || !time_host || !event_host || rows < 1 || rows > INT_MAX || device < 0 || device >= COX_MAX_DEVICES) {
    set_error("bad argument (times and events for 1 <= rows < 2^31, a plan to fill)");
    return OSD_EINVAL;
  }
  for (int64_t i = 0; i < rows; ++i) {
    if (!std::isfinite(time_host[i])) { set_error("row %lld: the time is not finite", (long long)i); return OSD_EINVAL; }
    if (!(event_host[i] == 0.0 || event_host[i] == 1.0)) { set_error("row %lld: the event flag is neither 0 nor 1", (long long)i); return OSD_EINVAL; }
  }
  const int n = (int)rows;
  std::vector<int> order((size_t)n), gstart((size_t)n), gend((size_t)n);
  std::vector<int> gev((size_t)n, 0);
  std::vector<unsigned char> ev((size_t)n);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return time_host[x] > time_host[y]; });
  for (int p = 0; p < n;) {
    int e = p;
    while (e + 1 < n && time_host[order[(size_t)e + 1]] == time_host[order[(size_t)p]]) ++e;
    for (int k = p; k <= e; ++k) { gstart[(size_t)k] = p; gend[(size_t)k] = e; }
    p = e + 1;
  }
  for (int p = 0; p < n; ++p) ev[(size_t)p] = event_host[order[(size_t)p]] == 1.0 ? 1 : 0;
  for (int p = 0; p < n; ++p) gev[(size_t)gend[(size_t)p]] += ev[(size_t)p];

  OSD_HIP(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  CoxPlan* pl = new CoxPlan;
  pl->device = device; pl->stream = s; pl->rows = rows;
  auto fill = [&]() -> int {
    OSD_TRY(pl->order.reserve(n));
    OSD_TRY(pl->gstart.reserve(n));
    OSD_TRY(pl->gend.reserve(n));
    OSD_TRY(pl->ev.reserve(n));
    OSD_TRY(pl->gev.reserve(n));
    OSD_HIP(hipMemcpyAsync(pl->order.get(), order.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, s));
    OSD_HIP(hipMemcpyAsync(pl->gstart.get(), gstart.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, s));
    OSD_HIP(hipMemcpyAsync(pl->gend.get(), gend.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, s));
    OSD_HIP(hipMemcpyAsync(pl->ev.get(), ev.data(), (size_t)n, hipMemcpyHostToDevice, s));
    OSD_HIP(hipMemcpyAsync(pl->gev.get(), gev.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, s));
    OSD_HIP(hipStreamSynchronize(s));                        // the host vectors end with this call
    return OSD_OK;
  };
  const int rc = fill();
  if (rc != OSD_OK) { delete pl; return rc; }
  *plan = pl;
  return OSD_OK;
}

int osd_val_cox_plan_destroy(void* plan) {
  if (!plan) return OSD_OK;
  CoxPlan* pl = (CoxPlan*)plan;
  const hipError_t e = hipSetDevice(pl->device);
  (void)e;
  delete pl;
  return OSD_OK;
}

int osd_val_cox_eval(void* plan, const float* X, int64_t rows, int ld, int D, const float* center, const float* scale, const float* w,
                     double* loss_host, double* grad_dev, float* score_dev) {
  CoxPlan* pl = (CoxPlan*)plan;
  if (!pl || !X || !center || !scale || !w || rows < 1 || D < 1 || D > COX_MAX_D || ld < D) {
    set_error("bad argument (a plan, rows >= 1, 1 <= D <= 8192, ld >= D)");
    return OSD_EINVAL;
  }
  if (rows != pl->rows) {
    set_error("the plan was made for %lld rows, not %lld", (long long)pl->rows, (long long)rows);
    return OSD_EINVAL;
  }
  if (!loss_host && !grad_dev && !score_dev) { set_error("bad argument (at least one output)"); return OSD_EINVAL; }
  OSD_HIP(hipSetDevice(pl->device));
  hipStream_t s = pl->stream;

  // column classes and lanes: those of osd_val_glm_eval, so a score has its bits
  const int Dq = (D + 3) / 4 * 4, quads = Dq / 4;
  const int NV = quads <= 256 ? 1 : quads <= 1024 ? 2 : quads <= 1536 ? 3 : 4;
  const unsigned T = (unsigned)(((quads + NV - 1) / NV + 63) / 64 * 64);       // 64 .. 512 lanes, 4 NV T >= Dq columns
  const bool aligned = (reinterpret_cast<uintptr_t>(X) & 15) == 0 && ld % 4 == 0 && ld >= Dq;
  // the partition: a function of rows alone
  const int64_t groups = (rows + COX_R - 1) / COX_R;
  int64_t want = (rows + COX_MIN_ITEM_ROWS - 1) / COX_MIN_ITEM_ROWS;
  if (want > COX_MAX_ITEMS) want = COX_MAX_ITEMS;
  const int64_t gpi = (groups + want - 1) / want;
  const unsigned items = (unsigned)((groups + gpi - 1) / gpi);
  const long long n = rows;
  const long long blocks = (n + SCAN_BLOCK - 1) / SCAN_BLOCK;
  const int parts = (int)std::min<long long>(blocks, COX_MAX_PARTS);
  const bool chain = loss_host || grad_dev;                  // anything beyond the scores

  CoxPassArgs a{};
  a.X = X; a.center = center; a.scale = scale; a.w = w;
  a.ld = ld; a.rows = rows; a.rows_per = gpi * COX_R;
  a.D = D; a.Dl = Dq;

  CoxWorkspace& ws = g_cox_ws[pl->device];
  std::lock_guard<std::mutex> hold(ws.mu);
  size_t off = 0;
  auto carve = [&](size_t bytes) { const size_t at = off; off += up256(bytes); return at; };
  const size_t o_eta = carve(score_dev ? 0 : (size_t)n * sizeof(float));
  const size_t o_e = carve(chain ? (size_t)n * sizeof(double) : 0), o_P = carve(chain ? (size_t)n * sizeof(double) : 0);
  const size_t o_q = carve(chain ? (size_t)n * sizeof(double) : 0), o_r = carve(grad_dev ? (size_t)n * sizeof(float) : 0);
  const size_t o_bs = carve(chain ? (size_t)blocks * sizeof(double) : 0), o_lp = carve(chain ? (size_t)blocks * sizeof(double) : 0);
  const size_t o_pm = carve(COX_MAX_PARTS * sizeof(float)), o_m = carve(sizeof(double));
  const size_t o_slab = carve(grad_dev ? (size_t)items * a.Dl * sizeof(double) : 0);
  OSD_TRY(ws.buf.reserve((int64_t)off));
  char* base = ws.buf.get();
  float* eta = score_dev ? score_dev : (float*)(base + o_eta);
  double *e = (double*)(base + o_e), *P = (double*)(base + o_P), *q = (double*)(base + o_q);
  double *bsum = (double*)(base + o_bs), *lpart = (double*)(base + o_lp), *m = (double*)(base + o_m);
  float *resid = (float*)(base + o_r), *pmax = (float*)(base + o_pm);
  a.eta = eta; a.resid = resid; a.slab = (double*)(base + o_slab);

  OSD_HIP(cox_launch(NV, false, aligned, items, T, s, a));
  if (chain) {
    OSD_HIP(launched(cox_max_part, dim3((unsigned)parts), dim3(256), 0, s, (const float*)eta, n, pmax));
    OSD_HIP(launched(cox_max_final, dim3(1), dim3(256), 0, s, (const float*)pmax, parts, m));
    CoxStageArgs st{};
    st.eta = eta; st.order = pl->order.get(); st.gend = pl->gend.get(); st.ev = pl->ev.get(); st.m = m; st.P = P;
    st.out = e; st.bsum = bsum; st.lpart = lpart; st.n = n;
    OSD_HIP(launched(cox_stage<0>, dim3((unsigned)blocks), dim3(SCAN_T), 0, s, st));
    OSD_HIP(launched(cox_scan_sums, dim3(1), dim3(SCAN_T), 0, s, bsum, blocks));
    OSD_HIP(launched(cox_scan_apply, dim3((unsigned)blocks), dim3(SCAN_T), 0, s, (const double*)e, P, (const double*)bsum, n, 0));
    st.out = q;
    OSD_HIP(launched(cox_stage<1>, dim3((unsigned)blocks), dim3(SCAN_T), 0, s, st));
    if (grad_dev) {
      OSD_HIP(launched(cox_scan_sums, dim3(1), dim3(SCAN_T), 0, s, bsum, blocks));
      OSD_HIP(launched(cox_scan_apply, dim3((unsigned)blocks), dim3(SCAN_T), 0, s, (const double*)q, P, (const double*)bsum, n, 1));      // P now holds the suffix sums
      OSD_HIP(launched(cox_resid, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const double*)e, (const double*)P,
                       (const int*)pl->gstart.get(), (const unsigned char*)pl->ev.get(), (const int*)pl->order.get(), n, resid));
      OSD_HIP(cox_launch(NV, true, aligned, items, T, s, a));
      OSD_HIP(launched(cox_reduce, dim3((unsigned)((D + 63) / 64)), dim3(64 * COX_RED_PARTS), 0, s, (const double*)a.slab, (int)items, D,
                       a.Dl, scale, grad_dev));
    }
  }
  std::vector<double> part(loss_host ? (size_t)blocks : 0);
  if (loss_host) OSD_HIP(hipMemcpyAsync(part.data(), lpart, (size_t)blocks * sizeof(double), hipMemcpyDeviceToHost, s));
  OSD_HIP(hipStreamSynchronize(s));
  if (loss_host) {
    double t = 0.0;
    for (long long b = 0; b < blocks; ++b) t += part[(size_t)b];
    *loss_host = 0.0 - t;
  }
  return OSD_OK;
}

int osd_val_concordance(void* stream, int device, const float* time_dev, const float* event_dev, const float* risk_dev, int64_t n,
                        int64_t* counts_host) {
  if (!time_dev || !event_dev || !risk_dev || !counts_host || n < 1 || n > INT_MAX || device < 0 || device >= COX_MAX_DEVICES) {
    set_error("bad argument (times, events and risks for 1 <= n < 2^31, four counts to fill)");
    return OSD_EINVAL;
  }
  OSD_HIP(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  const long long tiles = ((long long)n + OSD_CONC_I_TILE - 1) / OSD_CONC_I_TILE;
  ValBuf slab;
  OSD_TRY(slab.alloc((size_t)tiles * 3 * sizeof(unsigned long long)));
  OSD_HIP(launched(conc_kernel, dim3((unsigned)tiles), dim3(OSD_CONC_I_TILE), 0, s, time_dev, event_dev, risk_dev, (long long)n,
                   slab.as<unsigned long long>()));
  std::vector<unsigned long long> h((size_t)tiles * 3);
  OSD_HIP(read_back(s, h.data(), slab.get(), h.size() * sizeof(unsigned long long)));
  unsigned long long tot[3] = {0, 0, 0};
  for (long long b = 0; b < tiles; ++b)
    for (int k = 0; k < 3; ++k) tot[k] += h[(size_t)b * 3 + k];
  counts_host[0] = (int64_t)tot[0];                          // comparable
  counts_host[1] = (int64_t)tot[1];                          // risk_i > risk_j: concordant
  counts_host[2] = (int64_t)tot[2];                          // risk_i < risk_j
  counts_host[3] = (int64_t)(tot[0] - tot[1] - tot[2]);      // equal risks
  return OSD_OK;
}

}  // extern "C"
