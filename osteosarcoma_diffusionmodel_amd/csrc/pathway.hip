// pathway.hip -- per-patient pathway scores and their agreement with a generated pathway block:
//   osd_val_pathway_scores     for every row of X (rows patients x D genes, fp32, read in place, once) the score of S gene sets, each
//                              a list of m distinct columns: norm * sum_j (x_j - c_j) s_j (`mean`: norm 1/m; `zscore`: 1/sqrt(m)) or
//                              the single-sample enrichment score of Barbie et al. 2009 (`ssgsea`) in its closed form over the
//                              row's mid-ranks.
//   osd_val_pathway_agreement  the six column sums behind Pearson r, RMSE, bias and sd ratio of a block against standardised scores.
//
// One workgroup owns a row; nothing leaves it but the S scores.
//   pw_linear   the row into LDS as it is (one coalesced read); then a group of 16 lanes per set, four sets in flight per wavefront:
//               lane l adds the members l, l + 16, ... in double -- difference, product and sum --, a butterfly adds the group's
//               lanes, one division by m or sqrt(m).  Centre and scale come from a per-member table that pw_member_stats gathers
//               once per call, read beside the member list.
//   pw_ssgsea   the row into LDS as order-preserving unsigned keys (-0.0 first made +0.0), padded to a power of two with a key above
//               +inf; the bitonic sort of lds_sort.h (shared with gsea.hip); then a wavefront per set: a member's key is formed again
//               from X (the row was just read: a cache hit), its lower bound in the sorted keys is #{x < x_g}, its upper bound --
//               searched only where the next sorted key equals it -- #{x <= x_g}, and 2 r_g = their sum + 1 is an exact integer
//               that indexes the host-made table T[k] = (k / 2)^alpha.  Per member one product and two additions in double; the
//               sum of the ranks is an integer.  The ranks are never stored: the keys are all the LDS a row takes, N * 4 bytes (128
//               KiB at D = 32768), whatever the number of genes the sets use, and the sets need no de-duplication.  A row that holds
//               a NaN writes NaN to its S scores and leaves before the sort.
//   pa_partial  per (tile of 4096 rows, pathway) the six sums and the number of rows used: a lane adds its rows in ascending order,
//               a butterfly adds the lanes, lane 0 adds the four wavefronts; the host adds the tiles in ascending order.
// No atomics, and nothing depends on which rows share a launch: the same bits on every call and at every row_chunk, a permutation
// of the rows permutes the outputs, and a set listed twice gets the same bits twice.
// Host plumbing shared with gsea.hip: check_sets and Packed (val_common.h), PhaseClock and the two searches (val_columns.h).
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <vector>
#include <hip/hip_runtime.h>
#include "handle.h"
#include "lds_sort.h"
#include "val_columns.h"

namespace osd {
namespace {

constexpr int PW_MAX_D = 32768;            // keys of a row: 128 KiB of LDS
constexpr int PW_MAX_M = 1024;             // members of a set
constexpr int PW_MAX_THREADS = 1024;
constexpr int PW_GROUP = 16;               // lanes of pw_linear that share a set: four sets in flight per wavefront
constexpr int PW_AUTO_CHUNK = 1 << 20;     // rows of a launch when row_chunk = 0
constexpr uint32_t PW_PAD_KEY = 0xFFFFFFFFu;
constexpr int PA_THREADS = 256;
constexpr int PA_TILE = 4096;              // rows of a partial sum
constexpr int PA_MAX_S = 65535;            // a grid dimension
constexpr int PA_SUMS = 6;

enum { PW_MEAN = 0, PW_ZSCORE = 1, PW_SSGSEA = 2 };

// ascending as unsigned exactly where the floats ascend; -0.0 and +0.0 share a key, +inf lies below the padding
__device__ __forceinline__ uint32_t pw_key(float x) {
  uint32_t b = __float_as_uint(x);
  if (b == 0x80000000u) b = 0u;
  return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}

// grid (ceil(M / 256)).  cs [M]: every member's (centre, scale), 0 and 1 where the array is absent: gathered once per call, so that
// pw_linear reads them beside the member list, coalesced, and not per row through two more gathers
__global__ __launch_bounds__(256) void pw_member_stats(const int* __restrict__ members, int M, const float* __restrict__ center,
                                                       const float* __restrict__ scale, float2* __restrict__ cs) {
  const int e = (int)(blockIdx.x * 256 + threadIdx.x);
  if (e >= M) return;
  const int g = members[e];                                    // checked by the host: in [0, D)
  cs[e] = make_float2(center ? center[g] : 0.f, scale ? scale[g] : 1.f);
}

// grid (rows of the chunk), dynamic LDS D * 4 bytes.  cs: pw_member_stats' table, or NULL for centre 0 and scale 1
__global__ __launch_bounds__(PW_MAX_THREADS) void pw_linear(const float* __restrict__ X, int64_t row0, int ld, int D, int method,
                                                            const float2* __restrict__ cs, const int* __restrict__ offsets,
                                                            const int* __restrict__ members, int S, double* __restrict__ out) {
  extern __shared__ float pw_row[];
  const int tid = threadIdx.x, nt = blockDim.x;
  const int64_t row = row0 + blockIdx.x;
  const float* x = X + row * ld;
#pragma unroll 4
  for (int i = tid; i < D; i += nt) pw_row[i] = x[i];
  __syncthreads();
  const int lane = tid & (PW_GROUP - 1), ng = nt / PW_GROUP;
  for (int q = tid / PW_GROUP; q < S; q += ng) {
    const int lo = offsets[q], m = offsets[q + 1] - lo;        // 1 <= m <= PW_MAX_M
    double acc = 0.0;
    if (cs) {
      for (int e = lane; e < m; e += PW_GROUP) {
        const float2 v = cs[lo + e];
        acc += ((double)pw_row[members[lo + e]] - (double)v.x) * (double)v.y;   // members: checked by the host, in [0, D)
      }
    } else {
      for (int e = lane; e < m; e += PW_GROUP) acc += (double)pw_row[members[lo + e]];
    }
#pragma unroll
    for (int o = PW_GROUP / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o);     // inside the group's own lanes
    if (lane == 0) out[row * S + q] = acc / (method == PW_MEAN ? (double)m : sqrt((double)m));
  }
}

// grid (rows of the chunk), dynamic LDS N * 4 bytes; N: the power of two >= D
__global__ __launch_bounds__(PW_MAX_THREADS) void pw_ssgsea(const float* __restrict__ X, int64_t row0, int ld, int D, int N,
                                                            const int* __restrict__ offsets, const int* __restrict__ members, int S,
                                                            const double* __restrict__ table, double* __restrict__ out) {
  extern __shared__ uint32_t pw_keys[];
  __shared__ int has_nan;
  uint32_t* s = pw_keys;
  const int tid = threadIdx.x, nt = blockDim.x;
  const int64_t row = row0 + blockIdx.x;
  const float* x = X + row * ld;
  double* o = out + row * S;
  if (tid == 0) has_nan = 0;
  __syncthreads();
  bool nan = false;
  for (int i = tid; i < N; i += nt) {
    uint32_t key = PW_PAD_KEY;
    if (i < D) {
      const float v = x[i];
      nan |= v != v;
      key = pw_key(v);
    }
    s[i] = key;
  }
  if (nan) has_nan = 1;                                        // every writer writes the same value
  __syncthreads();
  if (has_nan) {                                               // the whole workgroup leaves
    for (int q = tid; q < S; q += nt) o[q] = NAN;
    return;
  }
  lds_bitonic_sort(s, N, tid, nt);
  const int lane = tid & 63, nw = nt >> 6;
  const double pairs = 0.5 * (double)D * (double)(D + 1);      // 1 + ... + D: an integer below 2^30
  for (int q = tid >> 6; q < S; q += nw) {
    const int lo = offsets[q], m = offsets[q + 1] - lo;        // 1 <= m <= PW_MAX_M, m < D
    double a = 0.0, b = 0.0;
    int r2sum = 0;                                             // at most 1024 * 65536
    for (int e = lane; e < m; e += 64) {
      const uint32_t key = pw_key(x[members[lo + e]]);         // checked by the host: in [0, D); not the padding: no NaN here
      const int l = lower_bound(s, 0, N, key);
      int u = l + 1;                                           // s[l] == key: the key is in the row
      if (u < N && s[u] == key) u = upper_bound(s, u, N, key); // a tie: where the run ends
      int r2 = l + u + 1;                                      // twice the mid-rank: 2 ... 2 D
      r2 = r2 < 2 * D ? r2 : 2 * D;                            // stays inside the table even if X changes under the call
      const double t = table[r2];
      a += (0.5 * (double)r2) * t;
      b += t;
      r2sum += r2;
    }
    wave_sum(a, b, r2sum);
    if (lane == 0) o[q] = a / b - (pairs - 0.5 * (double)r2sum) / (double)(D - m);
  }
}

// grid (tiles, S).  part [tiles][S][6], used [tiles][S]
__global__ __launch_bounds__(PA_THREADS) void pa_partial(const double* __restrict__ scores, int64_t rows, int S,
                                                         const float* __restrict__ block, int ld_b, const double* __restrict__ mu,
                                                         const double* __restrict__ isd, double* __restrict__ part,
                                                         long long* __restrict__ used) {
  __shared__ double wsum[PA_THREADS / 64][PA_SUMS];
  __shared__ long long wn[PA_THREADS / 64];
  const int tid = threadIdx.x, q = blockIdx.y;
  const int64_t r0 = (int64_t)blockIdx.x * PA_TILE, r1 = r0 + PA_TILE < rows ? r0 + PA_TILE : rows;
  const double m = mu[q], sc = isd[q];
  double sz = 0.0, sg = 0.0, szz = 0.0, sgg = 0.0, szg = 0.0, sdd = 0.0;
  long long n = 0;
  for (int64_t r = r0 + tid; r < r1; r += PA_THREADS) {
    const double z = (scores[r * S + q] - m) * sc, g = (double)block[r * ld_b + q];
    if (isfinite(z) && isfinite(g)) {
      const double d = g - z;
      sz += z; sg += g; szz += z * z; sgg += g * g; szg += z * g; sdd += d * d;
      ++n;
    }
  }
  wave_sum(sz, sg, szz, sgg, szg, sdd, n);
  const int wv = tid >> 6;
  if ((tid & 63) == 0) {
    wsum[wv][0] = sz; wsum[wv][1] = sg; wsum[wv][2] = szz; wsum[wv][3] = sgg; wsum[wv][4] = szg; wsum[wv][5] = sdd;
    wn[wv] = n;
  }
  __syncthreads();
  if (tid < PA_SUMS) {
    double a = wsum[0][tid];
    for (int v = 1; v < PA_THREADS / 64; ++v) a += wsum[v][tid];
    part[((size_t)blockIdx.x * S + q) * PA_SUMS + tid] = a;
  }
  if (tid == PA_SUMS) {
    long long a = wn[0];
    for (int v = 1; v < PA_THREADS / 64; ++v) a += wn[v];
    used[(size_t)blockIdx.x * S + q] = a;
  }
}

int pathway_scores(void* stream, int device, const float* X, int64_t rows, int ld, int D, int method, const float* center,
                   const float* scale, const int32_t* offsets, const int32_t* members, int S, const double* table, int row_chunk,
                   double* out, float* phase_ms) {
  if (!X || !offsets || !members || !out) { set_error("bad argument (NULL pointer)"); return OSD_EINVAL; }
  if (method != PW_MEAN && method != PW_ZSCORE && method != PW_SSGSEA) { set_error("bad argument (method: 0 mean, 1 zscore, 2 ssgsea)"); return OSD_EINVAL; }
  if (method == PW_SSGSEA && !table) { set_error("bad argument (ssgsea needs the rank table)"); return OSD_EINVAL; }
  if (D < 2 || D > PW_MAX_D) { set_error("bad argument (2 <= D <= %d)", PW_MAX_D); return OSD_EINVAL; }
  if (rows < 1 || ld < D || S < 1 || row_chunk < 0) { set_error("bad argument (rows >= 1, ld >= D, S >= 1, row_chunk >= 0)"); return OSD_EINVAL; }
  std::vector<int32_t> seen;
  OSD_TRY(check_sets(offsets, members, S, D, PW_MAX_M, "column", 'm', seen));
  const int M = offsets[S];
  const bool ranked = method == PW_SSGSEA;

  OSD_HIP(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  PhaseClock<2, float> clock(phase_ms);                        // upload, scoring
  OSD_HIP(clock.init());
  // one allocation, uploaded in one copy: the table first (doubles), then the offsets and the members
  Packed ws;
  const size_t at_tab = ws.put(table, ranked ? (size_t)(2 * D + 1) * sizeof(double) : 0);
  const size_t at_off = ws.put(offsets, (size_t)(S + 1) * sizeof(int32_t)), at_mem = ws.put(members, (size_t)M * sizeof(int32_t));
  const bool stats = !ranked && (center || scale);
  const size_t at_cs = ws.take(stats ? (size_t)M * sizeof(float2) : 0);  // filled on the device
  OSD_TRY(ws.alloc());
  OSD_HIP(clock.mark(0, st));
  OSD_HIP(ws.upload(st));
  OSD_HIP(clock.mark(1, st));
  OSD_HIP(hipStreamSynchronize(st));                           // the upload has left the staging vector
  const double* dtab = ws.at<const double>(at_tab);
  const int* doff = ws.at<const int>(at_off);
  const int* dmem = ws.at<const int>(at_mem);
  float2* dcs = stats ? ws.at<float2>(at_cs) : nullptr;
  if (stats) OSD_HIP(launched(pw_member_stats, dim3((unsigned)((M + 255) / 256)), 256, 0, st, dmem, M, center, scale, dcs));

  int N = 2;
  while (N < D) N <<= 1;
  // the workgroup: a lane per four keys of the sort (per key of the copy), 64 at least; rows up to 8192 keys stay at 512 lanes so
  // that four workgroups share a CU
  const int want = ranked ? N >> 2 : D;
  const int cap = (ranked ? N : D) <= 8192 ? (ranked ? 512 : 256) : PW_MAX_THREADS;
  int threads = 64;
  while (threads < want && threads < cap) threads <<= 1;
  const size_t lds = (size_t)(ranked ? N : D) * 4;
  if (ranked)
    OSD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(pw_ssgsea), hipFuncAttributeMaxDynamicSharedMemorySize, PW_MAX_D * 4));
  else
    OSD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(pw_linear), hipFuncAttributeMaxDynamicSharedMemorySize, PW_MAX_D * 4));
  const int64_t chunk = row_chunk ? row_chunk : PW_AUTO_CHUNK;
  for (int64_t r0 = 0; r0 < rows; r0 += chunk) {
    const unsigned c = (unsigned)(rows - r0 < chunk ? rows - r0 : chunk);
    if (ranked)
      OSD_HIP(launched(pw_ssgsea, dim3(c), threads, lds, st, X, r0, ld, D, N, doff, dmem, S, dtab, out));
    else
      OSD_HIP(launched(pw_linear, dim3(c), threads, lds, st, X, r0, ld, D, method, (const float2*)dcs, doff, dmem, S, out));
  }
  OSD_HIP(clock.mark(2, st));
  OSD_HIP(hipStreamSynchronize(st));                           // the workspace is free to go
  OSD_HIP(clock.add());
  return OSD_OK;
}

}  // namespace
}  // namespace osd

using namespace osd;

extern "C" {

int osd_val_pathway_scores(void* stream, int device, const float* X, int64_t rows, int ld, int D, int method, const float* center,
                           const float* scale, const int32_t* set_offsets_host, const int32_t* set_members_host, int S,
                           const double* rank_table_host, int row_chunk, double* out) {
  return pathway_scores(stream, device, X, rows, ld, D, method, center, scale, set_offsets_host, set_members_host, S, rank_table_host,
                        row_chunk, out, nullptr);
}

int osd_val_pathway_scores_timed(void* stream, int device, const float* X, int64_t rows, int ld, int D, int method, const float* center,
                                 const float* scale, const int32_t* set_offsets_host, const int32_t* set_members_host, int S,
                                 const double* rank_table_host, int row_chunk, double* out, float* phase_ms2) {
  if (!phase_ms2) { set_error("bad argument (NULL pointer)"); return OSD_EINVAL; }
  return pathway_scores(stream, device, X, rows, ld, D, method, center, scale, set_offsets_host, set_members_host, S, rank_table_host,
                        row_chunk, out, phase_ms2);
}

int osd_val_pathway_agreement(void* stream, int device, const double* scores, int64_t rows, int S, const float* block, int ld_b,
                              const double* mu_host, const double* isd_host, double* sums_host, int64_t* used_host) {
  if (!scores || !block || !mu_host || !isd_host || !sums_host || !used_host) { set_error("bad argument (NULL pointer)"); return OSD_EINVAL; }
  if (rows < 1 || S < 1 || S > PA_MAX_S || ld_b < S) { set_error("bad argument (rows >= 1, 1 <= S <= %d, ld_b >= S)", PA_MAX_S); return OSD_EINVAL; }
  const int64_t tiles = (rows + PA_TILE - 1) / PA_TILE;
  if (tiles > INT32_MAX) { set_error("bad argument (too many rows)"); return OSD_EINVAL; }
  OSD_HIP(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  Packed ws;
  const size_t at_mu = ws.put(mu_host, (size_t)S * sizeof(double)), at_isd = ws.put(isd_host, (size_t)S * sizeof(double));
  const size_t at_part = ws.take((size_t)tiles * S * PA_SUMS * sizeof(double)), at_used = ws.take((size_t)tiles * S * sizeof(long long));
  OSD_TRY(ws.alloc());
  OSD_HIP(ws.upload(st));
  double* dpart = ws.at<double>(at_part);
  long long* dused = ws.at<long long>(at_used);
  OSD_HIP(launched(pa_partial, dim3((unsigned)tiles, (unsigned)S), PA_THREADS, 0, st, scores, rows, S, block, ld_b, ws.at<const double>(at_mu),
                   ws.at<const double>(at_isd), dpart, dused));
  std::vector<double> part((size_t)tiles * S * PA_SUMS);
  std::vector<long long> used((size_t)tiles * S);
  OSD_HIP(hipMemcpyAsync(part.data(), dpart, part.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  OSD_HIP(read_back(st, used.data(), dused, used.size() * sizeof(long long)));
  for (int q = 0; q < S; ++q) {                                // the tiles in ascending order
    int64_t n = 0;
    for (int i = 0; i < PA_SUMS; ++i) sums_host[(size_t)q * PA_SUMS + i] = 0.0;
    for (int64_t t = 0; t < tiles; ++t) {
      for (int i = 0; i < PA_SUMS; ++i) sums_host[(size_t)q * PA_SUMS + i] += part[((size_t)t * S + q) * PA_SUMS + i];
      n += used[(size_t)t * S + q];
    }
    used_host[q] = n;
  }
  return OSD_OK;
}

}  // extern "C"
