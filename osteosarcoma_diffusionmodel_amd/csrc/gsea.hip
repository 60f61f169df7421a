// gsea.hip -- the permutation null of preranked gene-set enrichment analysis:
//   osd_val_gsea   for S gene sets, given as ranked positions in a list of D genes with non-negative position weights, the
//                  positive and the negative extreme of the weighted running sum (Subramanian et al. 2005) under the identity and
//                  under P gene-label permutations that all sets share.
//
// Permutation p >= 1 moves position i to rho_p(i), the rank of (key_p(i), i) among the D such pairs, key_p(i) word 0 of the Philox
// block at (seed; i, p, 0, TAG_GSEA); rho_0 is the identity.  The host de-duplicates the positions that some set uses (U <= D of
// them) and states every member as an index into that list; the permutations then go through perm_chunk at a time.  Per chunk:
//   gs_ranks_sort   one workgroup per permutation: the D keys into LDS (padded to a power of two with the largest key) and, unsorted,
//                   into global memory; the bitonic sort of lds_sort.h (shared with pathway.hip); rho_p of a used
//                   position is the lower bound of its key, and where the next sorted key equals it -- a 32-bit collision, or a
//                   key equal to the padding -- the number of smaller indices that carry the key is added from the unsorted copy.
//   gs_ranks_count  the alternative (OSD_GSEA_RANKS=count in the environment; DESIGN.md has both timings): the D keys in LDS, one
//                   lane per used position counts the keys below and not above its own over broadcast reads.
//   gs_hits         one workgroup per (permutation, set): the set's k ranks in LDS; they are distinct, so a hit's place in the
//                   sorted order is the number of smaller ones.  Integers: exact in any order.
//   gs_scan         one workgroup per (permutation, set): the weights of the sorted hits in LDS, ONE lane adds them up one after
//                   another (C_j, the order of the definition); every lane then forms up_j and dn_j of its hits -- two divisions
//                   and one subtraction each -- and the extremes with their first hit numbers come from (value, index) butterflies,
//                   whose result no order changes.
// No atomics; a permutation's result depends on (seed, p) alone: the same bits at every perm_chunk and on every call.
// Host plumbing shared with pathway.hip: check_sets and Packed (val_common.h), PhaseClock and lower_bound (val_columns.h).
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include <hip/hip_runtime.h>
#include "handle.h"
#include "lds_sort.h"
#include "rng.h"
#include "val_columns.h"

namespace osd {
namespace {

constexpr int GS_MAX_D = 32768;            // keys of a permutation: 128 KiB of LDS
constexpr int GS_MAX_K = 1024;             // members of a set
constexpr int GS_RANK_THREADS = 1024;
constexpr int GS_SET_THREADS = 256;
constexpr int GS_MAX_CHUNK = 65535;        // permutations of a chunk: a grid dimension
constexpr double GS_MAX_WEIGHT = 1e100;    // 1024 of them still add up far below DBL_MAX
constexpr size_t GS_WORKSPACE = 64u << 20; // bytes the automatic perm_chunk fills
constexpr uint32_t GS_PAD_KEY = 0xFFFFFFFFu;

__device__ __forceinline__ uint32_t gs_key(uint64_t seed, int i, int p) { return philox_at(seed, (uint32_t)i, (uint32_t)p, 0u, TAG_GSEA).x; }

// grid (chunk), dynamic LDS N * 4 bytes; N: the power of two >= max(D, 2).  gkeys [chunk][ldk >= D], ranks [chunk][U].
__global__ __launch_bounds__(GS_RANK_THREADS) void gs_ranks_sort(uint64_t seed, int p0, int D, int N, const int* __restrict__ upos, int U,
                                                                 uint32_t* gkeys, int ldk, int* __restrict__ ranks) {
  extern __shared__ uint32_t gs_lds[];
  uint32_t* s = gs_lds;
  const int tid = threadIdx.x, p = p0 + (int)blockIdx.x;
  int* out = ranks + (size_t)blockIdx.x * U;
  if (p == 0) {                                                // the observed order; the whole workgroup leaves
    for (int u = tid; u < U; u += GS_RANK_THREADS) out[u] = upos[u];
    return;
  }
  uint32_t* gk = gkeys + (size_t)blockIdx.x * ldk;
  for (int i = tid; i < N; i += GS_RANK_THREADS) {
    const uint32_t key = i < D ? gs_key(seed, i, p) : GS_PAD_KEY;
    s[i] = key;
    if (i < D) gk[i] = key;
  }
  __syncthreads();
  lds_bitonic_sort(s, N, tid, GS_RANK_THREADS);
  for (int u = tid; u < U; u += GS_RANK_THREADS) {
    const int i = upos[u];                                     // checked by the host: in [0, D)
    const uint32_t key = gk[i];
    const int lo = lower_bound(s, 0, N, key);
    int r = lo;                                                // the keys below this one: the padding is below none
    if (lo + 1 < N && s[lo + 1] == key)                        // the key occurs again: the smaller index goes first
      for (int j = 0; j < i; ++j) r += gk[j] == key;
    out[u] = r;
  }
}

// grid (ceil(U / GS_RANK_THREADS), chunk), dynamic LDS D4 * 4 bytes, D4 = D rounded up to 4
__global__ __launch_bounds__(GS_RANK_THREADS) void gs_ranks_count(uint64_t seed, int p0, int D, const int* __restrict__ upos, int U,
                                                                  int* __restrict__ ranks) {
  extern __shared__ uint32_t gs_lds[];
  uint32_t* s = gs_lds;
  const int tid = threadIdx.x, p = p0 + (int)blockIdx.y;
  const int u = (int)blockIdx.x * GS_RANK_THREADS + tid;
  int* out = ranks + (size_t)blockIdx.y * U;
  if (p == 0) {
    if (u < U) out[u] = upos[u];
    return;
  }
  const int D4 = (D + 3) & ~3;
  for (int i = tid; i < D4; i += GS_RANK_THREADS) s[i] = i < D ? gs_key(seed, i, p) : GS_PAD_KEY;
  __syncthreads();
  if (u >= U) return;
  const int i = upos[u];
  const uint32_t key = s[i];
  const uint4* s4 = reinterpret_cast<const uint4*>(s);
  int lt = 0, le = 0;
  for (int j = 0; j < (D4 >> 2); ++j) {                        // every lane reads the same four keys: a broadcast
    const uint4 k = s4[j];
    lt += (k.x < key) + (k.y < key) + (k.z < key) + (k.w < key);
    le += (k.x <= key) + (k.y <= key) + (k.z <= key) + (k.w <= key);
  }
  int r = lt;
  if (le != lt + 1)                                            // the key occurs again (or equals the padding)
    for (int j = 0; j < i; ++j) r += s[j] == key;
  out[u] = r;
}

// grid (S, chunk).  members [M]: indices into the used positions; hits [chunk][M]: every set's ranks, ascending.
__global__ __launch_bounds__(GS_SET_THREADS) void gs_hits(const int* __restrict__ ranks, int U, const int* __restrict__ offsets,
                                                          const int* __restrict__ members, int M, int* __restrict__ hits) {
  __shared__ __attribute__((aligned(16))) int r[GS_MAX_K];
  const int tid = threadIdx.x;
  const int lo = offsets[blockIdx.x], k = offsets[blockIdx.x + 1] - lo;      // 1 <= k <= GS_MAX_K
  const int* rk = ranks + (size_t)blockIdx.y * U;
  int* out = hits + (size_t)blockIdx.y * M + lo;
  const int k4 = (k + 3) & ~3;
  for (int e = tid; e < k4; e += GS_SET_THREADS) r[e] = e < k ? rk[members[lo + e]] : INT_MAX;
  __syncthreads();
  const int4* r4 = reinterpret_cast<const int4*>(r);
  for (int e = tid; e < k; e += GS_SET_THREADS) {
    const int v = r[e];
    int c = 0;                                                 // at most k - 1: v itself is not below v
    for (int j = 0; j < (k4 >> 2); ++j) {
      const int4 q = r4[j];
      c += (q.x < v) + (q.y < v) + (q.z < v) + (q.w < v);
    }
    out[c] = v;
  }
}

// (value, hit number): the larger value, among equal ones the earlier hit
__device__ __forceinline__ void gs_take_max(double& v, int& j, double ov, int oj) { if (ov > v || (ov == v && oj < j)) { v = ov; j = oj; } }
__device__ __forceinline__ void gs_take_min(double& v, int& j, double ov, int oj) { if (ov < v || (ov == v && oj < j)) { v = ov; j = oj; } }

// grid (S, chunk).  es_pos, es_neg [chunk][S]; lead [S][2], written by the permutation 0 alone.
__global__ __launch_bounds__(GS_SET_THREADS) void gs_scan(const int* __restrict__ hits, int M, const int* __restrict__ offsets,
                                                          const double* __restrict__ w, int D, int p0, double* __restrict__ es_pos,
                                                          double* __restrict__ es_neg, int* __restrict__ lead) {
  __shared__ double c[GS_MAX_K];
  __shared__ int h[GS_MAX_K];
  __shared__ double wup[GS_SET_THREADS / 64], wdn[GS_SET_THREADS / 64];
  __shared__ int wju[GS_SET_THREADS / 64], wjd[GS_SET_THREADS / 64];
  const int tid = threadIdx.x;
  const int lo = offsets[blockIdx.x], k = offsets[blockIdx.x + 1] - lo;
  const int* in = hits + (size_t)blockIdx.y * M + lo;
  for (int e = tid; e < k; e += GS_SET_THREADS) {
    const int pos = in[e];                                     // a rank: in [0, D)
    h[e] = pos;
    c[e] = w[pos];
  }
  __syncthreads();
  if (tid == 0) {                                              // C_j = w[h_0] + ... + w[h_j], added one after another
    double a = 0.0;
    for (int j = 0; j < k; ++j) { a += c[j]; c[j] = a; }
  }
  __syncthreads();
  const double nr = c[k - 1], dk = (double)k, miss_n = (double)(D - k);      // D > k
  double up = -INFINITY, dn = INFINITY;
  int ju = INT_MAX, jd = INT_MAX;
  for (int j = tid; j < k; j += GS_SET_THREADS) {
    double hit, prev;
    if (nr == 0.0) { hit = (double)(j + 1) / dk; prev = (double)j / dk; }
    else { hit = c[j] / nr; prev = (j ? c[j - 1] : 0.0) / nr; }
    const double miss = (double)(h[j] - j) / miss_n;
    gs_take_max(up, ju, hit - miss, j);
    gs_take_min(dn, jd, prev - miss, j);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ou = __shfl_xor(up, o), od = __shfl_xor(dn, o);
    const int oju = __shfl_xor(ju, o), ojd = __shfl_xor(jd, o);
    gs_take_max(up, ju, ou, oju);
    gs_take_min(dn, jd, od, ojd);
  }
  const int wv = tid >> 6;
  if ((tid & 63) == 0) { wup[wv] = up; wdn[wv] = dn; wju[wv] = ju; wjd[wv] = jd; }
  __syncthreads();
  if (tid == 0) {
    for (int v = 1; v < GS_SET_THREADS / 64; ++v) {
      gs_take_max(up, ju, wup[v], wju[v]);
      gs_take_min(dn, jd, wdn[v], wjd[v]);
    }
    const size_t o = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    es_pos[o] = up;
    es_neg[o] = dn;
    if (p0 + (int)blockIdx.y == 0) { lead[2 * blockIdx.x] = ju; lead[2 * blockIdx.x + 1] = jd; }
  }
}

int gsea(void* stream, int device, const double* weights, int D, const int32_t* offsets, const int32_t* positions, int S, int permutations,
         uint64_t seed, int perm_chunk, double* es_pos, double* es_neg, int32_t* lead, float* phase_ms) {
  if (!weights || !offsets || !positions || !es_pos || !es_neg || !lead) { set_error("bad argument (NULL pointer)"); return OSD_EINVAL; }
  if (D < 2 || D > GS_MAX_D) { set_error("bad argument (2 <= D <= %d)", GS_MAX_D); return OSD_EINVAL; }
  if (S < 1 || permutations < 0 || perm_chunk < 0) { set_error("bad argument (S >= 1, permutations >= 0, perm_chunk >= 0)"); return OSD_EINVAL; }
  for (int i = 0; i < D; ++i)
    if (!(weights[i] >= 0.0 && weights[i] <= GS_MAX_WEIGHT)) { set_error("weight %d is negative, not finite or above 1e100", i); return OSD_EINVAL; }
  // the positions some set uses, ascending, and every member as an index into them
  std::vector<int32_t> seen, slot((size_t)D, -1);
  OSD_TRY(check_sets(offsets, positions, S, D, GS_MAX_K, "position", 'k', seen));
  const int M = offsets[S];
  std::vector<int32_t> upos;
  for (int i = 0; i < D; ++i)
    if (seen[i] >= 0) { slot[i] = (int32_t)upos.size(); upos.push_back(i); }
  const int U = (int)upos.size();
  std::vector<int32_t> members((size_t)M);
  for (int e = 0; e < M; ++e) members[e] = slot[positions[e]];

  OSD_HIP(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  const char* mode = getenv("OSD_GSEA_RANKS");
  const bool count = mode && !strcmp(mode, "count");
  int N = 2;
  while (N < D) N <<= 1;
  const int ldk = (D + 3) & ~3, D4 = ldk;
  const int64_t total = (int64_t)permutations + 1;
  const size_t per_perm = 4 * ((size_t)ldk + (size_t)U + (size_t)M) + 16 * (size_t)S;
  int64_t chunk = perm_chunk ? perm_chunk : (int64_t)(GS_WORKSPACE / per_perm);
  if (chunk < 1) chunk = 1;
  if (chunk > GS_MAX_CHUNK) chunk = GS_MAX_CHUNK;
  if (chunk > total) chunk = total;

  // one allocation: the tables (uploaded in one copy), then the chunk's buffers
  Packed ws;
  const size_t at_w = ws.put(weights, (size_t)D * sizeof(double)), at_off = ws.put(offsets, (size_t)(S + 1) * sizeof(int32_t));
  const size_t at_upos = ws.put(upos.data(), (size_t)U * sizeof(int32_t)), at_mem = ws.put(members.data(), (size_t)M * sizeof(int32_t));
  const size_t at_es = ws.take((size_t)2 * chunk * S * sizeof(double)), at_lead = ws.take((size_t)2 * S * sizeof(int32_t));
  const size_t at_keys = ws.take(count ? 0 : (size_t)chunk * ldk * sizeof(uint32_t));
  const size_t at_ranks = ws.take((size_t)chunk * U * sizeof(int32_t)), at_hits = ws.take((size_t)chunk * M * sizeof(int32_t));
  OSD_TRY(ws.alloc());
  OSD_HIP(ws.upload(st));
  OSD_HIP(hipStreamSynchronize(st));                           // the upload has left the staging vector
  const double* dw = ws.at<const double>(at_w);
  const int* doff = ws.at<const int>(at_off);
  const int* dupos = ws.at<const int>(at_upos);
  const int* dmem = ws.at<const int>(at_mem);
  uint32_t* dkeys = ws.at<uint32_t>(at_keys);
  int* dranks = ws.at<int>(at_ranks);
  int* dhits = ws.at<int>(at_hits);
  int* dlead = ws.at<int>(at_lead);
  if (count)
    OSD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(gs_ranks_count), hipFuncAttributeMaxDynamicSharedMemorySize, GS_MAX_D * 4));
  else
    OSD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(gs_ranks_sort), hipFuncAttributeMaxDynamicSharedMemorySize, GS_MAX_D * 4));
  PhaseClock<3, float> clock(phase_ms);                        // ranks, hits, scan: summed over the chunks
  OSD_HIP(clock.init());
  double* dpos = ws.at<double>(at_es);
  double* dneg = dpos + (size_t)chunk * S;

  for (int64_t p0 = 0; p0 < total; p0 += chunk) {
    const int c = (int)(total - p0 < chunk ? total - p0 : chunk);
    const dim3 sets((unsigned)S, (unsigned)c);
    OSD_HIP(clock.mark(0, st));
    if (count)
      OSD_HIP(launched(gs_ranks_count, dim3((unsigned)((U + GS_RANK_THREADS - 1) / GS_RANK_THREADS), (unsigned)c), GS_RANK_THREADS,
                       (size_t)D4 * 4, st, seed, (int)p0, D, dupos, U, dranks));
    else
      OSD_HIP(launched(gs_ranks_sort, dim3((unsigned)c), GS_RANK_THREADS, (size_t)N * 4, st, seed, (int)p0, D, N, dupos,
                       U, dkeys, ldk, dranks));
    OSD_HIP(clock.mark(1, st));
    OSD_HIP(launched(gs_hits, sets, GS_SET_THREADS, 0, st, (const int*)dranks, U, doff,
                     dmem, M, dhits));
    OSD_HIP(clock.mark(2, st));
    OSD_HIP(launched(gs_scan, sets, GS_SET_THREADS, 0, st, (const int*)dhits, M, doff,
                     dw, D, (int)p0, dpos, dneg, dlead));
    OSD_HIP(clock.mark(3, st));
    OSD_HIP(hipMemcpyAsync(es_pos + p0 * S, dpos, (size_t)c * S * sizeof(double), hipMemcpyDeviceToHost, st));
    OSD_HIP(hipMemcpyAsync(es_neg + p0 * S, dneg, (size_t)c * S * sizeof(double), hipMemcpyDeviceToHost, st));
    if (p0 == 0) OSD_HIP(hipMemcpyAsync(lead, dlead, (size_t)2 * S * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    OSD_HIP(hipStreamSynchronize(st));
    OSD_HIP(clock.add());
  }
  return OSD_OK;
}

}  // namespace
}  // namespace osd

using namespace osd;

extern "C" {

int osd_val_gsea(void* stream, int device, const double* weights_host, int D, const int32_t* set_offsets_host,
                 const int32_t* set_positions_host, int S, int permutations, uint64_t seed, int perm_chunk, double* es_pos_host,
                 double* es_neg_host, int32_t* lead_host) {
  return gsea(stream, device, weights_host, D, set_offsets_host, set_positions_host, S, permutations, seed, perm_chunk, es_pos_host,
              es_neg_host, lead_host, nullptr);
}

int osd_val_gsea_timed(void* stream, int device, const double* weights_host, int D, const int32_t* set_offsets_host,
                       const int32_t* set_positions_host, int S, int permutations, uint64_t seed, int perm_chunk, double* es_pos_host,
                       double* es_neg_host, int32_t* lead_host, float* phase_ms3) {
  if (!phase_ms3) { set_error("bad argument (NULL pointer)"); return OSD_EINVAL; }
  return gsea(stream, device, weights_host, D, set_offsets_host, set_positions_host, S, permutations, seed, perm_chunk, es_pos_host,
              es_neg_host, lead_host, phase_ms3);
}

}  // extern "C"
