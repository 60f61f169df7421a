// validate.hip -- on-GPU validation metrics (utils/validation.py): RBF-MMD as a
// blocked Gram GEMM with an exp+reduce epilogue, per-feature two-sample Kolmogorov-Smirnov extremes over
// a hand-written segmented radix sort (segsort.hip, through seg_sort), within-pathway mean correlation and Pearson correlation as
// wavefront reductions.
// Entry points are stream/device based (no model handle) and synchronous: they return host scalars.
#include <limits.h>
#include <vector>
#include "handle.h"
#include "kernels.h"
#include "launch.h"
#include "val_columns.h"

namespace osd {

__global__ void k_rowsumsq(const float* x, int64_t rows, int cols, float* out) {
  const auto [lane, wave, nw] = wave_rows();
  for (int64_t r = wave; r < rows; r += nw) {
    float s = 0.f;
    for (int c = lane; c < cols; c += 64) { const float v = x[r * cols + c]; s = fmaf(v, v, s); }
    wave_sum(s);
    if (lane == 0) out[r] = s;
  }
}

// dst[f][r] = src[r][f] for f < nf
__global__ void k_gather_cols(const float* src, int ld, int64_t rows, int nf, float* dst) {
  const int64_t total = rows * nf;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / nf;
    const int f = (int)(i - r * nf);
    dst[(int64_t)f * rows + r] = src[r * ld + f];
  }
}

// extremes over all sample points v of cnt(a<=v)*n2 - cnt(b<=v)*n1 (scipy.stats.ks_2samp's cddiffs, exact integers)
__global__ void k_ks_extremes(const float* a, const float* b, long long n1, long long n2, long long* omax, long long* omin) {
  const int f = blockIdx.y;
  const float* af = a + (long long)f * n1;
  const float* bf = b + (long long)f * n2;
  long long mx = LLONG_MIN, mn = LLONG_MAX;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n1 + n2; i += (long long)gridDim.x * blockDim.x) {
    const float v = i < n1 ? af[i] : bf[i - n1];
    const long long d = upper_bound(af, 0ll, n1, v) * n2 - upper_bound(bf, 0ll, n2, v) * n1;
    mx = d > mx ? d : mx;
    mn = d < mn ? d : mn;
  }
  wave_max(mx);
  wave_min(mn);
  if ((threadIdx.x & 63) == 0) { atomicMax(omax + f, mx); atomicMin(omin + f, mn); }
}

// per selected column: sum and sum of squares (double) -- lane j of a wave owns columns j, j+64, ...
template <int MAXJ>
__global__ void k_col_moments(const float* x, int ld, int64_t rows, const int* cols, int g, double* sum, double* sumsq) {
  const auto [lane, wave, nw] = wave_rows();
  double s[MAXJ], q[MAXJ];
  int cj[MAXJ];
#pragma unroll
  for (int j = 0; j < MAXJ; ++j) { s[j] = q[j] = 0.0; const int gi = lane + 64 * j; cj[j] = gi < g ? cols[gi] : -1; }
  for (int64_t r = wave; r < rows; r += nw)
#pragma unroll
    for (int j = 0; j < MAXJ; ++j)
      if (cj[j] >= 0) { const double v = x[r * ld + cj[j]]; s[j] += v; q[j] += v * v; }
#pragma unroll
  for (int j = 0; j < MAXJ; ++j)
    if (cj[j] >= 0) { atomicAdd(sum + lane + 64 * j, s[j]); atomicAdd(sumsq + lane + 64 * j, q[j]); }
}

// S = sum_rows (sum_g (x - mu_g) * inv_sd_g)^2
template <int MAXJ>
__global__ void k_rowz_sq(const float* x, int ld, int64_t rows, const int* cols, int g, const double* mu, const double* isd, double* out) {
  const auto [lane, wave, nw] = wave_rows();
  int cj[MAXJ];
  double m[MAXJ], w[MAXJ];
#pragma unroll
  for (int j = 0; j < MAXJ; ++j) {
    const int gi = lane + 64 * j;
    cj[j] = gi < g ? cols[gi] : -1;
    m[j] = gi < g ? mu[gi] : 0.0;
    w[j] = gi < g ? isd[gi] : 0.0;
  }
  double acc = 0.0;
  for (int64_t r = wave; r < rows; r += nw) {
    double z = 0.0;
#pragma unroll
    for (int j = 0; j < MAXJ; ++j)
      if (cj[j] >= 0) z += ((double)x[r * ld + cj[j]] - m[j]) * w[j];
    wave_sum(z);
    acc += z * z;
  }
  if (lane == 0) atomicAdd(out, acc);
}

// five sums for Pearson: n is implicit
__global__ void k_pearson_sums(const float* a, int lda, const float* b, int ldb, int64_t rows, double* out5) {
  double sa = 0, sb = 0, saa = 0, sbb = 0, sab = 0;
  for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < rows; r += (int64_t)gridDim.x * blockDim.x) {
    const double x = a[r * lda], y = b[r * ldb];
    sa += x; sb += y; saa += x * x; sbb += y * y; sab += x * y;
  }
  wave_sum(sa, sb, saa, sbb, sab);
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(out5, sa); atomicAdd(out5 + 1, sb); atomicAdd(out5 + 2, saa); atomicAdd(out5 + 3, sbb); atomicAdd(out5 + 4, sab);
  }
}

// The key arrays of EpiNearest ([nq], k = 1) and EpiKnn ([nq][k]) after the Gram pass, one wavefront per (query, slot): the index out
// of the key, and the distance to that row recomputed as sum_c (q_c - r_c)^2 -- differences in fp32, the sum in double.  The expanded
// form |r|^2 + |q|^2 - 2 r.q the keys were ranked by cancels (its error is the size of a near copy's whole distance); this one returns
// an exact copy as 0.0f.  An empty slot (all-ones: no candidate) gives idx -1, d2 +inf.
__global__ void k_knn_refine(const float* Q, int64_t nq, const float* R, int D, int k, const unsigned long long* keys, float* d2_out,
                             int32_t* idx_out) {
  const auto [lane, wave, nw] = wave_rows();
  for (int64_t w = wave; w < nq * k; w += nw) {
    const unsigned long long key = keys[w];
    if (key == EpiKnn::NO_KEY) {                   // uniform over the wave
      if (lane == 0) { idx_out[w] = -1; d2_out[w] = INFINITY; }
      continue;
    }
    const int64_t j = (int64_t)(key & 0xffffffffull);
    const float* q = Q + (w / k) * D;
    const float* r = R + j * D;
    double s = 0.0;
    for (int c = lane; c < D; c += 64) { const float d = q[c] - r[c]; s += (double)d * (double)d; }
    wave_sum(s);
    if (lane == 0) { idx_out[w] = (int32_t)j; d2_out[w] = (float)s; }
  }
}

// One thread per query: its k (d2, idx) pairs into ascending (refined d2, idx) order, in place.  The Gram pass ranked by the expanded
// form, whose rounding can order two nearly equidistant rows the other way round than their recomputed distances; the empty slots
// (+inf, -1) are at the end already and stay there.
__global__ void k_knn_sort(int64_t nq, int k, float* d2, int32_t* idx) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= nq) return;
  float* d = d2 + i * k;
  int32_t* x = idx + i * k;
  for (int a = 1; a < k; ++a) {
    const float da = d[a];
    const int32_t xa = x[a];
    if (xa < 0) break;
    int b = a;
    for (; b > 0 && (d[b - 1] > da || (d[b - 1] == da && x[b - 1] > xa)); --b) { d[b] = d[b - 1]; x[b] = x[b - 1]; }
    d[b] = da; x[b] = xa;
  }
}

// ---- the Gram-pass driver --------------------------------------------------------------------------------------------------------
// Every distance-based metric is one or more passes of the 128 x 128 Gram GEMM over two row sets of D features, with an epilogue
// (epilogues.h: EpiRbfSum, EpiNearest, EpiKnn, EpiBallCount) that turns a_f . b_p and the rows' squared norms into its figure.
// GramPass owns what those entry points share: the argument check, the device, the kernels' LDS limits, the stream, the norm
// buffer and its launches, and the GemmArgs of a pass.  An entry point adds its own checks, its outputs and their initial values,
// its epilogue arguments, and ends with finish() or a read-back: a new distance metric is a new epilogue and one more of these.
struct GramSide { const float* x; int64_t n; float* sq; };    // rows [n][D] and their squared norms

struct GramPass {
  hipStream_t s = nullptr;
  ValBuf norms;                                        // (na + nb) floats: nothing here scales with na * nb
  GramSide a{}, b{};                                   // a: the tiles' feature side (GemmArgs::A), b: their patient side
  int D = 0;

  // the argument check of every pass; extra_ok: the entry point's own part of it (its outputs, its parameters)
  static int check(const float* A, int64_t na, const float* B, int64_t nb, int D, bool extra_ok, const char* what = "bad argument") {
    if (!A || !B || !extra_ok || na <= 0 || nb <= 0 || D <= 0 || na > INT_MAX / 2 || nb > INT_MAX / 2) { set_error("%s", what); return OSD_EINVAL; }
    return OSD_OK;
  }
  int begin(void* stream, int device, const float* A, int64_t na, const float* B, int64_t nb, int D_) {
    OSD_HIP(hipSetDevice(device));
    OSD_HIP(prepare_kernels());
    s = (hipStream_t)stream;
    OSD_TRY(norms.alloc((size_t)(na + nb) * 4));
    a = GramSide{A, na, norms.as<float>()};
    b = GramSide{B, nb, norms.as<float>() + na};
    D = D_;
    return OSD_OK;
  }
  // a's norms, and b's -- a's again when b is the same rows (share: the caller wants that; a pass of a against b is then triangular)
  int compute_norms(bool share = true) {
    OSD_HIP(launched(k_rowsumsq, 1024, 256, 0, s, a.x, a.n, D, a.sq));
    if (share && a.x == b.x && a.n == b.n) b.sq = a.sq;
    else OSD_HIP(launched(k_rowsumsq, 1024, 256, 0, s, b.x, b.n, D, b.sq));
    return OSD_OK;
  }
  // One Gram GEMM: rows f on the tiles' feature side against rows p.  tri: only the tiles on or above the diagonal (f and p the same)
  template <class Epi> hipError_t run(const GramSide& f, const GramSide& p, const typename Epi::Args& ea, int tri = 0) const {
    GemmArgs g{};
    g.A = f.x; g.lda = D; g.B0 = p.x; g.ldb0 = D; g.K0 = D; g.F = (int)f.n; g.P = (int)p.n; g.K = D; g.tri = tri;
    return launch_gemm<TileBig, true, true, Epi>(s, g, ea);
  }
  int finish() const { OSD_HIP(hipStreamSynchronize(s)); return OSD_OK; }
};

// dsum[RBF_SLOTS] += sum over f, p of exp(-gamma d2(f, p))
static hipError_t rbf_sum(const GramPass& gp, const GramSide& f, const GramSide& p, float gamma, double* dsum) {
  // K(X, X) is symmetric: the tiles on or above the diagonal, the off-diagonal ones weighted 2 -- half the MFMA work of the rectangle
  static_assert(TileBig::BF == 128 && TileBig::BP == 128, "the triangular schedule compares 128-row tile indices");
  const int tri = (f.x == p.x && f.n == p.n && f.sq == p.sq) ? 1 : 0;
  return gp.run<EpiRbfSum>(f, p, EpiRbfSum::Args{f.sq, p.sq, gamma, dsum, tri}, tri);
}

// total[i] = the sum of pass i's slots, in slot order, after the stream has drained
static int rbf_totals(const GramPass& gp, const double* dslots, int passes, double* total) {
  constexpr int NS = EpiRbfSum::RBF_SLOTS;
  std::vector<double> slots((size_t)passes * NS);
  OSD_HIP(read_back(gp.s, slots.data(), dslots, slots.size() * sizeof(double)));
  for (int k = 0; k < passes; ++k) {
    total[k] = 0.0;
    for (int i = 0; i < NS; ++i) total[k] += slots[(size_t)k * NS + i];
  }
  return OSD_OK;
}

// keys [nq][k] = the k smallest keys (float_bits(d2(p, f)) << 32) | f over the reference rows f != exclude[p], ascending; keys must
// hold all-ones on entry.  One pass over the rectangle in two launches: the leading KNN_SEED reference rows first, so that the
// workgroups of the second launch find thresholds to filter by (EpiKnn); each launch takes launch_gemm's path for its own extents.
constexpr int64_t KNN_SEED = 512;
static hipError_t knn_keys(const GramPass& gp, int k, const int32_t* exclude, unsigned long long* keys) {
  const GramSide& r = gp.a;
  for (int64_t lo = 0; lo < r.n;) {
    const int64_t cnt = (lo == 0 && r.n > KNN_SEED) ? KNN_SEED : r.n - lo;
    const GramSide part{r.x + lo * gp.D, cnt, r.sq + lo};
    const hipError_t e = gp.run<EpiKnn>(part, gp.b, EpiKnn::Args{part.sq, gp.b.sq, exclude, keys, k, (int)lo});
    if (e != hipSuccess) return e;
    lo += cnt;
  }
  return hipSuccess;
}

// osd_val_nearest (k = 1) and osd_val_knn after their checks: the key array [nq][k], all-ones, filled by keys_pass(gp, keys), then
// turned into indices and recomputed distances, ascending per query
template <class KeysPass>
static int nearest_rows(void* stream, int device, const float* Q, int64_t nq, const float* R, int64_t nr, int D, int k, float* d2_out,
                        int32_t* idx_out, KeysPass keys_pass) {
  GramPass gp;                                         // a = the reference rows, b = the queries
  OSD_TRY(gp.begin(stream, device, R, nr, Q, nq, D));
  ValBuf keys;                                         // O(nq k + nr): nothing here scales with nq * nr
  OSD_TRY(keys.alloc((size_t)nq * k * sizeof(unsigned long long)));
  OSD_HIP(hipMemsetAsync(keys.get(), 0xff, (size_t)nq * k * sizeof(unsigned long long), gp.s));  // EpiNearest::NO_KEY, EpiKnn::NO_KEY
  OSD_TRY(gp.compute_norms());
  OSD_HIP(keys_pass(gp, keys.as<unsigned long long>()));
  int64_t blocks = (nq * k + 3) / 4;                   // 4 wavefronts per workgroup, one (query, slot) each
  if (blocks > 4096) blocks = 4096;
  OSD_HIP(launched(k_knn_refine, (int)blocks, 256, 0, gp.s, Q, nq, R, D, k, keys.as<const unsigned long long>(), d2_out, idx_out));
  if (k > 1) OSD_HIP(launched(k_knn_sort, (int)((nq + 255) / 256), 256, 0, gp.s, nq, k, d2_out, idx_out));
  return gp.finish();
}

}  // namespace osd

using namespace osd;

extern "C" {

int osd_val_mmd(void* stream, int device, const float* X, int64_t n, const float* Y, int64_t m, int D, double gamma, double* mmd_out) {
  OSD_TRY(GramPass::check(X, n, Y, m, D, mmd_out != nullptr));
  GramPass gp;
  OSD_TRY(gp.begin(stream, device, X, n, Y, m, D));
  constexpr int NS = EpiRbfSum::RBF_SLOTS;
  ValBuf sums;
  OSD_TRY(sums.alloc(3 * NS * sizeof(double)));
  double* d = sums.as<double>();
  OSD_HIP(hipMemsetAsync(d, 0, 3 * NS * sizeof(double), gp.s));
  OSD_TRY(gp.compute_norms(false));                                 // each operand's norms once, for the three passes below
  if (gamma <= 0) gamma = 1.0 / D;                                  // utils/validation.py:283-284
  OSD_HIP(rbf_sum(gp, gp.a, gp.a, (float)gamma, d));
  OSD_HIP(rbf_sum(gp, gp.b, gp.b, (float)gamma, d + NS));
  OSD_HIP(rbf_sum(gp, gp.a, gp.b, (float)gamma, d + 2 * NS));
  double h[3];
  OSD_TRY(rbf_totals(gp, d, 3, h));
  const double v = h[0] / ((double)n * n) + h[1] / ((double)m * m) - 2.0 * h[2] / ((double)n * m);
  *mmd_out = sqrt(v > 0 ? v : 0.0);
  return OSD_OK;
}

int osd_val_rbf_sum(void* stream, int device, const float* A, int64_t n, const float* B, int64_t m, int D, double gamma, double* sum_out) {
  OSD_TRY(GramPass::check(A, n, B, m, D, sum_out && gamma > 0, "bad argument (gamma must be > 0)"));
  GramPass gp;
  OSD_TRY(gp.begin(stream, device, A, n, B, m, D));
  ValBuf sums;
  OSD_TRY(sums.alloc(EpiRbfSum::RBF_SLOTS * sizeof(double)));
  OSD_HIP(hipMemsetAsync(sums.get(), 0, EpiRbfSum::RBF_SLOTS * sizeof(double), gp.s));
  OSD_TRY(gp.compute_norms());                         // one operand: shared norms, the symmetric (triangular) schedule of rbf_sum
  OSD_HIP(rbf_sum(gp, gp.a, gp.b, (float)gamma, sums.as<double>()));
  return rbf_totals(gp, sums.as<double>(), 1, sum_out);
}

int osd_val_nearest(void* stream, int device, const float* Q, int64_t nq, const float* R, int64_t nr, int D, const int32_t* exclude,
                    float* d2_out, int32_t* idx_out) {
  OSD_TRY(GramPass::check(R, nr, Q, nq, D, d2_out && idx_out));
  // keys[p] = min over the reference rows f != exclude[p] of (float_bits(d2(p, f)) << 32) | f
  return nearest_rows(stream, device, Q, nq, R, nr, D, 1, d2_out, idx_out, [&](const GramPass& gp, unsigned long long* keys) {
    return gp.run<EpiNearest>(gp.a, gp.b, EpiNearest::Args{gp.a.sq, gp.b.sq, exclude, keys});
  });
}

int osd_val_knn(void* stream, int device, const float* Q, int64_t nq, const float* R, int64_t nr, int D, int k, const int32_t* exclude,
                float* d2_out, int32_t* idx_out) {
  OSD_TRY(GramPass::check(R, nr, Q, nq, D, d2_out && idx_out));
  if (k < 1 || k > EpiKnn::MAX_K) { set_error("k must lie in [1, %d]", EpiKnn::MAX_K); return OSD_EINVAL; }
  return nearest_rows(stream, device, Q, nq, R, nr, D, k, d2_out, idx_out,
                      [&](const GramPass& gp, unsigned long long* keys) { return knn_keys(gp, k, exclude, keys); });
}

// in_ref[p] += #{f : d2(p, f) <= r2_ref[f]}, in_query[p] += #{f : d2(p, f) <= r2_query[p]}; either pair may be null
int osd_val_ball_counts(void* stream, int device, const float* Q, int64_t nq, const float* R, int64_t nr, int D, const float* r2_ref,
                        const float* r2_query, int32_t* in_ref_out, int32_t* in_query_out) {
  OSD_TRY(GramPass::check(R, nr, Q, nq, D, true));
  if ((!r2_ref && !r2_query) || !r2_ref != !in_ref_out || !r2_query != !in_query_out) {
    set_error("bad argument (a radius array and its output come together, and at least one pair is needed)");
    return OSD_EINVAL;
  }
  GramPass gp;
  OSD_TRY(gp.begin(stream, device, R, nr, Q, nq, D));
  if (in_ref_out) OSD_HIP(hipMemsetAsync(in_ref_out, 0, (size_t)nq * sizeof(int32_t), gp.s));
  if (in_query_out) OSD_HIP(hipMemsetAsync(in_query_out, 0, (size_t)nq * sizeof(int32_t), gp.s));
  OSD_TRY(gp.compute_norms());
  OSD_HIP(gp.run<EpiBallCount>(gp.a, gp.b, EpiBallCount::Args{gp.a.sq, gp.b.sq, r2_ref, r2_query, in_ref_out, in_query_out}));
  return gp.finish();
}

int osd_val_ks_extremes(void* stream, int device, const float* real, int64_t n1, const float* synth, int64_t n2, int ld, int nf,
                        int64_t* dmax_out, int64_t* dmin_out) {
  if (!real || !synth || !dmax_out || !dmin_out || n1 <= 0 || n2 <= 0 || nf <= 0 || nf > ld) { set_error("bad argument"); return OSD_EINVAL; }
  if ((double)n1 * nf > 2.0e9 || (double)n2 * nf > 2.0e9) { set_error("too many items for one segmented sort"); return OSD_EINVAL; }
  OSD_HIP(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  ValBuf cols, sorted, ext, tmp;
  const size_t na = (size_t)n1 * nf, nb = (size_t)n2 * nf;
  OSD_TRY(cols.alloc((na + nb) * 4));
  OSD_TRY(sorted.alloc((na + nb) * 4));
  OSD_TRY(ext.alloc((size_t)2 * nf * sizeof(long long)));
  float* ca = cols.as<float>(); float* cb = ca + na;
  float* sa = sorted.as<float>(); float* sb = sa + na;     // the sort's second buffers
  OSD_HIP(launched(k_gather_cols, 2048, 256, 0, s, real, ld, n1, nf, ca));
  OSD_HIP(launched(k_gather_cols, 2048, 256, 0, s, synth, ld, n2, nf, cb));
  // segsort.h: the sorted floats end up back in `cols`
  OSD_TRY(tmp.alloc(seg_count_bytes(n1 > n2 ? n1 : n2, nf)));
  OSD_TRY(seg_sort(s, ca, sa, (long long)n1, nf, tmp.as<int>()));
  OSD_TRY(seg_sort(s, cb, sb, (long long)n2, nf, tmp.as<int>()));
  std::vector<long long> init((size_t)2 * nf);
  for (int f = 0; f < nf; ++f) { init[f] = LLONG_MIN; init[nf + f] = LLONG_MAX; }
  long long* emax = ext.as<long long>(); long long* emin = emax + nf;
  OSD_HIP(hipMemcpyAsync(emax, init.data(), init.size() * sizeof(long long), hipMemcpyHostToDevice, s));
  int bx = (int)((n1 + n2 + 255) / 256);
  if (bx > 256) bx = 256;
  OSD_HIP(launched(k_ks_extremes, dim3(bx, nf), 256, 0, s, ca, cb, (long long)n1, (long long)n2, emax, emin));
  std::vector<long long> res((size_t)2 * nf);
  OSD_HIP(read_back(s, res.data(), emax, res.size() * sizeof(long long)));
  for (int f = 0; f < nf; ++f) { dmax_out[f] = res[f]; dmin_out[f] = res[nf + f]; }
  return OSD_OK;
}

// the grid of the one-wavefront-per-row column kernels: 16 rows per workgroup of four wavefronts, at most 1024 workgroups
static int col_blocks(int64_t rows) { const int64_t b = (rows + 15) / 16; return b > 1024 ? 1024 : (int)b; }

int osd_val_col_moments(void* stream, int device, const float* data, int64_t rows, int ld, const int32_t* cols_host, int g,
                        double* sum_host, double* sumsq_host) {
  if (!data || !sum_host || !sumsq_host || rows < 1) { set_error("bad argument"); return OSD_EINVAL; }
  hipStream_t s = (hipStream_t)stream;
  ValBuf dc, dm;
  OSD_TRY(upload_cols(device, s, cols_host, g, ld, 512, dc));
  OSD_TRY(dm.alloc((size_t)2 * g * sizeof(double)));
  OSD_HIP(hipMemsetAsync(dm.get(), 0, (size_t)2 * g * sizeof(double), s));
  OSD_HIP(launched(k_col_moments<8>, col_blocks(rows), 256, 0, s, data, ld, rows, dc.as<const int>(), g, dm.as<double>(), dm.as<double>() + g));
  std::vector<double> hm((size_t)2 * g);
  OSD_HIP(read_back(s, hm.data(), dm.get(), (size_t)2 * g * sizeof(double)));
  for (int i = 0; i < g; ++i) { sum_host[i] = hm[i]; sumsq_host[i] = hm[g + i]; }
  return OSD_OK;
}

int osd_val_rowz_sq(void* stream, int device, const float* data, int64_t rows, int ld, const int32_t* cols_host, int g, const double* mu_host,
                    const double* isd_host, double* S_host) {
  if (!data || !mu_host || !isd_host || !S_host || rows < 1) { set_error("bad argument"); return OSD_EINVAL; }
  hipStream_t s = (hipStream_t)stream;
  ValBuf dc, dm;
  OSD_TRY(upload_cols(device, s, cols_host, g, ld, 512, dc));
  OSD_TRY(dm.alloc((size_t)(2 * g + 1) * sizeof(double)));
  double* mu = dm.as<double>(); double* isd = mu + g; double* S = isd + g;
  OSD_HIP(hipMemcpyAsync(mu, mu_host, (size_t)g * sizeof(double), hipMemcpyHostToDevice, s));
  OSD_HIP(hipMemcpyAsync(isd, isd_host, (size_t)g * sizeof(double), hipMemcpyHostToDevice, s));
  OSD_HIP(hipMemsetAsync(S, 0, sizeof(double), s));
  OSD_HIP(launched(k_rowz_sq<8>, col_blocks(rows), 256, 0, s, data, ld, rows, dc.as<const int>(), g, mu, isd, S));
  OSD_HIP(read_back(s, S_host, S, sizeof(double)));
  return OSD_OK;
}

int osd_val_mean_offdiag_corr(void* stream, int device, const float* data, int64_t rows, int ld, const int32_t* cols_host, int g,
                              double* out) {
  if (!data || !cols_host || !out || rows < 2 || g < 2 || g > 512) { set_error("bad argument (2 <= genes <= 512, rows >= 2)"); return OSD_EINVAL; }
  std::vector<double> sum((size_t)g), sumsq((size_t)g), mu((size_t)g), isd((size_t)g);
  OSD_TRY(osd_val_col_moments(stream, device, data, rows, ld, cols_host, g, sum.data(), sumsq.data()));
  for (int i = 0; i < g; ++i) {
    const double m = sum[i] / rows;
    const double var = (sumsq[i] - rows * m * m) / (rows - 1);          // ddof = 1, as pandas .corr()
    mu[i] = m;
    isd[i] = var > 0 ? 1.0 / sqrt(var) : NAN;                           // constant column -> NaN, as pandas
  }
  double hs = 0;
  OSD_TRY(osd_val_rowz_sq(stream, device, data, rows, ld, cols_host, g, mu.data(), isd.data(), &hs));
  *out = (hs / (rows - 1) - g) / ((double)g * (g - 1));
  return OSD_OK;
}

int osd_val_column_sums(void* stream, int device, const float* x, int64_t rows, int ld, int cols, double* sums_host) {
  if (!x || !sums_host || rows < 1 || cols < 1 || ld < cols) { set_error("bad argument"); return OSD_EINVAL; }
  OSD_HIP(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  ValBuf d;
  OSD_TRY(d.alloc((size_t)2 * cols * sizeof(double)));
  OSD_HIP(hipMemsetAsync(d.get(), 0, (size_t)2 * cols * sizeof(double), s));
  OSD_HIP(cons_column_sums(s, x, ld, rows, cols, d.as<double>()));
  OSD_HIP(read_back(s, sums_host, d.get(), (size_t)cols * sizeof(double)));
  return OSD_OK;
}

int osd_val_gram(void* stream, int device, const float* x, int64_t rows, int ld, const int32_t* cols_host, int g, double* gram_host) {
  if (!x || !gram_host || rows < 1) { set_error("bad argument"); return OSD_EINVAL; }
  hipStream_t s = (hipStream_t)stream;
  ValBuf dc, dm, dC;
  OSD_TRY(upload_cols(device, s, cols_host, g, ld, CONS_MAX_SET, dc));
  OSD_TRY(dm.alloc((size_t)ld * sizeof(float2)));
  OSD_TRY(dC.alloc((size_t)CONS_MAX_SET * CONS_MAX_SET * sizeof(double)));
  std::vector<float2> ident((size_t)ld, make_float2(0.f, 1.f));            // no standardisation: raw products
  OSD_HIP(hipMemcpyAsync(dm.get(), ident.data(), (size_t)ld * sizeof(float2), hipMemcpyHostToDevice, s));
  OSD_HIP(hipMemsetAsync(dC.get(), 0, (size_t)CONS_MAX_SET * CONS_MAX_SET * sizeof(double), s));
  OSD_HIP(cons_gram(s, x, ld, rows, dc.as<const int>(), g, dc.as<const int>(), g, dm.as<const float2>(), dC.as<double>()));
  std::vector<double> full((size_t)CONS_MAX_SET * CONS_MAX_SET);
  OSD_HIP(read_back(s, full.data(), dC.get(), full.size() * sizeof(double)));
  for (int i = 0; i < g; ++i)
    for (int j = 0; j < g; ++j) gram_host[(size_t)i * g + j] = full[(size_t)i * CONS_MAX_SET + j];
  return OSD_OK;
}

int osd_val_pearson_sums(void* stream, int device, const float* a, int lda, const float* b, int ldb, int64_t rows, double* out5_host) {
  if (!a || !b || !out5_host || rows < 1) { set_error("bad argument"); return OSD_EINVAL; }
  OSD_HIP(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  ValBuf d;
  OSD_TRY(d.alloc(5 * sizeof(double)));
  OSD_HIP(hipMemsetAsync(d.get(), 0, 5 * sizeof(double), s));
  int blocks = (int)((rows + 255) / 256);
  if (blocks > 1024) blocks = 1024;
  OSD_HIP(launched(k_pearson_sums, blocks, 256, 0, s, a, lda, b, ldb, rows, d.as<double>()));
  OSD_HIP(read_back(s, out5_host, d.get(), 5 * sizeof(double)));
  return OSD_OK;
}

int osd_val_pearson(void* stream, int device, const float* a, int lda, const float* b, int ldb, int64_t rows, double* out) {
  if (!out || rows < 2) { set_error("bad argument"); return OSD_EINVAL; }
  double h[5];
  OSD_TRY(osd_val_pearson_sums(stream, device, a, lda, b, ldb, rows, h));
  const double n = (double)rows;
  const double cov = h[4] - h[0] * h[1] / n, va = h[2] - h[0] * h[0] / n, vb = h[3] - h[1] * h[1] / n;
  *out = cov / sqrt(va * vb);
  return OSD_OK;
}

}  // extern "C"
