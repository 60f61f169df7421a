// segsort.h -- the segmented LSD radix sort of fp32 keys over equal-length segments, as its callers see it (the kernels and the
// pass loop are in segsort.hip, compiled once): osd_val_ks_extremes, osd_val_marginals and osd_val_group_ranks sort their column
// segments with seg_sort.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace osd {

constexpr int SEG_CHUNK = 4096;           // keys per wave and pass
constexpr int SEG_WAVES = 4;              // waves per workgroup

// the order-preserving uint32 image of a float, and back
__device__ __forceinline__ uint32_t f2key(float f) {
  const uint32_t u = __float_as_uint(f);
  return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float key2f(uint32_t k) {
  return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu));
}

// waves per segment of n keys, and the bytes of the count buffer seg_sort needs for nf such segments: cnt[seg][digit][wave]
inline int seg_wps(long long n) { return (int)((n + SEG_CHUNK - 1) / SEG_CHUNK); }
inline size_t seg_count_bytes(long long n, int nf) { return (size_t)nf * 256 * (size_t)seg_wps(n) * sizeof(int); }

// The four stable 8-bit passes over nf segments of n floats each, ping-pong between buf0 and buf1 (nf * n floats each): the sorted
// floats come back in buf0.  cnt: seg_count_bytes(n, nf) at least.  nf * n <= 2e9.  Returns OSD_OK or OSD_EHIP.
int seg_sort(hipStream_t s, float* buf0, float* buf1, long long n, int nf, int* cnt);

}  // namespace osd
