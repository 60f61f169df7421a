// lds_sort.h -- the bitonic sort of N unsigned keys in LDS that gsea.hip (the keys of a permutation) and pathway.hip (the keys of a
// patient's expression row) share: N a power of two >= 2, every thread of the workgroup calls it with the same arguments after the
// keys are written and a barrier has passed; it returns behind a barrier with s ascending.  Two distances per pass on four keys per
// lane, so a pass reads and writes every key once for two stages of the network.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace osd {

// a and b in ascending (asc) or descending order
__device__ __forceinline__ void lds_sort_order(uint32_t& a, uint32_t& b, bool asc) {
  if ((a > b) == asc) { const uint32_t t = a; a = b; b = t; }
}

// tid: the thread's index in the workgroup, threads: the workgroup's size
__device__ __forceinline__ void lds_bitonic_sort(uint32_t* s, int N, int tid, int threads) {
  for (int k = 2; k <= N; k <<= 1) {                           // bitonic: runs of k keys, ascending where bit k of the index is clear
    int j = k >> 1;
    for (; j >= 2; j >>= 2) {                                  // the distances j and h = j / 2 in one pass: four keys per lane
      const int h = j >> 1;
      for (int t = tid; t < (N >> 2); t += threads) {
        const int i = ((t & ~(h - 1)) << 2) | (t & (h - 1));   // bits h and j clear: i | j | h < N; bit k is the same in all four
        const bool asc = (i & k) == 0;
        uint32_t x0 = s[i], x1 = s[i | h], x2 = s[i | j], x3 = s[i | j | h];
        lds_sort_order(x0, x2, asc); lds_sort_order(x1, x3, asc);
        lds_sort_order(x0, x1, asc); lds_sort_order(x2, x3, asc);
        s[i] = x0; s[i | h] = x1; s[i | j] = x2; s[i | j | h] = x3;
      }
      __syncthreads();
    }
    if (j == 1) {                                              // an odd number of distances: the last one alone
      for (int t = tid; t < (N >> 1); t += threads) {
        const int i = t << 1;
        uint32_t a = s[i], b = s[i | 1];
        lds_sort_order(a, b, (i & k) == 0);
        s[i] = a; s[i | 1] = b;
      }
      __syncthreads();
    }
  }
}

}  // namespace osd
