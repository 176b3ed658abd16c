// The search inside one row of a canonical CSR (columns sorted and unique inside a row), shared by sgl_edge_split.hip (K10: is a pair
// stored?), sgl_csr_select.hip (K13: the upper entry of a lower entry's pair) and sgl_csr_merge.hip (K15: a column's rank in the other
// side's row, and whether it is stored there).  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

// the p in [rowptr[row], rowptr[row + 1]) with col[p] == v, or -1.  The range [lo, lo + n) always holds v's position if there is
// one: probe the last element of the lower half, keep one half.
__device__ __forceinline__ int64_t csr_row_find(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col, const int64_t row,
                                                const int32_t v) {
    int64_t lo = rowptr[row];
    int64_t n = rowptr[row + 1] - lo;
    if (n <= 0) return -1;
    while (n > 1) {
        const int64_t half = n >> 1;
        const bool up = col[lo + half - 1] < v;      // v lies beyond the lower half
        lo = up ? lo + half : lo;
        n = up ? n - half : half;
    }
    return col[lo] == v ? lo : -1;
}

// the lower bound, csr_row_find's sibling: the first p in [lo, lo + n) with col[p] >= v, or lo + n when every column is below v -- the
// number of columns below v, counted from lo.  The same halving: the answer always lies in [lo, lo + n].  Nothing outside
// [lo, lo + n) is read whatever the columns hold (sorted or not), and n <= 0 reads nothing.
__device__ __forceinline__ int64_t csr_range_lower_bound(const int32_t *__restrict__ col, int64_t lo, int64_t n, const int32_t v) {
    while (n > 0) {
        const int64_t half = n >> 1;
        const bool up = col[lo + half] < v;          // v lies beyond the probe
        lo = up ? lo + half + 1 : lo;
        n = up ? n - half - 1 : half;
    }
    return lo;
}

}  // namespace
