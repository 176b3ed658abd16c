// K15: the union of two canonical CSRs of one shape (columns sorted and unique inside a row), row by row, as a new canonical CSR -- the
// graph transforms of the reference that ADD entries (sgl/data/transforms.py: add_edges with del_repeated, add_self_loops;
// sgl/data/utils.py: to_undirected), which there concatenate COO lists and build a new scipy csr_matrix.  Both rows are sorted and
// unique, so the union is a merge, and the slot of every entry follows from ranks alone: with c a column of row i,
//     slot(c) = #{A's columns < c} + #{B's columns < c} - #{common columns < c}.
// Two passes like K13 (sgl_csr_select.hip): count the union of every row, scan the counts into the new row pointer (rocPRIM), write.
// No sort, no atomics, no LDS, no entry-sized temporary: the temporaries are the counts and the scan's workspace, O(n_rows).
//
// Both passes are ONE kernel template (FILL = false / true) around ONE predicate, merge_other: the rank of a column in the other
// side's row (csr_range_lower_bound, sgl_csr_search.h) and whether it is stored there -- one bisection answers both, which is what
// csr_row_find would answer with a second one.  G lanes walk a row in strides of G entries (G = 4, 16 or 64, compiled; 256 / G rows per
// workgroup, rows grid-strided):
//   * A's k-th entry goes to k + rank in B - (common columns before it): the last is the running count plus the population count of
//     the group's bits of the wavefront's 64-bit __ballot below the lane;
//   * a B entry that A stores too writes nothing (A's walk wrote the slot, with the sum or with A's value); the others go to
//     rank in A + their rank among B's own, again running count + ballot.
// The count pass walks A only: len A + len B - common.  Every slot depends on the two rows alone, so every instance, grid and stream
// writes the same bytes.  All lanes of a group share their control flow (row, trip counts), so they reach each ballot together; lanes
// of other groups that are elsewhere contribute bits the group masks away.
//
// Hostile contents never trap: a row's range is clamped into [0, nnz] before anything is read, a search reads inside that range only,
// columns are compared and copied but never index anything, and a fill never writes before the start or at or beyond the end of its
// output row (a row that is not sorted and unique, which the contract forbids, then loses entries instead of writing out of bounds).
#include "sgl_csr_search.h"
#include "sgl_rows.h"

#include <rocprim/device/device_scan.hpp>

namespace {

struct Side {
    const int64_t *rowptr;
    const int32_t *col;
    int64_t nnz;
};

struct Merge {
    Side a, b;
    int64_t n_rows;
    int mode;
};

// row i of a side as [begin, end), inside [0, nnz] whatever the row pointer holds
__device__ __forceinline__ void merge_row(const Side &s, const int64_t i, int64_t &begin, int64_t &end) {
    const int64_t lo = s.rowptr[i], hi = s.rowptr[i + 1];
    begin = lo < 0 ? 0 : lo > s.nnz ? s.nnz : lo;
    end = hi < begin ? begin : hi > s.nnz ? s.nnz : hi;
}

// is column c also stored in [begin, end) of the other side?  q: its lower bound there (the position of c when it is stored).  The one
// place where that is decided.
__device__ __forceinline__ bool merge_other(const int32_t *__restrict__ col, const int64_t begin, const int64_t end, const int32_t c, int64_t &q) {
    q = csr_range_lower_bound(col, begin, end - begin, c);
    return q < end && col[q] == c;
}

template <int G, bool FILL>
__global__ __launch_bounds__(256) void csr_merge_kernel(const Merge m, const uint32_t *__restrict__ a_val, const uint32_t *__restrict__ b_val,
                                                        int64_t *__restrict__ counts, const int64_t *__restrict__ out_rowptr,
                                                        int32_t *__restrict__ out_col, uint32_t *__restrict__ out_val,
                                                        int64_t *__restrict__ out_pos_a, int64_t *__restrict__ out_pos_b) {
    static_assert(G >= 1 && G <= 64 && (G & (G - 1)) == 0, "a group is a power-of-two part of one wavefront");
    constexpr int kRows = 256 / G;
    const int lane = threadIdx.x & (G - 1);
    const int shift = (threadIdx.x & 63) & ~(G - 1);                 // the group's first bit in the wavefront's ballot
    const uint64_t group = G == 64 ? ~0ull : ((1ull << (G & 63)) - 1);
    const uint64_t below = (1ull << lane) - 1;
    for (int64_t i = (int64_t)blockIdx.x * kRows + threadIdx.x / G; i < m.n_rows; i += (int64_t)gridDim.x * kRows) {
        int64_t a0, a1, b0, b1;
        merge_row(m.a, i, a0, a1);
        merge_row(m.b, i, b0, b1);
        int64_t out = 0, out_end = 0, common = 0;
        if (FILL) {
            out = out_rowptr[i];
            out_end = out_rowptr[i + 1];
        }
        if (FILL || (a1 > a0 && b1 > b0)) {                          // the count of a row with an empty side needs no walk
            for (int64_t base = a0; base < a1; base += G) {
                const int64_t p = base + lane;
                int32_t c = 0;
                int64_t q = b0;
                const bool both = p < a1 && merge_other(m.b.col, b0, b1, c = m.a.col[p], q);
                const uint64_t bits = ((uint64_t)__ballot(both) >> shift) & group;
                if (FILL && p < a1) {
                    const int64_t o = out + (p - a0) + (q - b0) - (common + __popcll(bits & below));
                    if (o >= out && o < out_end) {
                        uint32_t v = a_val[p];                       // the bits, whatever they mean as a float
                        if (both && m.mode == SGL_MERGE_SUM) v = __float_as_uint(__uint_as_float(v) + __uint_as_float(b_val[q]));
                        out_col[o] = c;
                        out_val[o] = v;
                        if (out_pos_a) out_pos_a[o] = p;
                        if (out_pos_b) out_pos_b[o] = both ? q : -1;
                    }
                }
                common += __popcll(bits);
            }
        }
        if (!FILL) {
            if (lane == 0) counts[i] = (a1 - a0) + (b1 - b0) - common;
            continue;
        }
        int64_t own = 0;                                             // B's entries that A does not store, so far
        for (int64_t base = b0; base < b1; base += G) {
            const int64_t p = base + lane;
            int32_t c = 0;
            int64_t q = a0;
            const bool only = p < b1 && !merge_other(m.a.col, a0, a1, c = m.b.col[p], q);
            const uint64_t bits = ((uint64_t)__ballot(only) >> shift) & group;
            if (only) {
                const int64_t o = out + (q - a0) + own + __popcll(bits & below);
                if (o >= out && o < out_end) {
                    out_col[o] = c;
                    out_val[o] = b_val[p];
                    if (out_pos_a) out_pos_a[o] = -1;
                    if (out_pos_b) out_pos_b[o] = p;
                }
            }
            own += __popcll(bits);
        }
    }
}

struct Tmp {
    std::vector<void *> ptrs;
    ~Tmp() {
        for (void *p : ptrs) (void)hipFree(p);
    }
    template <typename T>
    int alloc(const char *who, T **out, size_t count) {
        void *p = nullptr;
        hipError_t e = hipMalloc(&p, std::max<size_t>(count, 1) * sizeof(T));
        if (e != hipSuccess) return sgl::fail((int)e, "%s: hipMalloc failed: %s", who, hipGetErrorString(e));
        ptrs.push_back(p);
        *out = reinterpret_cast<T *>(p);
        return SGL_OK;
    }
};

// what both entries refuse, before any launch
int check_merge(const char *who, const int64_t *a_rowptr, const int32_t *a_col, int64_t nnz_a, const int64_t *b_rowptr, const int32_t *b_col,
                int64_t nnz_b, int64_t n_rows, int64_t n_cols, int lanes) {
    SGL_REQUIRE(n_rows >= 0 && n_cols >= 0 && nnz_a >= 0 && nnz_b >= 0, "%s: bad sizes (negative)", who);
    SGL_REQUIRE(n_rows < ((int64_t)1 << 31) && n_cols <= INT32_MAX, "%s: bad sizes (row counts must be < 2^31, column counts <= INT32_MAX)", who);
    SGL_REQUIRE(a_rowptr && a_col && b_rowptr && b_col, "%s: NULL arguments (a_rowptr, a_col, b_rowptr, b_col)", who);
    SGL_REQUIRE(lanes == 0 || lanes == 4 || lanes == 16 || lanes == 64, "%s: lanes must be 0 (auto), 4, 16 or 64", who);
    SGL_REQUIRE(aligned_to(a_rowptr, 8) && aligned_to(a_col, 4) && aligned_to(b_rowptr, 8) && aligned_to(b_col, 4),
                "%s: pointers must be aligned to their element size", who);
    return SGL_OK;
}

// lanes per row from the mean row length of the longer side (K13's rule)
int pick_lanes(int lanes, int64_t n_rows, int64_t nnz_a, int64_t nnz_b) {
    if (lanes) return lanes;
    const int64_t mean = n_rows > 0 ? std::max(nnz_a, nnz_b) / n_rows : 0;
    return mean < 8 ? 4 : mean < 32 ? 16 : 64;
}

template <bool FILL>
void launch_merge(int lanes, hipStream_t st, const Merge &m, const float *a_val, const float *b_val, int64_t *counts, const int64_t *out_rowptr,
                  int32_t *out_col, float *out_val, int64_t *out_pos_a, int64_t *out_pos_b) {
    const int64_t rows_per_block = 256 / lanes;
    int64_t blocks = (m.n_rows + rows_per_block - 1) / rows_per_block;
    if (blocks > 32768) blocks = 32768;                              // 256 CUs x 8 workgroups x 16 rounds; the rows beyond are strided
    const uint32_t *av = reinterpret_cast<const uint32_t *>(a_val), *bv = reinterpret_cast<const uint32_t *>(b_val);
    uint32_t *bits = reinterpret_cast<uint32_t *>(out_val);
    if (lanes == 4)
        hipLaunchKernelGGL((csr_merge_kernel<4, FILL>), dim3((unsigned)blocks), dim3(256), 0, st, m, av, bv, counts, out_rowptr, out_col, bits,
                           out_pos_a, out_pos_b);
    else if (lanes == 16)
        hipLaunchKernelGGL((csr_merge_kernel<16, FILL>), dim3((unsigned)blocks), dim3(256), 0, st, m, av, bv, counts, out_rowptr, out_col, bits,
                           out_pos_a, out_pos_b);
    else
        hipLaunchKernelGGL((csr_merge_kernel<64, FILL>), dim3((unsigned)blocks), dim3(256), 0, st, m, av, bv, counts, out_rowptr, out_col, bits,
                           out_pos_a, out_pos_b);
}

}  // namespace

SGL_EXPORT int sgl_csr_merge_rowptr(const int64_t *a_rowptr, const int32_t *a_col, int64_t nnz_a, const int64_t *b_rowptr, const int32_t *b_col,
                                    int64_t nnz_b, int64_t n_rows, int64_t n_cols, int lanes, int64_t *d_out_rowptr, int64_t *h_nnz_out,
                                    void *stream) {
    const char *who = "sgl_csr_merge_rowptr";
    const int rc0 = check_merge(who, a_rowptr, a_col, nnz_a, b_rowptr, b_col, nnz_b, n_rows, n_cols, lanes);
    if (rc0 != SGL_OK) return rc0;
    SGL_REQUIRE(d_out_rowptr && h_nnz_out, "sgl_csr_merge_rowptr: NULL arguments (d_out_rowptr, h_nnz_out)");
    SGL_REQUIRE(aligned_to(d_out_rowptr, 8), "sgl_csr_merge_rowptr: pointers must be aligned to their element size");
    hipStream_t st = sgl::as_stream(stream);
    if (n_rows == 0 || (nnz_a == 0 && nnz_b == 0)) {
        SGL_HIP_CHECK(hipMemsetAsync(d_out_rowptr, 0, sizeof(int64_t) * (size_t)(n_rows + 1), st));
        SGL_HIP_CHECK(hipStreamSynchronize(st));
        *h_nnz_out = 0;
        return SGL_OK;
    }
    const Merge m{{a_rowptr, a_col, nnz_a}, {b_rowptr, b_col, nnz_b}, n_rows, SGL_MERGE_SUM};
    Tmp tmp;
    int rc;
    int64_t *counts = nullptr;
    const size_t n_scan = (size_t)n_rows + 1;
    if ((rc = tmp.alloc(who, &counts, n_scan)) != SGL_OK) return rc;
    SGL_HIP_CHECK(hipMemsetAsync(counts + n_rows, 0, sizeof(int64_t), st));      // the scan's last input; every row's count is written
    launch_merge<false>(pick_lanes(lanes, n_rows, nnz_a, nnz_b), st, m, nullptr, nullptr, counts, nullptr, nullptr, nullptr, nullptr, nullptr);
    SGL_LAUNCH_CHECK(who);
    size_t bytes = 0;
    SGL_HIP_CHECK(rocprim::exclusive_scan(nullptr, bytes, counts, d_out_rowptr, (int64_t)0, n_scan, rocprim::plus<int64_t>(), st));
    char *scratch = nullptr;
    if ((rc = tmp.alloc(who, &scratch, bytes)) != SGL_OK) return rc;
    SGL_HIP_CHECK(rocprim::exclusive_scan(scratch, bytes, counts, d_out_rowptr, (int64_t)0, n_scan, rocprim::plus<int64_t>(), st));
    int64_t total = 0;
    SGL_HIP_CHECK(hipMemcpyAsync(&total, d_out_rowptr + n_rows, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    SGL_HIP_CHECK(hipStreamSynchronize(st));
    *h_nnz_out = total;
    return SGL_OK;
}

SGL_EXPORT int sgl_csr_merge_fill(const int64_t *a_rowptr, const int32_t *a_col, const float *a_val, int64_t nnz_a, const int64_t *b_rowptr,
                                  const int32_t *b_col, const float *b_val, int64_t nnz_b, int64_t n_rows, int64_t n_cols, int mode, int lanes,
                                  const int64_t *d_out_rowptr, int32_t *d_out_col, float *d_out_val, int64_t *d_out_pos_a, int64_t *d_out_pos_b,
                                  void *stream) {
    const char *who = "sgl_csr_merge_fill";
    const int rc0 = check_merge(who, a_rowptr, a_col, nnz_a, b_rowptr, b_col, nnz_b, n_rows, n_cols, lanes);
    if (rc0 != SGL_OK) return rc0;
    SGL_REQUIRE(mode == SGL_MERGE_SUM || mode == SGL_MERGE_KEEP_A, "sgl_csr_merge_fill: mode must be SGL_MERGE_SUM (0) or SGL_MERGE_KEEP_A (1)");
    SGL_REQUIRE(a_val && b_val && d_out_rowptr && d_out_col && d_out_val,
                "sgl_csr_merge_fill: NULL arguments (a_val, b_val, d_out_rowptr, d_out_col, d_out_val)");
    SGL_REQUIRE(aligned_to(a_val, 4) && aligned_to(b_val, 4) && aligned_to(d_out_rowptr, 8) && aligned_to(d_out_col, 4) && aligned_to(d_out_val, 4) &&
                    aligned_to(d_out_pos_a, 8) && aligned_to(d_out_pos_b, 8),
                "sgl_csr_merge_fill: pointers must be aligned to their element size");
    if (n_rows == 0 || (nnz_a == 0 && nnz_b == 0)) return SGL_OK;
    const Merge m{{a_rowptr, a_col, nnz_a}, {b_rowptr, b_col, nnz_b}, n_rows, mode};
    launch_merge<true>(pick_lanes(lanes, n_rows, nnz_a, nnz_b), sgl::as_stream(stream), m, a_val, b_val, nullptr, d_out_rowptr, d_out_col, d_out_val,
                       d_out_pos_a, d_out_pos_b);
    SGL_LAUNCH_CHECK(who);
    return SGL_OK;
}
