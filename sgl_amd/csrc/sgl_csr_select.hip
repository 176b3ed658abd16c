// K13: filter a canonical CSR (columns sorted and unique inside a row) into a new canonical CSR -- the graph transforms of the
// reference (sgl/data/transforms.py: get_subgraph, random_drop_nodes, drop_edges, biased_drop_edges, random_drop_edges,
// remove_self_loops), which there go through a COO edge list, a boolean index and a new scipy csr_matrix.  A stable compaction
// under monotone new ids keeps the columns of a row sorted and unique, so a transform is two passes over the entries: count the kept
// entries of every output row, scan the counts into the new row pointer (rocPRIM, the setup path's library call, like ingest), then
// write the kept entries.  No sort, no atomics, no LDS, no entry-sized temporary: the only temporaries are the counts and the scan's
// workspace, O(n_rows_out).
//
// Both passes are ONE kernel template (FILL = false / true) around ONE predicate, select_keep, so the count and the fill cannot
// disagree.  G lanes walk a row in strides of G entries (G = 4, 16 or 64, compiled; 256 / G rows per workgroup, rows grid-strided).
// Inside a stride the slot of a kept entry is the running count plus the population count of the group's bits of the wavefront's
// 64-bit __ballot below the lane: stable, and independent of G and of the grid, so every instance writes the same bytes.  All lanes of
// a group share their control flow (row, trip count), so they reach the ballot together; lanes of other groups that are elsewhere
// contribute bits the group masks away.
//
// Hostile contents never trap: a map value outside [0, n_out) and a column outside [0, n_cols) count as dropped before anything is
// indexed by them, the search of the symmetric mask stays inside one row of the source, and a fill never writes at or beyond the end
// of its output row (a map that sends two rows to one, which the contract forbids, then loses entries instead of writing out of bounds).
#include "sgl_csr_search.h"
#include "sgl_hash.h"
#include "sgl_rows.h"

#include <rocprim/device/device_scan.hpp>

namespace {

constexpr uint64_t kEdgeDropStream = 103;

struct Select {
    const int64_t *rowptr;
    const int32_t *col;
    int64_t n_rows, n_cols;
    const int32_t *row_map, *col_map;     // old id -> new id, NULL = identity
    int64_t n_rows_out, n_cols_out;
    const uint8_t *keep;                  // [nnz] or NULL
    int symmetric_mask, drop_self, symmetric;
    uint64_t drop_below, seed;
};

// is entry p = (i, col[p]) of the source kept?  cj: its output column.  The one place where that is decided.
__device__ __forceinline__ bool select_keep(const Select &s, const int64_t i, const int64_t p, int32_t &cj) {
    const int32_t j = s.col[p];
    if (j < 0 || j >= s.n_cols) return false;
    cj = s.col_map ? s.col_map[j] : j;
    if (cj < 0 || cj >= s.n_cols_out) return false;
    if (s.drop_self && i == j) return false;
    if (s.keep) {
        int64_t q = p;
        if (s.symmetric_mask && j < i) q = j < s.n_rows ? csr_row_find(s.rowptr, s.col, j, (int32_t)i) : -1;   // i < 2^31 (host check)
        if (q < 0 || !s.keep[q]) return false;                                  // a lower entry without a stored mirror is dropped
    }
    if (s.drop_below) {
        const bool swap = s.symmetric && j < i;
        const uint64_t a = swap ? (uint64_t)j : (uint64_t)i, b = swap ? (uint64_t)i : (uint64_t)j;
        if (hash4(s.seed, kEdgeDropStream, a, b) < s.drop_below) return false;
    }
    return true;
}

template <int G, bool FILL>
__global__ __launch_bounds__(256) void csr_select_kernel(const Select s, const float *__restrict__ val, int64_t *__restrict__ counts,
                                                         const int64_t *__restrict__ out_rowptr, int32_t *__restrict__ out_col,
                                                         uint32_t *__restrict__ out_val, int64_t *__restrict__ out_pos) {
    static_assert(G >= 1 && G <= 64 && (G & (G - 1)) == 0, "a group is a power-of-two part of one wavefront");
    constexpr int kRows = 256 / G;
    const int lane = threadIdx.x & (G - 1);
    const int shift = (threadIdx.x & 63) & ~(G - 1);                 // the group's first bit in the wavefront's ballot
    const uint64_t group = G == 64 ? ~0ull : ((1ull << (G & 63)) - 1);
    const uint64_t below = (1ull << lane) - 1;
    for (int64_t i = (int64_t)blockIdx.x * kRows + threadIdx.x / G; i < s.n_rows; i += (int64_t)gridDim.x * kRows) {
        const int64_t ri = s.row_map ? (int64_t)s.row_map[i] : i;
        if (ri < 0 || ri >= s.n_rows_out) continue;                  // the whole group leaves: nothing of this row is read
        const int64_t begin = s.rowptr[i], end = s.rowptr[i + 1];
        int64_t out = 0, out_end = 0, run = 0;
        if (FILL) {
            out = out_rowptr[ri];
            out_end = out_rowptr[ri + 1];
        }
        for (int64_t base = begin; base < end; base += G) {
            const int64_t p = base + lane;
            int32_t cj = 0;
            const bool kept = p < end && select_keep(s, i, p, cj);
            const uint64_t bits = ((uint64_t)__ballot(kept) >> shift) & group;
            if (FILL && kept) {
                const int64_t o = out + run + __popcll(bits & below);
                if (o < out_end) {
                    out_col[o] = cj;
                    out_val[o] = reinterpret_cast<const uint32_t *>(val)[p];     // the bits, whatever they mean as a float
                    if (out_pos) out_pos[o] = p;
                }
            }
            run += __popcll(bits);
        }
        if (!FILL && lane == 0) counts[ri] = run;
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
int check_select(const char *who, const int64_t *d_rowptr, const int32_t *d_col, int64_t n_rows, int64_t n_cols, int64_t nnz,
                 const int32_t *d_row_map, const int32_t *d_col_map, int64_t n_rows_out, int64_t n_cols_out, const uint8_t *d_entry_keep,
                 int symmetric_mask, int lanes) {
    SGL_REQUIRE(n_rows >= 0 && n_cols >= 0 && nnz >= 0 && n_rows_out >= 0 && n_cols_out >= 0, "%s: bad sizes (negative)", who);
    SGL_REQUIRE(n_rows < ((int64_t)1 << 31) && n_rows_out < ((int64_t)1 << 31) && n_cols <= INT32_MAX && n_cols_out <= INT32_MAX,
                "%s: bad sizes (row counts must be < 2^31, column counts <= INT32_MAX)", who);
    SGL_REQUIRE(d_row_map || n_rows_out == n_rows, "%s: bad sizes (without a row map n_rows_out must be n_rows)", who);
    SGL_REQUIRE(d_col_map || n_cols_out == n_cols, "%s: bad sizes (without a column map n_cols_out must be n_cols)", who);
    SGL_REQUIRE(d_rowptr && d_col, "%s: NULL arguments (d_rowptr, d_col)", who);
    SGL_REQUIRE(!symmetric_mask || d_entry_keep, "%s: NULL arguments (symmetric_mask needs d_entry_keep)", who);
    SGL_REQUIRE(lanes == 0 || lanes == 4 || lanes == 16 || lanes == 64, "%s: lanes must be 0 (auto), 4, 16 or 64", who);
    SGL_REQUIRE(aligned_to(d_rowptr, 8) && aligned_to(d_col, 4) && aligned_to(d_row_map, 4) && aligned_to(d_col_map, 4),
                "%s: pointers must be aligned to their element size", who);
    return SGL_OK;
}

// lanes per row from the mean row length: a group wider than a row leaves lanes idle, a narrower one walks it in more strides
int pick_lanes(int lanes, int64_t n_rows, int64_t nnz) {
    if (lanes) return lanes;
    const int64_t mean = n_rows > 0 ? nnz / n_rows : 0;
    return mean < 8 ? 4 : mean < 32 ? 16 : 64;
}

template <bool FILL>
void launch_select(int lanes, hipStream_t st, const Select &s, const float *val, int64_t *counts, const int64_t *out_rowptr, int32_t *out_col,
                   float *out_val, int64_t *out_pos) {
    const int64_t rows_per_block = 256 / lanes;
    int64_t blocks = (s.n_rows + rows_per_block - 1) / rows_per_block;
    if (blocks > 32768) blocks = 32768;                              // 256 CUs x 8 workgroups x 16 rounds; the rows beyond are strided
    uint32_t *bits = reinterpret_cast<uint32_t *>(out_val);
    if (lanes == 4)
        hipLaunchKernelGGL((csr_select_kernel<4, FILL>), dim3((unsigned)blocks), dim3(256), 0, st, s, val, counts, out_rowptr, out_col, bits, out_pos);
    else if (lanes == 16)
        hipLaunchKernelGGL((csr_select_kernel<16, FILL>), dim3((unsigned)blocks), dim3(256), 0, st, s, val, counts, out_rowptr, out_col, bits, out_pos);
    else
        hipLaunchKernelGGL((csr_select_kernel<64, FILL>), dim3((unsigned)blocks), dim3(256), 0, st, s, val, counts, out_rowptr, out_col, bits, out_pos);
}

}  // namespace

SGL_EXPORT int sgl_csr_select_rowptr(const int64_t *d_rowptr, const int32_t *d_col, int64_t n_rows, int64_t n_cols, int64_t nnz,
                                     const int32_t *d_row_map, const int32_t *d_col_map, int64_t n_rows_out, int64_t n_cols_out,
                                     const uint8_t *d_entry_keep, int symmetric_mask, int drop_self, uint64_t drop_below, uint64_t seed,
                                     int symmetric, int lanes, int64_t *d_out_rowptr, int64_t *h_nnz_out, void *stream) {
    const char *who = "sgl_csr_select_rowptr";
    const int rc0 = check_select(who, d_rowptr, d_col, n_rows, n_cols, nnz, d_row_map, d_col_map, n_rows_out, n_cols_out, d_entry_keep,
                                 symmetric_mask, lanes);
    if (rc0 != SGL_OK) return rc0;
    SGL_REQUIRE(d_out_rowptr && h_nnz_out, "sgl_csr_select_rowptr: NULL arguments (d_out_rowptr, h_nnz_out)");
    SGL_REQUIRE(aligned_to(d_out_rowptr, 8), "sgl_csr_select_rowptr: pointers must be aligned to their element size");
    hipStream_t st = sgl::as_stream(stream);
    if (nnz == 0 || n_rows == 0 || n_rows_out == 0 || n_cols_out == 0) {
        SGL_HIP_CHECK(hipMemsetAsync(d_out_rowptr, 0, sizeof(int64_t) * (size_t)(n_rows_out + 1), st));
        SGL_HIP_CHECK(hipStreamSynchronize(st));
        *h_nnz_out = 0;
        return SGL_OK;
    }
    const Select s{d_rowptr, d_col, n_rows, n_cols, d_row_map, d_col_map, n_rows_out, n_cols_out, d_entry_keep, symmetric_mask, drop_self,
                   symmetric, drop_below, seed};
    Tmp tmp;
    int rc;
    int64_t *counts = nullptr;
    const size_t n_scan = (size_t)n_rows_out + 1;
    if ((rc = tmp.alloc(who, &counts, n_scan)) != SGL_OK) return rc;
    SGL_HIP_CHECK(hipMemsetAsync(counts, 0, sizeof(int64_t) * n_scan, st));      // rows that no source row maps to have length 0
    launch_select<false>(pick_lanes(lanes, n_rows, nnz), st, s, nullptr, counts, nullptr, nullptr, nullptr, nullptr);
    SGL_LAUNCH_CHECK(who);
    size_t bytes = 0;
    SGL_HIP_CHECK(rocprim::exclusive_scan(nullptr, bytes, counts, d_out_rowptr, (int64_t)0, n_scan, rocprim::plus<int64_t>(), st));
    char *scratch = nullptr;
    if ((rc = tmp.alloc(who, &scratch, bytes)) != SGL_OK) return rc;
    SGL_HIP_CHECK(rocprim::exclusive_scan(scratch, bytes, counts, d_out_rowptr, (int64_t)0, n_scan, rocprim::plus<int64_t>(), st));
    int64_t total = 0;
    SGL_HIP_CHECK(hipMemcpyAsync(&total, d_out_rowptr + n_rows_out, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    SGL_HIP_CHECK(hipStreamSynchronize(st));
    *h_nnz_out = total;
    return SGL_OK;
}

SGL_EXPORT int sgl_csr_select_fill(const int64_t *d_rowptr, const int32_t *d_col, const float *d_val, int64_t n_rows, int64_t n_cols, int64_t nnz,
                                   const int32_t *d_row_map, const int32_t *d_col_map, int64_t n_rows_out, int64_t n_cols_out,
                                   const uint8_t *d_entry_keep, int symmetric_mask, int drop_self, uint64_t drop_below, uint64_t seed,
                                   int symmetric, int lanes, const int64_t *d_out_rowptr, int32_t *d_out_col, float *d_out_val,
                                   int64_t *d_out_pos, void *stream) {
    const char *who = "sgl_csr_select_fill";
    const int rc0 = check_select(who, d_rowptr, d_col, n_rows, n_cols, nnz, d_row_map, d_col_map, n_rows_out, n_cols_out, d_entry_keep,
                                 symmetric_mask, lanes);
    if (rc0 != SGL_OK) return rc0;
    SGL_REQUIRE(d_val && d_out_rowptr && d_out_col && d_out_val, "sgl_csr_select_fill: NULL arguments (d_val, d_out_rowptr, d_out_col, d_out_val)");
    SGL_REQUIRE(aligned_to(d_val, 4) && aligned_to(d_out_rowptr, 8) && aligned_to(d_out_col, 4) && aligned_to(d_out_val, 4) &&
                    aligned_to(d_out_pos, 8),
                "sgl_csr_select_fill: pointers must be aligned to their element size");
    if (nnz == 0 || n_rows == 0 || n_rows_out == 0 || n_cols_out == 0) return SGL_OK;
    const Select s{d_rowptr, d_col, n_rows, n_cols, d_row_map, d_col_map, n_rows_out, n_cols_out, d_entry_keep, symmetric_mask, drop_self,
                   symmetric, drop_below, seed};
    launch_select<true>(pick_lanes(lanes, n_rows, nnz), sgl::as_stream(stream), s, d_val, nullptr, d_out_rowptr, d_out_col, d_out_val, d_out_pos);
    SGL_LAUNCH_CHECK(who);
    return SGL_OK;
}
