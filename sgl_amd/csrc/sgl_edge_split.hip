// K10: "is (i, j) a stored entry?" for a list of pairs, and the candidate stream of the negative edges of a link-prediction split --
// what the reference's mask_test_edges (sgl/tasks/utils.py:148-259) does with a Python set of every stored edge and one
// np.random.randint pair at a time (lines 166-168 and 181-236).  Gather-shaped like the rest of the library: each answer is a search
// inside ONE row of a canonical CSR (columns sorted and unique inside a row) -- two rowptr reads and ceil(log2(len + 1)) dependent
// probes of col, no nnz-sized key array.
//
// Layout.  One lane per query, 256 queries per workgroup, index loads and stores coalesced.  The bisection step is a pair of selects,
// no branch; a lane's trip count is its own row's.  14-16 VGPRs, 8 wavefronts per SIMD: the dependent loads of one query are hidden
// by the other wavefronts, not by more queries per lane -- 2, 4 and 8 queries per lane in lockstep were measured at the products
// shape and took 1.6-1.8 x as long.  No LDS, no atomics, plain vector stores.
//
// Indices (sgl_csr_find): negative ones count from the end; one still outside its range gives -1 and reads NOTHING.  The kernels
// never trap.  sgl_edge_candidates draws its own indices, in range by construction.
#include "sgl_csr_search.h"
#include "sgl_hash.h"
#include "sgl_rows.h"

namespace {

using i64x2 = long __attribute__((ext_vector_type(2)));
static_assert(sizeof(i64x2) == 16, "an edge is two int64");

__global__ __launch_bounds__(256) void csr_find_kernel(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col, const int64_t n_rows,
                                                       const int64_t n_cols, const int64_t *__restrict__ edges, const int edges16,
                                                       const int64_t n_q, int64_t *__restrict__ out) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= n_q) return;
    int64_t s, t;
    if (edges16) {
        const i64x2 p = *reinterpret_cast<const i64x2 *>(edges + 2 * q);
        s = p[0];
        t = p[1];
    } else {                                         // an edge list that starts on an odd multiple of 8 bytes
        s = edges[2 * q];
        t = edges[2 * q + 1];
    }
    if (s < 0) s += n_rows;                          // python-style negative index
    if (t < 0) t += n_cols;
    const bool ok = s >= 0 && s < n_rows && t >= 0 && t < n_cols;
    out[q] = ok ? csr_row_find(rowptr, col, s, (int32_t)t) : -1;     // n_cols <= INT32_MAX (host check)
}

// candidate t: the ordered pair (i, j) = (mulhi64(h(seed, 102, t, 0), n), mulhi64(h(seed, 102, t, 1), n)); its key is the unordered
// pair as one integer, min * n + max (< 2^62 for n < 2^31), when i != j and (i, j) is not stored, else -1
__global__ __launch_bounds__(256) void edge_candidates_kernel(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col, const int64_t n,
                                                              const uint64_t seed, const int64_t first, const int64_t count,
                                                              int64_t *__restrict__ edges, const int edges16, int64_t *__restrict__ key) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= count) return;
    const uint64_t t = (uint64_t)first + (uint64_t)q;
    const int64_t i = (int64_t)mulhi64(hash4(seed, 102, t, 0), (uint64_t)n);
    const int64_t j = (int64_t)mulhi64(hash4(seed, 102, t, 1), (uint64_t)n);
    if (edges16) {
        i64x2 p;
        p[0] = i;
        p[1] = j;
        *reinterpret_cast<i64x2 *>(edges + 2 * q) = p;
    } else {
        edges[2 * q] = i;
        edges[2 * q + 1] = j;
    }
    const bool free_pair = i != j && csr_row_find(rowptr, col, i, (int32_t)j) < 0;      // a self pair is refused without a search
    key[q] = free_pair ? (i < j ? i * n + j : j * n + i) : -1;
}

}  // namespace

SGL_EXPORT int sgl_csr_find(const int64_t *d_rowptr, const int32_t *d_col, int64_t n_rows, int64_t n_cols, const int64_t *d_edges, int64_t n_q,
                            int64_t *d_pos, void *stream) {
    SGL_REQUIRE(n_q >= 0 && n_rows >= 0 && n_cols >= 0 && n_cols <= INT32_MAX, "sgl_csr_find: bad sizes");
    SGL_REQUIRE(d_rowptr && d_col && d_edges && d_pos, "sgl_csr_find: NULL arguments");
    SGL_REQUIRE(aligned_to(d_rowptr, 8) && aligned_to(d_col, 4) && aligned_to(d_edges, 8) && aligned_to(d_pos, 8),
                "sgl_csr_find: pointers must be aligned to their element size");
    if (n_q == 0) return SGL_OK;
    const int64_t blocks = (n_q + 255) / 256;
    if (!sgl::launch_fits(blocks, 256)) return sgl::fail(SGL_ERR_UNSUPPORTED, "sgl_csr_find: too many pairs for one launch (split the list)");
    hipLaunchKernelGGL(csr_find_kernel, dim3((unsigned)blocks), dim3(256), 0, sgl::as_stream(stream), d_rowptr, d_col, n_rows, n_cols, d_edges,
                       aligned_to(d_edges, 16) ? 1 : 0, n_q, d_pos);
    SGL_LAUNCH_CHECK("sgl_csr_find");
    return SGL_OK;
}

SGL_EXPORT int sgl_edge_candidates(const int64_t *d_rowptr, const int32_t *d_col, int64_t n, uint64_t seed, int64_t first, int64_t count,
                                   int64_t *d_edges, int64_t *d_key, void *stream) {
    SGL_REQUIRE(n >= 1 && n < ((int64_t)1 << 31), "sgl_edge_candidates: bad sizes (1 <= n < 2^31)");
    SGL_REQUIRE(first >= 0 && count >= 0 && first <= INT64_MAX - count, "sgl_edge_candidates: bad sizes (first, count)");
    SGL_REQUIRE(d_rowptr && d_col && d_edges && d_key, "sgl_edge_candidates: NULL arguments");
    SGL_REQUIRE(aligned_to(d_rowptr, 8) && aligned_to(d_col, 4) && aligned_to(d_edges, 8) && aligned_to(d_key, 8),
                "sgl_edge_candidates: pointers must be aligned to their element size");
    if (count == 0) return SGL_OK;
    const int64_t blocks = (count + 255) / 256;
    if (!sgl::launch_fits(blocks, 256))
        return sgl::fail(SGL_ERR_UNSUPPORTED, "sgl_edge_candidates: too many candidates for one launch (split the list)");
    hipLaunchKernelGGL(edge_candidates_kernel, dim3((unsigned)blocks), dim3(256), 0, sgl::as_stream(stream), d_rowptr, d_col, n, seed, first, count,
                       d_edges, aligned_to(d_edges, 16) ? 1 : 0, d_key);
    SGL_LAUNCH_CHECK("sgl_edge_candidates");
    return SGL_OK;
}
