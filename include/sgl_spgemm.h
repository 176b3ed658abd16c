/* sgl_spgemm.h -- K17: the product of two canonical device CSRs as a new canonical CSR, part of libsgl_hip.so.
 *
 * C = A . B with A [m, k] and B [k, n]: rowptr int64 (m + 1 / k + 1 offsets), col int32, val float32, columns ascending and unique inside
 * a row; C comes out the same way.  The reference forms such products with scipy (sgl/data/base_dataset.py:313-396,
 * sample_by_meta_path, "# extremely slow"); here it is two calls in the shape of sgl_csr_select_* / sgl_csr_merge_* (sgl_hip.h): the
 * first writes C's row pointer and returns its number of entries through the host, the second fills C's columns and values.
 *
 * Conventions are those of sgl_hip.h: every function returns SGL_OK or an error code (text: sgl_last_error()); pointers named d_* are
 * device pointers, h_* host pointers; the last argument is the HIP stream (NULL: the default one).
 *
 * PATTERN.  Structural: (i, c) is stored iff some stored A[i, j] meets a stored B[j, c].  A sum that comes out exactly zero STAYS
 * stored, as in sgl_csr_merge_*.  scipy's product drops such entries: [[1, -1], [2, 3]] @ [[1, 0], [1, 5]] in float32 has 3 stored
 * entries there and 4 here.
 *
 * VALUES.
 *   SGL_SPGEMM_SUM   v(i, c) = the chain  acc = 0;  for the entries j of A's row i in storage order with B[j, c] stored:
 *                    acc = fadd_rn(acc, fmul_rn(A[i, j], B[j, c])).  The product is rounded, then the sum; nothing is contracted to an
 *                    fma.  This is the arithmetic of scipy's float32 csr_matmat.  No atomic touches a value: every row class, window
 *                    size, grid and stream writes the same bytes.
 *   SGL_SPGEMM_ONES  every stored value is 1.0; a_val and b_val are never read (they may be NULL).
 *
 * FORCING ARGUMENTS (0 = auto; any other value must be one a compiled instance serves, else SGL_ERR_INVALID by name):
 *   narrow_cap   rows with at most this many candidate products (sum over A's row of the lengths of B's rows) are expanded, sorted
 *                and compressed in LDS, the others go through an LDS bitmap: SGL_SPGEMM_NARROW_CAPS.
 *   window_cols  columns one bitmap covers: SGL_SPGEMM_WINDOWS.
 * sgl_csr_matmul_rule resolves both on the host (no device is touched).
 *
 * HOSTILE CONTENTS NEVER TRAP.  Row ranges are clamped into [0, nnz]; a column of A outside [0, k) is an empty row of B; a column of B
 * outside [0, n) is skipped; a fill never writes outside its output row.
 *
 * m, k, n < 2^31; every entry offset, nnz(C) and a row's candidate count are 64-bit. */
#ifndef SGL_SPGEMM_H
#define SGL_SPGEMM_H

#include "sgl_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SGL_SPGEMM_SUM 0
#define SGL_SPGEMM_ONES 1
#define SGL_SPGEMM_NARROW_CAPS {32, 128, 512}       /* LDS slice of a row: 4, 16, 64 lanes per row          */
#define SGL_SPGEMM_WINDOWS {1024, 32768, 524288}    /* bitmap of a workgroup: 128 B, 4 KB, 64 KB of LDS     */

/* h_rule[0] = the narrow cap, h_rule[1] = the window that a call with these arguments uses (auto: the largest cap; the smallest
 * window that covers n columns, else the largest). */
int sgl_csr_matmul_rule(int narrow_cap, int window_cols, int64_t n, int *h_rule);

/* d_out_rowptr [m + 1] <- C's row pointer; *h_nnz_out <- nnz(C).  Synchronises the stream (the total comes back through the host). */
int sgl_csr_matmul_rowptr(const int64_t *a_rowptr, const int32_t *a_col, int64_t nnz_a, const int64_t *b_rowptr, const int32_t *b_col,
                          int64_t nnz_b, int64_t m, int64_t k, int64_t n, int narrow_cap, int window_cols, int64_t *d_out_rowptr,
                          int64_t *h_nnz_out, void *stream);

/* d_out_col / d_out_val [nnz(C)] <- C's columns and values under `mode`, for the row pointer the first call wrote (same arguments). */
int sgl_csr_matmul_fill(const int64_t *a_rowptr, const int32_t *a_col, const float *a_val, int64_t nnz_a, const int64_t *b_rowptr,
                        const int32_t *b_col, const float *b_val, int64_t nnz_b, int64_t m, int64_t k, int64_t n, int mode, int narrow_cap,
                        int window_cols, const int64_t *d_out_rowptr, int32_t *d_out_col, float *d_out_val, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SGL_SPGEMM_H */
