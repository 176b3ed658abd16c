/* sgl_ensemble.h -- K16: the sub-graph ensemble aggregators of the heterogeneous models (NARS), part of libsgl_hip.so.
 *
 * The reference's *OneDimConvolution modules (sgl/models/simple_models.py:5-84, read by BaseHeteroSGAPModel / FastBaseHeteroSGAPModel,
 * sgl/models/base_model.py:69-222) take the rows x[idx] of M = n_groups * group_size propagated matrices, stack them, multiply by
 * learnable weights and reduce over the members of every group.  Here that is ONE pass: every input element is read once, every
 * output element written once, nothing is stacked.
 *
 * Conventions are those of sgl_hip.h: every function returns SGL_OK or an error code (text: sgl_last_error()); pointers named d_* are
 * device pointers, h_* host arrays; leading dimensions are in elements; the last argument is the HIP stream (NULL: the default one).
 * Matrix m = g * group_size + s is member s of group g.  The scratch query returns a number of floats. */
#ifndef SGL_ENSEMBLE_H
#define SGL_ENSEMBLE_H

#include "sgl_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SGL_ENSEMBLE_MAX_GROUP 64    /* members of one group  */
#define SGL_ENSEMBLE_MAX_MEMBERS 256 /* matrices of one call  */

/* out_g[i, f] = ( sum_{s < group_size} X_{g,s}[idx[i], f] * W[(g * group_size + s) * ldw + f * cs] ) / divisor,   g < n_groups.
 *
 * h_x / h_ldx: the M matrices, [n_rows, d] each, in member order; a matrix may be a row view into a larger buffer (pointer at its first
 *   row, the buffer's pitch).  d_idx: n_idx int64 row indices on the device, or NULL: all rows in order (n_idx must then be n_rows).
 *   A negative index counts from the end; an index outside [-n_rows, n_rows) makes that output row NaN -- the kernel never traps.
 * d_w: the weight table, M rows of ldw floats; cs = 0: one weight per matrix (column 0 of its row), cs = 1: one per matrix and column.
 * The sum is one fma chain in member order that starts from the first (rounded) product; then a TRUE division by `divisor`, skipped
 *   when divisor == 1.
 * h_out / h_ldo: the n_groups outputs, [n_idx, d] each (a concatenated slab is n_groups pointers d apart on one pitch).  Columns
 *   [d, d + pad_cols) of every output row are the row's own padding and are written as zeros (see sgl_hip.h, "Row outputs and padding").
 * Rows are read and written 16 bytes per lane when every pointer is 16-byte aligned and every pitch a multiple of 4 floats, element by
 *   element otherwise; nothing beyond column d of an input's last row is read.  Outputs must not alias inputs.
 * group_size <= SGL_ENSEMBLE_MAX_GROUP, M <= SGL_ENSEMBLE_MAX_MEMBERS, d + pad_cols <= SGL_MAX_WIDTH: else SGL_ERR_UNSUPPORTED. */
int sgl_ensemble_combine_f32(int n_groups, int group_size, const float *const *h_x, const int64_t *h_ldx, int64_t n_rows,
                             const int64_t *d_idx, int64_t n_idx, const float *d_w, int64_t ldw, int cs, float divisor,
                             float *const *h_out, const int64_t *h_ldo, int64_t pad_cols, int64_t d, void *stream);

/* Weight gradient of the above (the matrices are constants of the model: there is no dX):
 *   cs = 1:  d_dw[m * lddw + f] = ( sum_i dOut_{g(m)}[i, f] * X_m[idx[i], f] ) / divisor
 *   cs = 0:  d_dw[m * lddw]     = ( sum_i sum_f dOut_{g(m)}[i, f] * X_m[idx[i], f] ) / divisor
 * h_dout / h_lddo: the n_groups incoming gradients, [n_idx, d] each.  A fixed two-level reduction through d_scratch (16-byte aligned,
 * >= sgl_ensemble_combine_bwd_scratch(...) floats), no atomics: two runs give the same bits.  A row whose index is out of range
 * contributes NaN, as the forward's row is NaN. */
int64_t sgl_ensemble_combine_bwd_scratch(int n_groups, int group_size, int64_t n_idx, int64_t d, int cs);
int sgl_ensemble_combine_bwd_f32(int n_groups, int group_size, const float *const *h_x, const int64_t *h_ldx, int64_t n_rows,
                                 const int64_t *d_idx, int64_t n_idx, const float *const *h_dout, const int64_t *h_lddo, int cs,
                                 float divisor, float *d_dw, int64_t lddw, float *d_scratch, int64_t d, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SGL_ENSEMBLE_H */
