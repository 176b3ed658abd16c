/* sgl_linear_rows.h -- K22: the fused linear head of sgl_linear_head.h (K21) on STORED rows, part of libsgl_hip.so.  Opt-in
 * (fused_head="in_place" in tricks.classification).  What the models hold is a resident table of propagated rows x [n_rows, d] -- float32
 * or bfloat16 (bf16 hop storage) -- and an index list; K21 reads a dense float32 [n, d] matrix, so every step first gathered (and, for
 * bfloat16, widened) the batch into a copy that was written once and read twice.  Here both kernels read row idx[i] of the table where it
 * is stored: batch row i = x[idx[i], :], i = 0 .. m - 1.  There is no intermediate matrix.
 *
 * ARGUMENTS.  d_x: the table, n_rows rows of d elements, pitch ldx IN ELEMENTS.  d_idx: int64 [m] on the device, or NULL = identity (then
 * m must equal n_rows: the full pass over a table).  A negative index counts from the end.  An index outside [-n_rows, n_rows) never
 * traps: that batch row reads as NaN in every column, and its outputs follow (pred = 0 by K21's first-NaN rule, the loss and dz are NaN
 * if the row is live; dW is NaN in the columns it reaches) -- the rule of sgl_gather_rows_bf16_f32 and sgl_edge_dot_f32.  labels,
 * row_loss, pred, dz and z are indexed by the batch position i, not by the table row.  Everything else -- W, bias, labels, w, the outputs,
 * the scratch -- is exactly as in sgl_linear_class_f32 / sgl_linear_wgrad_f32; sgl_linear_class_rule, sgl_linear_wgrad_rule and
 * sgl_linear_wgrad_scratch apply with n = m.  m = 0: nothing is done, the weight gradient gives zeros.  n_rows = 0 with m > 0 is refused
 * (SGL_ERR_INVALID), C > SGL_LINEAR_HEAD_MAX_C returns SGL_ERR_UNSUPPORTED.  The calls run on `stream`; nothing synchronises or allocates;
 * there are no atomics.
 *
 * CONTRACT.  Batch row i of *_rows_* on (x, idx) equals, BIT FOR BIT, row i of the K21 entry point applied to the float32 matrix
 * G[i, :] = float(x[idx[i], :]) (a bfloat16 element widens exactly: its bits << 16) -- for every output and every subset of the outputs,
 * whatever the table's element type, pitch, alignment or lane width, whatever n_rows, m, duplicates in idx or its order.  dW and db equal
 * sgl_linear_wgrad_f32(G, dz) bit for bit under the same "loss_blocks".  K21's error bounds therefore apply unchanged, with x read as the
 * widened stored values.  W stays float32 (in LDS, on v_mfma_f32_32x32x2_f32): the bfloat16 matrix instruction would round W.
 *   Nothing beyond column d of the table's last row is read; pads of the outputs are not written.  Lanes of the class kernel: a float32
 * table is read in 16-byte pieces when its base is 16-byte aligned and its pitch a multiple of 4 elements, a bfloat16 table in 8-byte
 * pieces (4 elements) when its base is 8-byte aligned and its pitch a multiple of 4 elements, else element by element; W on its own rule
 * (16-byte aligned, pitch a multiple of 4).  The weight gradient reads one element per lane. */
#ifndef SGL_LINEAR_ROWS_H
#define SGL_LINEAR_ROWS_H

#include "sgl_linear_head.h"

#ifdef __cplusplus
extern "C" {
#endif

int sgl_linear_class_rows_f32(const float *d_x, int64_t ldx, int64_t n_rows, const int64_t *d_idx, int64_t m, int64_t d, const float *d_w,
                              int64_t ldw, int64_t c, const float *d_bias, const int64_t *d_labels, float w, float *d_row_loss,
                              int64_t *d_pred, float *d_dz, int64_t lddz, float *d_z, int64_t ldz, void *stream);
int sgl_linear_class_rows_bf16(const uint16_t *d_x, int64_t ldx, int64_t n_rows, const int64_t *d_idx, int64_t m, int64_t d,
                               const float *d_w, int64_t ldw, int64_t c, const float *d_bias, const int64_t *d_labels, float w,
                               float *d_row_loss, int64_t *d_pred, float *d_dz, int64_t lddz, float *d_z, int64_t ldz, void *stream);

int sgl_linear_wgrad_rows_f32(const float *d_x, int64_t ldx, int64_t n_rows, const int64_t *d_idx, int64_t m, int64_t d, const float *d_dz,
                              int64_t lddz, int64_t c, float *d_dw, int64_t lddw, float *d_db, void *d_scratch, void *stream);
int sgl_linear_wgrad_rows_bf16(const uint16_t *d_x, int64_t ldx, int64_t n_rows, const int64_t *d_idx, int64_t m, int64_t d,
                               const float *d_dz, int64_t lddz, int64_t c, float *d_dw, int64_t lddw, float *d_db, void *d_scratch,
                               void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SGL_LINEAR_ROWS_H */
