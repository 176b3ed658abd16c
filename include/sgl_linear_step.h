/* sgl_linear_step.h -- K23: the training step of the linear head of sgl_linear_head.h (K21) in ONE pass over X, part of libsgl_hip.so.
 * Opt-in (fused_head="one_pass" / "one_pass_in_place" in tricks.classification).  K21's step is two launches and a fold: the class kernel
 * reads X and writes dZ [n, C], the weight gradient reads dZ and X again.  Here launch 1 reads every row of X once, through the class
 * kernel's wide lanes, and leaves the row losses, the arg-max and one partial table of (dW | db) per row block; dZ never leaves the chip.
 * Launch 2 is K21's ordered fold.
 *
 * ARGUMENTS.  As sgl_linear_class_f32 (x, W, bias, labels, w, row_loss, pred) and sgl_linear_wgrad_f32 (dW [C, d] pitch lddw, db [C], the
 * scratch); the *_rows_* entry points read batch row i from row idx[i] of a stored float32 / bfloat16 table with the conventions of
 * sgl_linear_rows.h (ldx in elements, idx NULL = identity and then m = n_rows, negative indices count from the end, an index out of
 * range reads as a row of NaN and never traps).  dW and db are REQUIRED, labels too; row_loss and pred are optional.  n = 0: the step
 * kernel is not launched and the fold writes zeros.  The kernels run on `stream`; nothing synchronises or allocates: d_scratch
 * (sgl_linear_step_scratch bytes, 16-byte aligned) is the caller's.
 *
 * SHAPES.  A wavefront keeps ALL of (dW | db) in accumulator registers: CT x TU tiles of 32 classes x 32 columns, CT = 1 / 2 / 4 the
 * class tiles that cover C, TU = ceil((d + 1) / 32) (column d of X reads as 1, so db rides along), next to the 32 rows it is working on.
 * Supported: C <= SGL_LINEAR_STEP_MAX_C = 128 and TU <= 7 for CT = 1, TU <= 4 for CT = 2, TU <= 2 for CT = 4 -- C <= 32 up to d = 222,
 * C <= 64 up to d = 127, C <= 128 up to d = 63.  These are the instances that compile without scratch memory: 8 tiles next to 8 column
 * tiles of the row (C <= 32, d = 223 .. 254) and 8 class tiles of logits next to 8 tiles of dW (C > 128) spill, and are not compiled.
 * Any other shape returns SGL_ERR_UNSUPPORTED; nothing falls back.
 *
 * WORK.  B row blocks of R rows: sgl_linear_wgrad_rule's B and R ("loss_blocks" replaces the choice as there).  One workgroup of four
 * wavefronts per block, no slabs.  Wavefront v takes the block's tiles of 32 rows v, v + 4, ... in ascending order.  Per tile: the rows
 * are loaded once into registers (16 bytes per lane, 8 for bfloat16); the logits form on v_mfma_f32_32x32x2_f32 with W in LDS -- K21's
 * chain; K21's epilogue gives row_loss, pred and dz in the accumulator layout; per class tile the dz tile, per column tile the X tile
 * goes through a wavefront-private LDS tile of 32 x 32 floats (pitch 36) and comes back transposed: step s = 0 .. 15 of a tile pair
 * multiplies rows (16 (s / 8) + s % 8) and that + 8 of the tile.  After its last tile the four wavefronts are added in LDS as
 * ((v0 + v1) + v2) + v3 and ONE table per workgroup goes to the scratch; the fold adds the B tables in ascending block order.
 *   LDS of a workgroup, bytes: 4 max(C (8 ceil(d / 8) + 4) + 32 CT + 4 * 32 * 36, 8192) <= 53 760 (C = 128, d = 63): W, the bias, four
 * tiles; the 32 KiB of the last addition alias them.  No launch asks for more than 64 KiB.
 *
 * CONTRACT.  No atomics.  Two runs are bit-equal.  row_loss and pred are bit-equal to sgl_linear_class_f32 on the same rows (the same
 * chain, the same epilogue).  The *_rows_* entry points are bit-equal, in every output, to sgl_linear_step_f32 on
 * G[i, :] = float(x[idx[i], :]).  The bits of dW and db depend on (the values, n, d, C, B) alone -- not on pitches, alignment or lane
 * width; they are NOT those of sgl_linear_wgrad_f32: the order of the rows inside a block differs.  Nothing beyond column d of a last
 * row of x or W is read; pads of dW are not written.
 *
 * ERROR BOUND of dW[j, col] (db: x = 1), first order, u = 2^-24, dz and its bound from sgl_linear_head.h:
 *   sum_i |x[i, col]| (K21's dz bound for (i, j)) + (A + B + 8) u sum_i |dz[i, j] x[i, col]|,   A = 32 ceil(ceil(R / 32) / 4)
 * A term passes one product, at most A adds in its wavefront (ceil(ceil(R / 32) / 4) tiles of 16 steps of 2 adds), 3 adds in LDS and B
 * in the fold.  A < R / 4 + 32. */
#ifndef SGL_LINEAR_STEP_H
#define SGL_LINEAR_STEP_H

#include "sgl_linear_rows.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SGL_LINEAR_STEP_MAX_C 128

/* Host only: out[0] = row blocks B, out[1] = rows per block R (both 0 when n = 0), out[2] = class tiles CT, out[3] = column tiles TU,
 * out[4] = LDS bytes of a workgroup.  SGL_ERR_UNSUPPORTED for a shape outside SHAPES (the message states the rule); reads "loss_blocks". */
int sgl_linear_step_rule(int64_t n, int64_t d, int64_t c, int64_t *out);

/* bytes of the partial tables: B tables of 8192 floats; -1 for sizes the rule refuses */
int64_t sgl_linear_step_scratch(int64_t n, int64_t d, int64_t c);

int sgl_linear_step_f32(const float *d_x, int64_t ldx, int64_t n, int64_t d, const float *d_w, int64_t ldw, int64_t c, const float *d_bias,
                        const int64_t *d_labels, float w, float *d_row_loss, int64_t *d_pred, float *d_dw, int64_t lddw, float *d_db,
                        void *d_scratch, void *stream);
int sgl_linear_step_rows_f32(const float *d_x, int64_t ldx, int64_t n_rows, const int64_t *d_idx, int64_t m, int64_t d, const float *d_w,
                             int64_t ldw, int64_t c, const float *d_bias, const int64_t *d_labels, float w, float *d_row_loss,
                             int64_t *d_pred, float *d_dw, int64_t lddw, float *d_db, void *d_scratch, void *stream);
int sgl_linear_step_rows_bf16(const uint16_t *d_x, int64_t ldx, int64_t n_rows, const int64_t *d_idx, int64_t m, int64_t d,
                              const float *d_w, int64_t ldw, int64_t c, const float *d_bias, const int64_t *d_labels, float w,
                              float *d_row_loss, int64_t *d_pred, float *d_dw, int64_t lddw, float *d_db, void *d_scratch, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SGL_LINEAR_STEP_H */
