/* sgl_linear_head.h -- K21: a linear classification head fused with its loss, part of libsgl_hip.so.  Opt-in (fused_head=True in
 * tricks.classification): the torch head (addmm, then K14 on the logits, two rocBLAS products in the backward) stays the default.
 *
 * (1) sgl_linear_class_f32: the logits Z = X W^T + b are formed on v_mfma_f32_32x32x2_f32 and never leave the registers unless asked for;
 * K14's per-row work (sgl_class_loss_grad_f32, sgl_hip.h) runs on the accumulators.  x [n, d] (pitch ldx), W [C, d] in nn.Linear's layout
 * (pitch ldw), bias [C] or NULL, labels int64 [n] or NULL, a scalar weight w.  Row i is LIVE iff 0 <= labels[i] < C.  Outputs, each
 * optional, at least one required (when n > 0):
 *   row_loss[i] = logsumexp(Z[i]) - Z[i, labels[i]]          0 for a row that is not live
 *   dz[i, j]    = w (softmax(Z[i])_j - [j = labels[i]])      0 for a row that is not live                         (pitch lddz)
 *   pred[i]     = the lowest index of the row's maximum; a NaN counts as the maximum, the first NaN wins         (every row)
 *   z[i, j]     = Z[i, j]                                                                                          (every row; pitch ldz)
 * With neither row_loss nor dz no exponential is evaluated and labels may be NULL.  C <= SGL_LINEAR_HEAD_MAX_C: a larger C returns
 * SGL_ERR_UNSUPPORTED.  n = 0: nothing is done.  d = 0: Z = b.
 *
 * CONTRACT.  No atomics, no scratch; two runs are bit-equal, and so is every subset of the outputs.  A row's outputs do not depend on n
 * or on where the row stands.  A logit is ONE chain over the columns: for every group of 8 columns in ascending order and e = 0 .. 3,
 * acc = acc + W[j, 8 q + e] x[i, 8 q + e] + W[j, 8 q + 4 + e] x[i, 8 q + 4 + e] (one MFMA step; columns >= d are zeros), then + b[j]
 * once.  The order depends on d alone: not on C, the class's slot, the pitches, the alignment or the column chunks.  Nothing beyond
 * column d of a last row of x or W is read; pads of the outputs are not written.  16-byte lanes when a matrix's base is 16-byte aligned
 * and its pitch a multiple of 4 floats (x and W together; dz and z each on its own), else one float per access.  "loss_blocks"
 * (sgl_set_tuning) caps the grid as it does for K9.  The kernel runs on `stream`.
 *
 * ERROR BOUNDS (u = 2^-24; first order; T_ij = sum_col |W[j, col] x[i, col]| + |b[j]|).
 *   logits   |z - Z|           <= E_ij = (d + 3) u T_ij                            (a term passes one product, <= d adds, the bias add)
 * With E_i = max_j E_ij, m = max_j Z_ij, p = softmax(Z[i]) and lse = logsumexp(Z[i]) in exact arithmetic:
 *   row_loss |l - L_i|         <= 2 E_i + (C + 16) 2^-23 + 2^-23 (|lse| + |L_i|)
 *   dz       |dz - dZ_ij|      <= |w| (p_j (expm1(2 E_i) + (C + 8 + |Z_ij - m|) 2^-23) + 2^-23)
 *   pred     Z[i, pred_i]      >= m - 2 E_i                                        (finite rows)
 * How: logsumexp moves by at most E_i and Z[i, y] by E_i when every logit moves by at most E_i; p_j by the factor exp(2 E_i).  On the
 * logits as formed: z - m is one rounding (relative u |z - m| on the exponential), expf and logf are within 2 ulp (the device library
 * states 1), the sum of the C exponentials is in [1, C] and has relative error (C + 2) 2^-23, the logarithm of it adds 2 ulp of a
 * value <= log 256, and m + log s, - z_y, the division, the subtraction of the one and the product with w are one rounding each.
 *
 * (2) sgl_linear_wgrad_f32: dW = dZ^T X [C, d] (pitch lddw) and db = the column sums of dZ [C], deterministic.  Two kernels.  B row
 * blocks x S slabs of output tiles: a workgroup owns R consecutive rows and a slab of CT x UT tiles of 32 classes x 32 columns
 * (CT = 1 / 2 / 4 / 8 covers C, UT = 8 / CT; db is the column d of an X extended by ones); its four wavefronts keep the slab in
 * accumulator registers, wavefront v takes the row pairs v, v + 4, ... of the block in ascending order, one MFMA step per pair, and
 * the four are added in LDS as ((v0 + v1) + v2) + v3; the workgroup writes one table to the scratch.  A fold adds the B tables of
 * every (j, col) in ascending block order, one float32 add each.  n = 0 gives zeros.
 *   BLOCKS.  R >= 40 C (d + 1) / d rows (the tables are at most 5 % of the traffic of X), B = ceil(n / R) <= 2048; "loss_blocks" > 0
 * REPLACES the choice as in sgl_cluster_sums.h: B = ceil(n / ceil(n / min(loss_blocks, n, 2048))).
 *   ORDER.  The bits of dW and db depend on (the values of x and dz, n, d, C, B) alone -- not on pitches or alignment (every access is
 * one float).  Two runs are bit-equal.  Error: |dW[j, col] - exact| <= (R / 2 + B + 8) u sum_i |dz[i, j] x[i, col]| (first order): a
 * term passes one product, at most R / 4 + 1 adds in its wavefront, 3 adds in LDS and B in the fold; db the same with x = 1.
 * dX = dZ W is not computed here (pre-propagated features need no gradient).  Nothing synchronises or allocates: d_scratch
 * (sgl_linear_wgrad_scratch bytes, 16-byte aligned) is the caller's.
 * The same two kernels on rows idx[i] of a stored float32 or bfloat16 table, without the gathered copy: sgl_linear_rows.h (K22). */
#ifndef SGL_LINEAR_HEAD_H
#define SGL_LINEAR_HEAD_H

#include "sgl_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SGL_LINEAR_HEAD_MAX_C 256

int sgl_linear_class_f32(const float *d_x, int64_t ldx, int64_t n, int64_t d, const float *d_w, int64_t ldw, int64_t c, const float *d_bias,
                         const int64_t *d_labels, float w, float *d_row_loss, int64_t *d_pred, float *d_dz, int64_t lddz, float *d_z,
                         int64_t ldz, void *stream);

/* Host only: the instance a call takes.  rule[0] = accumulator tiles of 32 classes (the compiled count that covers c), rule[1] = row
 * tiles of 32 rows per wavefront, rule[2] = columns of W held in LDS at once (a multiple of 8; d rounded up to 8 when all fit),
 * rule[3] = their row pitch in LDS in floats (rule[2] + 4).  LDS of a workgroup: (c rule[3] + 32 rule[0]) floats <= 64 KiB. */
int sgl_linear_class_rule(int64_t d, int64_t c, int rule[4]);

/* Host only: out[0] = row blocks B, out[1] = rows per block R (both 0 when n = 0), out[2] = class tiles per slab CT, out[3] = column
 * tiles per slab UT, out[4] = slabs S = ceil(ceil((d + 1) / 32) / UT); reads "loss_blocks". */
int sgl_linear_wgrad_rule(int64_t n, int64_t d, int64_t c, int64_t *out);

/* bytes of the partial tables: B x S tables of 32 CT x 32 UT floats; -1 for sizes the rule refuses */
int64_t sgl_linear_wgrad_scratch(int64_t n, int64_t d, int64_t c);

int sgl_linear_wgrad_f32(const float *d_x, int64_t ldx, int64_t n, int64_t d, const float *d_dz, int64_t lddz, int64_t c, float *d_dw,
                         int64_t lddw, float *d_db, void *d_scratch, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SGL_LINEAR_HEAD_H */
