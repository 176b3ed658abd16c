/* sgl_hop_rows.h -- K24: the learnable hop aggregators on STORED hop rows, part of libsgl_hip.so.  Opt-in
 * (config.aggregate_in_place).  A GAMLP-style model holds H resident hop tables [n_rows, d] -- float32 or bfloat16 (bf16 hop storage)
 * -- and trains on an index list.  The float32 aggregator kernels of sgl_hip.h (row-dot scores, weighted sum, its backward, column
 * sums) read dense [n, d] matrices, so every step first gathered (and, for bfloat16, widened) the B x H x d mini-batch rows into a
 * float32 copy.  The kernels here read row idx[i] of every table where it is stored; there is no intermediate matrix.
 *
 * ROW SOURCE (every entry point).  h_x: HOST array of n_hops <= SGL_HOP_ROWS_MAX_HOPS device pointers, one element type; h_ldx: HOST
 * array of their pitches IN ELEMENTS (NULL: every pitch is d rounded up to 4).  Every table has n_rows rows of d <=
 * SGL_HOP_ROWS_MAX_D columns.  d_idx: int64 [m] on the device, or NULL = identity (then m must equal n_rows).  A negative index
 * counts from the end.  An index outside [-n_rows, n_rows) never traps: that row reads as NaN in each of its d columns, and the
 * outputs it enters follow (its scores, its output row, its dW row; every column sum).  Rows must be 16-byte aligned (float32) or
 * 8-byte aligned (bfloat16) on pitches that are multiples of 4 elements: the vector that straddles column d is read inside the
 * row's pitch and masked.  Anything else -- and n_hops or d beyond the limits -- returns SGL_ERR_UNSUPPORTED with the entry's name in
 * sgl_last_error(); NULL tables, bad sizes, m != n_rows without an index, a table without rows under m > 0 return SGL_ERR_INVALID.
 * m = 0: nothing is launched, SGL_OK.  The calls run on `stream`; nothing synchronises or allocates; there are no atomics.
 *
 * CONTRACT.  With G_h[i, :] = float(X_h[idx[i], :]) (a bfloat16 element widens exactly: its bits << 16), scores, wsum and wsum_bwd
 * equal, BIT FOR BIT, the float32 entry points of sgl_hip.h for the row-dot pair, the 2-D weighted sum and its dW, applied to the
 * G_h, whatever the tables' element type, pitch or m: the same lane layout, the same lane order of every reduction, the same fma
 * chain in hop order.  colsum folds in a fixed order of its own that depends on (m, d) only: two runs give the same bits.
 *
 *   scores    P[i, h - h0] = <X_h[idx_i], vec> for h in [h0, h1), ldp >= h1 - h0;  A[i] = sum over the hops j with bit j of u_mask
 *             set of <X_j[idx_i], U[j, :]> (U: [n_hops, ldu]; u_mask = 0: no A, the plain gate scores -- then in the lane layout of
 *             the plain row-dot of sgl_hip.h, whose bits P has, which are also the scores inside the one-pass gate kernel).  vec and U are 16-byte
 *             aligned and zero-padded to whole vectors (ldu a multiple of 4).
 *   wsum      out[i, :] = sum_h W[i ldw + h] X_h[idx_i, :], one fma chain from 0 in hop order; ldw = 0: one weight vector for every
 *             row.  out: float32 on its own pitch ldo; pad_cols columns after d are the row's declared padding and are written as
 *             zeros (d + pad_cols and ldo multiples of 4).
 *   wsum_bwd  dW[i, h] = <dOut[i, :], X_h[idx_i, :]>; dOut: dense float32 [m, d] on pitch lddo, dword-aligned.  There is no dX: the
 *             stored tables carry no gradient.
 *   colsum    out[h, :] = sum_i w[i ldw + h sw] X_h[idx_i, :]: sw = 1, one weight per row and hop (ldw >= n_hops); sw = 0, one per
 *             row for every hop.  d_scratch: sgl_hop_rows_colsum_scratch floats, 16-byte aligned.  m = 0 leaves out untouched. */
#ifndef SGL_HOP_ROWS_H
#define SGL_HOP_ROWS_H

#include <stdint.h>

#define SGL_HOP_ROWS_MAX_HOPS 16
#define SGL_HOP_ROWS_MAX_D 512

#ifdef __cplusplus
extern "C" {
#endif

int sgl_hop_rows_scores_f32(int n_hops, const float *const *h_x, const int64_t *h_ldx, int64_t n_rows, const int64_t *d_idx, int64_t m,
                            const float *d_u, int64_t ldu, uint64_t u_mask, const float *d_vec, int h0, int h1, float *d_p, int64_t ldp,
                            float *d_a, int64_t d, void *stream);
int sgl_hop_rows_scores_bf16(int n_hops, const uint16_t *const *h_x, const int64_t *h_ldx, int64_t n_rows, const int64_t *d_idx, int64_t m,
                             const float *d_u, int64_t ldu, uint64_t u_mask, const float *d_vec, int h0, int h1, float *d_p, int64_t ldp,
                             float *d_a, int64_t d, void *stream);

int sgl_hop_rows_wsum_f32(int n_hops, const float *const *h_x, const int64_t *h_ldx, int64_t n_rows, const int64_t *d_idx, int64_t m,
                          const float *d_w, int64_t ldw, float *d_out, int64_t ldo, int64_t pad_cols, int64_t d, void *stream);
int sgl_hop_rows_wsum_bf16(int n_hops, const uint16_t *const *h_x, const int64_t *h_ldx, int64_t n_rows, const int64_t *d_idx, int64_t m,
                           const float *d_w, int64_t ldw, float *d_out, int64_t ldo, int64_t pad_cols, int64_t d, void *stream);

int sgl_hop_rows_wsum_bwd_f32(int n_hops, const float *const *h_x, const int64_t *h_ldx, int64_t n_rows, const int64_t *d_idx, int64_t m,
                              const float *d_dout, int64_t lddo, float *d_dw, int64_t lddw, int64_t d, void *stream);
int sgl_hop_rows_wsum_bwd_bf16(int n_hops, const uint16_t *const *h_x, const int64_t *h_ldx, int64_t n_rows, const int64_t *d_idx, int64_t m,
                               const float *d_dout, int64_t lddo, float *d_dw, int64_t lddw, int64_t d, void *stream);

/* floats of scratch the column sums need for m output rows; 0 for arguments outside the limits */
int64_t sgl_hop_rows_colsum_scratch(int n_hops, int64_t m, int64_t d);
int sgl_hop_rows_colsum_f32(int n_hops, const float *const *h_x, const int64_t *h_ldx, int64_t n_rows, const int64_t *d_idx, int64_t m,
                            const float *d_w, int64_t ldw, int sw, float *d_out, int64_t ldo, float *d_scratch, int64_t d, void *stream);
int sgl_hop_rows_colsum_bf16(int n_hops, const uint16_t *const *h_x, const int64_t *h_ldx, int64_t n_rows, const int64_t *d_idx, int64_t m,
                             const float *d_w, int64_t ldw, int sw, float *d_out, int64_t ldo, float *d_scratch, int64_t d, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SGL_HOP_ROWS_H */
