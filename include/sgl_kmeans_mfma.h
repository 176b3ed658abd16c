/* sgl_kmeans_mfma.h -- K18: the k-means assignment step on the matrix cores, part of libsgl_hip.so.  Opt-in: sgl_kmeans_assign_f32
 * (sgl_hip.h, K9) stays the default and keeps its bits.
 *
 * labels[i] = argmin_j |x_i - c_j|^2 searched in the CENTRED EXPANDED form: with x' = fl(x - shift), c' = fl(c - shift) the score of
 * centre j is fmaf(-2, <c'_j, x'_i>, |c'_j|^2), the products on v_mfma_f32_32x32x2_f32 (|x'_i|^2 is the same for every j and is never
 * formed).  The shift moves both sides, so the distances are unchanged in exact arithmetic; it is what makes the expanded form usable
 * on data with an offset (NAFS features are non-negative).  d_shift: [d] floats, or NULL = no shift; callers pass the mean of the
 * centres.
 *
 * mindist[i] (optional) is the DIRECT form sum_c (x_ic - c_jc)^2 for the centre j = labels[i] that was chosen, on the uncentred data:
 * relative error (d + 3) 2^-24 for THAT centre whatever the offset of the data; its summation order depends on d alone.  It is not
 * bit-equal to K9's mindist (the order differs).
 *
 * CONTRACT.  No atomics; two runs are bit-equal; a row's outputs do not depend on n or on where the row stands.  The lowest index
 * wins among equal scores; a NaN score never wins: a row holding NaN gets label 0 and mindist NaN.  A row holding +-Inf gets SOME
 * label in [0, k) and the direct-form value for it (unspecified; K9 differs here).  On finite rows the label L may differ from the
 * exact argmin b only when the two centres are closer than the rounding of the form: D[i, L] - D[i, b] <= 2 (E_L + E_b) with
 * E_j = (d + 3) 2^-23 (|c'_j|^2 + 2 |x'_i| |c'_j|) + 2^-23 sqrt(D[i, j]) (|x'_i| + |c'_j|).
 *
 * Conventions, checks, alignment rules (16-byte lanes when both bases are 16-byte aligned and both pitches multiples of 4 floats, else
 * one float per access), n = 0 (nothing is done) and d = 0 (labels 0, distances 0) are those of sgl_kmeans_assign_f32.  The pads of
 * the caller's buffers are never used and nothing beyond column d of a last row is read.  k <= SGL_KMEANS_MATRIX_MAX_K; a larger k
 * returns SGL_ERR_UNSUPPORTED.  "loss_blocks" (sgl_set_tuning) caps the grid as it does for K9. */
#ifndef SGL_KMEANS_MFMA_H
#define SGL_KMEANS_MFMA_H

#include "sgl_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SGL_KMEANS_MATRIX_MAX_K 256

int sgl_kmeans_assign_matrix_f32(const float *d_x, int64_t ldx, int64_t n, int64_t d, const float *d_centres, int64_t ldc, int64_t k,
                                 const float *d_shift, int64_t *d_labels, float *d_mindist, void *stream);

/* Host only: the instance a call with these sizes takes.  rule[0] = accumulator tiles of 32 centres (the compiled count that covers
 * k), rule[1] = row tiles of 32 rows per wavefront, rule[2] = columns of the centres held in LDS at once (a multiple of 8; >= d rounded
 * up to 8 when all fit), rule[3] = their row pitch in LDS in floats.  vec4: 16-byte lanes (1) or one float per access (0). */
int sgl_kmeans_assign_matrix_rule(int64_t d, int64_t k, int vec4, int rule[4]);

#ifdef __cplusplus
}
#endif
#endif /* SGL_KMEANS_MFMA_H */
