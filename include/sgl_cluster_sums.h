/* sgl_cluster_sums.h -- K19: the per-cluster column sums and counts of the k-means centre update in one pass over X, part of
 * libsgl_hip.so.  Opt-in: kmeans(update="spmm"), the membership-matrix SpMM, stays the default and keeps its bits.
 *
 *   sums[j, c] = sum over {i : labels[i] = j} of x[i, c]          counts[j] = #{i : labels[i] = j}
 *
 * An empty cluster gives a zero row and a zero count.  A row whose label is outside [0, k) is skipped: nothing is indexed by it and
 * it is not read into any sum.  n = 0 gives zeros; d = 0 gives the counts alone; neither starts the partial kernel.  Only columns
 * 0 .. d - 1 of the k rows of d_sums are written (pitch lds >= d floats: the pads keep what they held).  The call is ordered on
 * `stream`, synchronises nothing and allocates nothing: d_scratch (sgl_cluster_sums_scratch bytes, 16-byte aligned) is the caller's.
 *
 * TWO KERNELS, no sort, no CSR, no plan, no atomics.  (1) B row blocks x S column slabs: a workgroup owns R consecutive rows and one
 * slab of columns, keeps k x slab float32 accumulators in LDS, and adds its rows to them in ascending row order; it writes its table
 * and (slab 0) its int32 counts to the scratch.  (2) A fold adds the B tables of every (j, c) in ascending block order, one float32
 * add per block, and the counts into int64.
 *
 * LDS BUDGET AND SGL_CLUSTER_SUMS_MAX_K.  A workgroup's LDS -- k x slab float32 accumulators and k int32 counts -- is at most 64 KiB
 * (16 384 words: what a launch gets without asking for more, and two workgroups fit a CU's 160 KiB).  The slab is the whole row (dp = d
 * rounded up to 4) while k x (dp + 1) words fit, else the row is cut into S = ceil(dp / floor4(16384 / k - 1)) slabs of
 * round_up4(ceil(dp / S)) columns.  MAX_K = 1024 is the largest power of two that leaves a slab of three 16-byte vectors per row
 * (floor4(16384 / 1024 - 1) = 12 columns; 2048 would leave 4); a larger k returns SGL_ERR_UNSUPPORTED.  Every slab is read by its own
 * workgroups, so X is still read once overall.
 *
 * BLOCKS.  R >= 40 k dp / d rows, B = ceil(n / R) <= 2048: a table is written once and read once (2 k dp floats) against the R d
 * floats of X its block reads, so the tables' traffic is at most 5 % of X (5.0 % at n = 2 449 029, k = 47, d = 100: B = 1302,
 * R = 1881) and no block holds fewer rows than make its table worth writing.  The tuning key "loss_blocks" (sgl_set_tuning), when
 * > 0, REPLACES that choice: B = ceil(n / ceil(n / min(loss_blocks, n, 2048))).  B and R are functions of (n, d, k, loss_blocks) alone.
 *
 * ORDER GUARANTEE.  The bits of d_sums depend on (the values of x, labels, n, d, k, B) -- not on the 16-byte / 4-byte lane choice,
 * the pitches, the alignment or the slab split: every (j, c) is the float32 sum, one add per row in ascending row order from +0,
 * over the rows of cluster j in each block, then one add per block in ascending block order from +0.  Two runs are bit-equal.
 * Error: a two-level sequential sum of depth at most R + B, |sums[j, c] - exact| <= (R + B) 2^-24 sum_i |x[i, c]| over the cluster's
 * rows (first order) -- a tighter bound than one chain over all the cluster's rows has.  NaN / Inf in x[i, c] reach
 * sums[labels[i], c] alone.
 *
 * Alignment: 16-byte lanes when d_x is 16-byte aligned and ldx a multiple of 4 floats, else one float per access; d_x, d_sums 4-byte,
 * d_labels, d_counts 8-byte, d_scratch 16-byte aligned.  Nothing beyond column d of the last row of x is read. */
#ifndef SGL_CLUSTER_SUMS_H
#define SGL_CLUSTER_SUMS_H

#include "sgl_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SGL_CLUSTER_SUMS_MAX_K 1024

/* Host only: the launch decisions of a call with these sizes (and the current "loss_blocks").  out[0] = row blocks B, out[1] = rows
 * per block R (B R >= n > (B - 1) R; both 0 when n = 0 or d = 0: no partial kernel), out[2] = columns per slab, out[3] = slabs S,
 * out[4] = LDS bytes of a workgroup ((k slab + k) x 4).  vec4: 16-byte lanes (1) or one float per access (0): it changes the
 * threads of a workgroup and none of the five. */
int sgl_cluster_sums_rule(int64_t n, int64_t d, int64_t k, int vec4, int64_t *out);

/* bytes of the partial tables: B x S tables of k x slab floats, then B x k int32 counts; -1 for sizes the rule refuses */
int64_t sgl_cluster_sums_scratch(int64_t n, int64_t d, int64_t k);

int sgl_cluster_sums_f32(const float *d_x, int64_t ldx, int64_t n, int64_t d, const int64_t *d_labels, int64_t k, float *d_sums,
                         int64_t lds, int64_t *d_counts, void *d_scratch, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SGL_CLUSTER_SUMS_H */
