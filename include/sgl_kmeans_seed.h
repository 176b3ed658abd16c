/* sgl_kmeans_seed.h -- K20: greedy k-means++ seeding on the device, part of libsgl_hip.so.  Opt-in: kmeans(init="greedy-k-means++");
 * init="k-means++", the torch seeding, stays the default and keeps its bits.
 *
 * Step j = 0 .. k - 1 tries L_j candidate rows (L_0 = 1, L_j = trials after it) against near_{j-1}[i], the squared distance of row i
 * to the nearest centre chosen so far (+inf before step 0):
 *
 *   D_l[i]       = sum_c (x[i, c] - x[cand_l, c])^2                  the direct form, bit-equal to what sgl_kmeans_assign_f32 returns
 *                                                                    in its 16-byte-lane form against the one centre x[cand_l]
 *   trial_l[i]   = min(near_{j-1}[i], D_l[i])                        NaN where either is NaN
 *   pot_l        = the float64 sum over i of the FINITE trial_l[i]   (a NaN or infinite entry is stored as computed and adds nothing)
 *   best         = the l of the lowest pot_l, the lowest l on a tie
 *   centre_ids[j] = cand[best],  pot[j] = pot_best,  near_j = trial_best
 *
 * and draws the candidates of step j + 1 from draws[j + 1, 0 .. trials): with t = u * pot_best (one float64 multiply), the first row
 * whose cumulative float64 sum of near_j, in ascending row order and over finite entries alone, is GREATER than t -- searchsorted's
 * right=True: a row at distance zero is never drawn.  No such row (every distance zero, u * pot rounding up to pot): row n - 1.  The
 * first centre is row min(floor(draws[0, 0] * n), n - 1).  trials = 1 is plain k-means++; sklearn's greedy seeding is trials = 2 +
 * floor(ln k).
 *
 * TWO LAUNCHES PER STEP on `stream`, 2 k for a seeding; no host read, no allocation, no atomics; the host learns nothing before the end.
 * (1) seed_step, B row blocks, one pass over X: the L candidate rows are staged in LDS (negated, padded to whole vectors), LPR lanes own
 * a row of x in registers as in K9 and take the candidates from LDS, so L candidates cost one read of X.  The block writes
 * trial[l][i] (L n floats: 5 % of X at L = 5, d = 100), reads its own R x L entries back and writes their float64 sum P[b][l]: thread
 * t of 256 adds the entries t, t + 256, ... of the block in ascending order, then the 256 sums are halved eight times (t += t + 128,
 * t += t + 64, ...): an order that depends on the block's row count alone.  near_{j-1} is row best_{j-1} of the PREVIOUS trial table,
 * selected by reading that index on the device: nothing is committed by a copy, two tables take turns.
 * (2) seed_pick, one workgroup: pot_l = sum_b P[b][l] in ascending b; best; the outputs of the step; then for every draw the first
 * block whose inclusive prefix of P[.][best] (ascending b) exceeds t and, inside it, the running sum over trial[best] that starts at
 * the prefix of the blocks before.  P[b] and the running sum over block b round differently: when no row of that block exceeds t the
 * block's last row is taken.  The pick of step k - 1 is launched with further workgroups, which each find `best` again the same way
 * and copy their part of trial[best] to near.
 *
 * BLOCKS.  R = max(256, ceil(n / 2048)) rows, B = ceil(n / R) <= 2048: functions of n alone.  The staging of a block re-reads L
 * rows for R rows of X (3 % at L = 8, R = 256).  The tuning key "loss_blocks" (sgl_set_tuning), when > 0, REPLACES that choice as in
 * K19: B = ceil(n / ceil(n / min(loss_blocks, n, 2048))).
 *
 * LDS BUDGET AND THE COLUMN-CHUNK RULE.  A workgroup gets 64 KiB (16 384 words, what a launch gets without asking).  With dp = d
 * rounded up to 4, the L rows are staged whole while L dp <= 16 384: every width of the register layouts (d <= 2048) at every L <= 8.
 * Wider rows are streamed, one row per wavefront as in K9's streaming kernel, and the candidates are staged in column chunks of
 * W = floor(16384 / L / 256) x 256 columns (2048 at L = 8, 16 384 at L = 1) whenever L dp is beyond the budget; the L partial sums
 * of a row stay in registers across the chunks, so every width up to SGL_MAX_WIDTH is served.  The float64 block sums reuse the tile:
 * the launch asks for max(4 L W, 2048 L) bytes.
 *
 * ORDER GUARANTEE.  The bits of the three outputs depend on (the values of x, n, d, k, trials, B, the draws) -- not on the pitch, the
 * alignment, the 16-byte / 4-byte lane choice or the column chunks: a distance is always summed in the order of K9's 16-byte-lane
 * form (lane l of LPR holds the vectors l, l + LPR, ...; elements 0 and 2 in one fma chain, 1 and 3 in the other; the lane sums of
 * sgl_kmeans.hip), 4-byte lanes read the same four columns one by one.  Two runs are bit-equal.
 *
 * Alignment: 16-byte lanes when d_x is 16-byte aligned and ldx a multiple of 4 floats, else one float per access; d_x, d_near 4-byte,
 * d_draws, d_centre_ids, d_pot 8-byte, d_scratch 16-byte aligned.  Nothing beyond column d of the last row of x is read.
 *
 * Refused: trials outside [1, SGL_KMEANS_SEED_MAX_TRIALS] (SGL_ERR_UNSUPPORTED), k < 1 or n < k (SGL_ERR_INVALID); sgl_last_error
 * has the text.  Draws are taken as they are (uniform in [0, 1) by contract); every row id formed from them is clamped to [0, n). */
#ifndef SGL_KMEANS_SEED_H
#define SGL_KMEANS_SEED_H

#include "sgl_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SGL_KMEANS_SEED_MAX_TRIALS 8 /* 2 + floor(ln k) for every k up to 1 096 */

/* Host only: the launch decisions of a seeding with these sizes (and the current "loss_blocks").  out[0] = row blocks B, out[1] =
 * rows per block R (B R >= n > (B - 1) R), out[2] = columns per chunk W of the staged candidates (dp when they are staged whole),
 * out[3] = chunks ceil(dp / W), out[4] = LDS bytes of a seed_step workgroup. */
int sgl_kmeans_seed_rule(int64_t n, int64_t d, int trials, int64_t *out);

/* bytes of the scratch: P (2048 x 8 float64), cand (8 int64), best (16 bytes), then the two trial tables of trials x n floats, each
 * rounded up to 16 bytes -- a function of (n, trials) alone; -1 for sizes the rule refuses */
int64_t sgl_kmeans_seed_scratch(int64_t n, int trials);

/* d_draws: float64 [k, trials], row-major; d_centre_ids: int64 [k]; d_near: float32 [n]; d_pot: float64 [k] */
int sgl_kmeans_seed_f32(const float *d_x, int64_t ldx, int64_t n, int64_t d, int64_t k, int trials, const double *d_draws,
                        int64_t *d_centre_ids, float *d_near, double *d_pot, void *d_scratch, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SGL_KMEANS_SEED_H */
