// K24: the learnable hop aggregators (LearnableWeightedMessageOp: simple, simple_allow_neg, gate, ori_ref, jk) on STORED hop rows
// (include/sgl_hop_rows.h).  A training step used to gather the B x H x d mini-batch rows into a float32 copy (sgl_gather_hops_*:
// one read, one write; a bfloat16 table is widened on the way) and then read that copy four times -- scores, weighted sum, its
// backward, the column sums of the parameter gradients.  The four kernels here read row idx[i] of every hop table where it is stored.
//
// ROW SOURCE, shared by all of them: up to 16 tables of one element type (float32, or bfloat16 as uint16_t), each with its own
// pointer and pitch, n_rows rows of d <= 512 columns; a device int64 index list of m entries (NULL: row i is row i).  The index of
// an output row is read ONCE, by lane 0 of the row's lane group, made non-negative, range-checked, and the row number is broadcast
// inside the group (from_lane); an index out of range gives the row -1: every lane then loads row 0 and takes NaN instead -- nothing
// traps, no address is formed from the bad index.  Offsets are 64-bit.  The H rows of a node are H independent random lines: all their loads
// (batches of 8 in the streaming kernels) are issued before the first use.
//
// NUMERICS.  A bfloat16 element is widened exactly in registers (bits << 16) from 8-byte loads of 4 elements, so lane l, chunk c owns
// the same four columns as in the float32 row kernels and every reduction runs in the same lane order: kernels 1-3 are BIT-IDENTICAL
// to sgl_gather_hops_* followed by sgl_hop_rowdot2_f32 (u_mask = 0: sgl_hop_rowdot_f32, the plain row-dot and its lane layout) /
// sgl_hop_wsum2d_f32 / sgl_hop_wsum2d_bwd_f32 (same row_instance, dot_chunks, group_sum; the same fma chain in hop order).  The column sums (kernel 4) fold in a fixed order of their own: two runs, same bits.
// No atomics; LDS only for U where there is a reference part (as in hop_rowdot2_reg_kernel) and for the column-sum fold.
#include "sgl_common.h"
#include "sgl_rows.h"
#include "../../include/sgl_hop_rows.h"

namespace {

typedef uint32_t u2 __attribute__((ext_vector_type(2)));
typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));

template <typename T>
struct Tables {
    const T *p[SGL_HOP_ROWS_MAX_HOPS];
    int64_t ld[SGL_HOP_ROWS_MAX_HOPS];
};

// the four columns from c of a stored row as float32, zeros at and beyond column d (the vector that straddles d lies inside the
// row's pitch, a multiple of 4 elements)
__device__ __forceinline__ f4 row_load4(const float *__restrict__ p, const int c, const int d) { return load_masked<4>(p, c, d); }
__device__ __forceinline__ f4 row_load4(const uint16_t *__restrict__ p, const int c, const int d) {
    const u2 r = *reinterpret_cast<const u2 *>(p + c);
    f4 v = (f4){__uint_as_float(r[0] << 16), __uint_as_float(r[0] & 0xffff0000u), __uint_as_float(r[1] << 16),
                __uint_as_float(r[1] & 0xffff0000u)};
    if (c + 4 > d) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (c + e >= d) v[e] = 0.f;
    }
    return v;
}
// chunk at column c of row s of table h; s < 0: the index was out of range -- row 0 is loaded in its place (no branch around the
// load: the loads of a batch stay together) and the d columns are replaced by NaN
template <typename T>
__device__ __forceinline__ f4 source_load4(const Tables<T> hx, const int h, const int64_t s, const int c, const int d) {
    f4 v = row_load4(hx.p[h] + (s < 0 ? 0 : s) * hx.ld[h], c, d);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = (s < 0 && c + e < d) ? __builtin_nanf("") : v[e];
    return v;
}

// The table row of output row i: resolved by lane 0 of the group of LPR lanes, broadcast to the others; -1 = out of range.
template <int LPR>
__device__ __forceinline__ int64_t source_row(const int64_t *__restrict__ idx, const int64_t i, const bool live, const int l,
                                              const int64_t n_rows) {
    int64_t s = -1;
    if (l == 0 && live) {
        s = idx ? idx[i] : i;
        if (s < 0) s += n_rows;
        if (s < 0 || s >= n_rows) s = -1;
    }
    const uint32_t lo = __float_as_uint(from_lane<LPR>(__uint_as_float((uint32_t)(uint64_t)s), 0));
    const uint32_t hi = __float_as_uint(from_lane<LPR>(__uint_as_float((uint32_t)((uint64_t)s >> 32)), 0));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

// ---- 1. scores: hop_rowdot2_reg_kernel (sgl_aggregate.hip) on the row source ----------------------------------------------------
// P[i, h - h0] = <X_h[idx_i], vec> for h in [h0, h1); A[i] = sum over the hops j of u_mask of <X_j[idx_i], U[j]>.  The H rows of a
// node sit in registers, every element is read once.  U is staged in LDS once per block, as there.
template <typename T, int LPR, int CH, int HMAX>
__global__ __launch_bounds__(256) void hop_rows_scores_kernel(const Tables<T> hx, const int n_hops, const int64_t n_rows,
                                                              const int64_t *__restrict__ idx, const float *__restrict__ u,
                                                              const int64_t ldu, const unsigned long long u_mask,
                                                              const float *__restrict__ vec, const int h0, const int h1,
                                                              float *__restrict__ p, const int64_t ldp, float *__restrict__ a,
                                                              const int64_t m, const int d) {
    constexpr int SLOTS = LPR * CH;
    // U lives in dynamic LDS, HMAX x SLOTS vectors, only when there is a reference part: the plain gate scores (u_mask = 0) are
    // launched with no LDS at all and never wait at the barrier
    extern __shared__ f4 us[];
    if (u_mask) {
        for (int i = threadIdx.x; i < HMAX * SLOTS; i += 256) {
            const int h = i / SLOTS, col = (i - h * SLOTS) * 4;
            us[i] = (h < n_hops && ((u_mask >> h) & 1ull) && col < d) ? load_masked<4>(u + (int64_t)h * ldu, col, d) : (f4){0.f, 0.f, 0.f, 0.f};
        }
    }
    const auto [l, r, live] = row_lane<LPR>(m);
    const int64_t s = source_row<LPR>(idx, r, live, l, n_rows);
    f4 x[HMAX][CH], vv[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const int col = (c * LPR + l) * 4;
        const bool on = chunk_on<LPR>(c, l, live, d);
        vv[c] = (col < d) ? load_masked<4>(vec, col, d) : (f4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int h = 0; h < HMAX; ++h) x[h][c] = (on && h < n_hops) ? source_load4(hx, h, s, col, d) : (f4){0.f, 0.f, 0.f, 0.f};
    }
    if (u_mask) __syncthreads();
    float acc[HMAX];
    float shared = 0.f;
#pragma unroll
    for (int h = 0; h < HMAX; ++h) {
        acc[h] = dot_chunks(vv, x[h]);
        if (h < n_hops && ((u_mask >> h) & 1ull)) {
#pragma unroll
            for (int c = 0; c < CH; ++c) shared = dot4(us[h * SLOTS + c * LPR + l], x[h][c], shared);
        }
    }
#pragma unroll
    for (int h = 0; h < HMAX; ++h) acc[h] = group_sum<LPR>(acc[h]);
    shared = group_sum<LPR>(shared);
    if (live && l == 0) {
#pragma unroll
        for (int h = 0; h < HMAX; ++h)
            if (h >= h0 && h < h1) p[r * ldp + (h - h0)] = acc[h];
        if (a) a[r] = shared;
    }
}

// ---- 2. weighted sum: out[i, :] = sum_h W[i ldw + h] X_h[idx_i, :] -------------------------------------------------------------------
// One fma chain from 0 in hop order per element (hop_wsum2d_kernel's).  LPR lanes walk a row 16 bytes each; the row's weights are
// read once; the hop loads of a chunk go out in batches of 8 before the first fma.  Columns [d, dw) are the output's declared
// padding: zeros.  ovec: the output rows are 16-byte vectors.
// (min blocks: left alone, the scheduler spends the whole register file on hoisted loads -- 256 VGPRs, one wave per SIMD)
template <typename T, int LPR>
__global__ __launch_bounds__(256, 3) void hop_rows_wsum_kernel(const Tables<T> hx, const int n_hops, const int64_t n_rows,
                                                            const int64_t *__restrict__ idx, const float *__restrict__ w,
                                                            const int64_t ldw, float *__restrict__ out, const int64_t ldo,
                                                            const int64_t m, const int d, const int dw, const bool ovec) {
    const auto [l, r, live] = row_lane<LPR>(m);
    const int64_t s = source_row<LPR>(idx, r, live, l, n_rows);
    if (!live) return;
    float wv[SGL_HOP_ROWS_MAX_HOPS];
#pragma unroll
    for (int h = 0; h < SGL_HOP_ROWS_MAX_HOPS; ++h) wv[h] = h < n_hops ? w[r * ldw + h] : 0.f;
    float *__restrict__ orow = out + r * ldo;
#pragma unroll 1
    for (int c = l * 4; c < dw; c += LPR * 4) {
        f4 acc = (f4){0.f, 0.f, 0.f, 0.f};
        if (c < d) {
#pragma unroll
            for (int hb = 0; hb < SGL_HOP_ROWS_MAX_HOPS; hb += 8) {
                if (hb < n_hops) {
                    f4 x[8];
#pragma unroll
                    for (int q = 0; q < 8; ++q)
                        if (hb + q < n_hops) x[q] = source_load4(hx, hb + q, s, c, d);
#pragma unroll
                    for (int q = 0; q < 8; ++q)
                        if (hb + q < n_hops) acc = fma4(acc, wv[hb + q], x[q]);
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (c + e >= d) acc[e] = 0.f;        // the pad is zero whatever the weights are (inf x 0)
        }
        if (ovec && c + 4 <= dw) {
            __builtin_nontemporal_store(acc, reinterpret_cast<f4 *>(orow + c));
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (c + e < dw) orow[c + e] = acc[e];
        }
    }
}

// ---- 3. backward of the weighted sum: dW[i, h] = <dOut[i, :], X_h[idx_i, :]> -- hop_rowdot_reg_kernel on the row source -------------
// dOut is autograd's dense [m, d] gradient: dword-aligned 16-byte loads, the partial vector at column d element by element.
template <typename T, int LPR, int CH, int HMAX>
__global__ __launch_bounds__(256) void hop_rows_wsum_bwd_kernel(const Tables<T> hx, const int n_hops, const int64_t n_rows,
                                                                const int64_t *__restrict__ idx, const float *__restrict__ g,
                                                                const int64_t ldg, float *__restrict__ dwt, const int64_t lddw,
                                                                const int64_t m, const int d) {
    const auto [l, r, live] = row_lane<LPR>(m);
    const int64_t s = source_row<LPR>(idx, r, live, l, n_rows);
    f4 gv[CH], xv[HMAX][CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const int col = (c * LPR + l) * 4;
        const bool on = chunk_on<LPR>(c, l, live, d);
        gv[c] = (f4){0.f, 0.f, 0.f, 0.f};
        if (on) {
            const float *gp = g + r * ldg + col;
            if (col + 4 <= d) {
                const f4u t = *reinterpret_cast<const f4u *>(gp);
                gv[c] = (f4){t[0], t[1], t[2], t[3]};
            } else {
#pragma unroll
                for (int e = 0; e < 3; ++e)
                    if (col + e < d) gv[c][e] = gp[e];
            }
        }
#pragma unroll
        for (int h = 0; h < HMAX; ++h) xv[h][c] = (on && h < n_hops) ? source_load4(hx, h, s, col, d) : (f4){0.f, 0.f, 0.f, 0.f};
    }
    float acc[HMAX];
#pragma unroll
    for (int h = 0; h < HMAX; ++h) acc[h] = dot_chunks(gv, xv[h]);
#pragma unroll
    for (int h = 0; h < HMAX; ++h) acc[h] = group_sum<LPR>(acc[h]);
    if (live && l == 0) {
#pragma unroll
        for (int h = 0; h < HMAX; ++h)
            if (h < n_hops) dwt[r * lddw + h] = acc[h];
    }
}

// ---- 4. column sums: out[h, :] = sum_i w[i ldw + h sw] X_h[idx_i, :] ----------------------------------------------------------------
// Level one: a block takes per_block consecutive output rows, its 256 / LPR lane groups one row each per step; a lane keeps its CH
// chunks of up to 8 hops in registers (acc[HMAX][CH]; tables h_off .. h_off + n_hops - 1 of n_total: with 12 or 16 hop accumulators
// every instance went to scratch, so more than 8 hops take two launches over the index list) and issues the hop loads of a row in
// batches of 8 / CH hops before it uses them.
// Then the groups are folded through LDS in group order and the block's partial table goes to the scratch.  Level two: one
// wavefront per (hop, 16-byte column slot) adds the blocks' partials, lane l the blocks l, l + 64, ... in that order, then a fixed
// butterfly.  Both orders depend on (m, d) only.
#define COLSUM_ROWS_MIN_BLOCKS(HMAX, CH) (((HMAX) * (CH) <= 8) ? 4 : 2)   // the scheduler left alone: 256 VGPRs in every instance
template <typename T, int LPR, int CH, int HMAX>
__global__ __launch_bounds__(256, COLSUM_ROWS_MIN_BLOCKS(HMAX, CH)) void hop_rows_colsum_partial_kernel(const Tables<T> hx, const int n_hops, const int64_t n_rows,
                                                                      const int64_t *__restrict__ idx, const float *__restrict__ w,
                                                                      const int64_t ldw, const int sw, const int h_off,
                                                                      const int n_total, float *__restrict__ scratch,
                                                                      const int64_t m, const int d, const int64_t per_block) {
    constexpr int RPB = 256 / LPR, HB = (8 / CH < HMAX) ? 8 / CH : HMAX;   // hops per batch of loads: divides HMAX
    __shared__ f4 red[256];
    const int t = threadIdx.x, l = t % LPR, g = t / LPR;
    const int64_t r0 = (int64_t)blockIdx.x * per_block, r1 = min(r0 + per_block, m);
    f4 acc[HMAX][CH];
#pragma unroll
    for (int h = 0; h < HMAX; ++h)
#pragma unroll
        for (int c = 0; c < CH; ++c) acc[h][c] = (f4){0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int64_t rb = r0; rb < r1; rb += RPB) {          // the same trip count for every lane of the block
        const bool live = rb + g < r1;
        const int64_t r = live ? rb + g : r0;
        const int64_t s = source_row<LPR>(idx, r, live, l, n_rows);
#pragma unroll
        for (int hb = 0; hb < HMAX; hb += HB) {
            f4 x[HB][CH];
            float wv[HB];
#pragma unroll
            for (int q = 0; q < HB; ++q)
                if (hb + q < n_hops) {
                    wv[q] = live ? w[r * ldw + (int64_t)(h_off + hb + q) * sw] : 0.f;
#pragma unroll
                    for (int c = 0; c < CH; ++c) {
                        const int col = (c * LPR + l) * 4;
                        x[q][c] = (live && col < d) ? source_load4(hx, hb + q, s, col, d) : (f4){0.f, 0.f, 0.f, 0.f};
                    }
                }
#pragma unroll
            for (int q = 0; q < HB; ++q)
                if (hb + q < n_hops && live) {
#pragma unroll
                    for (int c = 0; c < CH; ++c) acc[hb + q][c] = fma4(acc[hb + q][c], wv[q], x[q][c]);
                }
        }
    }
    constexpr int DP = LPR * CH * 4;                     // floats of one partial row
#pragma unroll
    for (int h = 0; h < HMAX; ++h) {
        if (h < n_hops) {
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                red[t] = acc[h][c];
                __syncthreads();
                if (g == 0) {
                    f4 sum = red[l];
                    for (int q = 1; q < RPB; ++q) {
                        const f4 o = red[q * LPR + l];
#pragma unroll
                        for (int e = 0; e < 4; ++e) sum[e] += o[e];
                    }
                    *reinterpret_cast<f4 *>(scratch + ((int64_t)blockIdx.x * n_total + h_off + h) * DP + (c * LPR + l) * 4) = sum;
                }
                __syncthreads();
            }
        }
    }
}

__global__ __launch_bounds__(64) void hop_rows_colsum_final_kernel(const float *__restrict__ scratch, const int n_blocks, const int n_hops,
                                                                   const int slots, const int dp, float *__restrict__ out,
                                                                   const int64_t ldo, const int d) {
    const int h = blockIdx.x / slots, slot = blockIdx.x - h * slots;
    f4 s = (f4){0.f, 0.f, 0.f, 0.f};
    for (int b = threadIdx.x; b < n_blocks; b += 64) {
        const f4 o = *reinterpret_cast<const f4 *>(scratch + ((int64_t)b * n_hops + h) * dp + slot * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) s[e] += o[e];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) s[e] = group_sum<64>(s[e]);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (slot * 4 + e < d) out[(int64_t)h * ldo + slot * 4 + e] = s[e];
    }
}

// ---- host: the row source's checks, once for the eight entry points ---------------------------------------------------------------
template <typename T>
int fill_source(const char *who, Tables<T> &hx, int n_hops, const T *const *h_x, const int64_t *h_ldx, int64_t n_rows,
                const int64_t *d_idx, int64_t m, int64_t d) {
    constexpr int kAlign = sizeof(T) == 4 ? 16 : 8;
    if (n_hops < 1) return sgl::fail(SGL_ERR_INVALID, "%s: n_hops=%d: at least one table is needed", who, n_hops);
    if (n_hops > SGL_HOP_ROWS_MAX_HOPS)
        return sgl::fail(SGL_ERR_UNSUPPORTED, "%s: n_hops=%d: at most %d tables", who, n_hops, SGL_HOP_ROWS_MAX_HOPS);
    if (!h_x) return sgl::fail(SGL_ERR_INVALID, "%s: NULL table pointer array", who);
    if (n_rows < 0 || m < 0 || d < 1) return sgl::fail(SGL_ERR_INVALID, "%s: bad sizes (n_rows, m >= 0 and d >= 1)", who);
    if (d > SGL_HOP_ROWS_MAX_D) return sgl::fail(SGL_ERR_UNSUPPORTED, "%s: d=%lld: rows of at most %d columns", who, (long long)d, SGL_HOP_ROWS_MAX_D);
    if (!d_idx && m != n_rows) return sgl::fail(SGL_ERR_INVALID, "%s: without an index list m must equal n_rows", who);
    if (m > 0 && n_rows == 0) return sgl::fail(SGL_ERR_INVALID, "%s: a table without rows", who);
    for (int h = 0; h < SGL_HOP_ROWS_MAX_HOPS; ++h) {
        hx.p[h] = h < n_hops ? h_x[h] : nullptr;
        hx.ld[h] = h < n_hops ? (h_ldx ? h_ldx[h] : (d + 3) / 4 * 4) : 0;
        if (h >= n_hops) continue;
        if (!hx.p[h]) return sgl::fail(SGL_ERR_INVALID, "%s: table %d: NULL pointer", who, h);
        if (hx.ld[h] < d) return sgl::fail(SGL_ERR_INVALID, "%s: table %d: pitch %lld < d", who, h, (long long)hx.ld[h]);
        if (hx.ld[h] % 4 != 0 || !aligned_to(hx.p[h], kAlign))
            return sgl::fail(SGL_ERR_UNSUPPORTED, "%s: table %d: rows must be %d-byte aligned on a pitch that is a multiple of 4 elements", who,
                             h, kAlign);
    }
    return SGL_OK;
}

template <typename T>
int scores_impl(const char *who, int n_hops, const T *const *h_x, const int64_t *h_ldx, int64_t n_rows, const int64_t *d_idx, int64_t m,
                const float *d_u, int64_t ldu, uint64_t u_mask, const float *d_vec, int h0, int h1, float *d_p, int64_t ldp, float *d_a,
                int64_t d, void *stream) {
    Tables<T> hx;
    const int rc = fill_source(who, hx, n_hops, h_x, h_ldx, n_rows, d_idx, m, d);
    if (rc != SGL_OK) return rc;
    SGL_REQUIRE(h0 >= 0 && h0 <= h1 && h1 <= n_hops, "%s: bad hop range", who);
    SGL_REQUIRE((u_mask >> n_hops) == 0, "%s: u_mask names a hop beyond n_hops", who);
    if (m == 0) return SGL_OK;
    SGL_REQUIRE(d_vec && (h1 == h0 || (d_p && ldp >= h1 - h0)), "%s: bad arguments", who);
    SGL_REQUIRE(u_mask == 0 || (d_u && d_a && ldu >= d), "%s: the reference part needs U [n_hops, ldu] and A [m]", who);
    if (!aligned_to(d_vec, 16) || (u_mask && (!aligned_to(d_u, 16) || ldu % 4 != 0)))
        return sgl::fail(SGL_ERR_UNSUPPORTED, "%s: vec and U must be 16-byte aligned, zero-padded to whole vectors", who);
    hipStream_t st = sgl::as_stream(stream);
    float *a_out = u_mask ? d_a : nullptr;
    // the 8 x 5 layout belongs to the reference part (sgl_core.cpp: it pays in the jk-score kernel alone); without one this is the plain
    // row-dot, in the layout and lane order of hop_rowdot_reg_kernel and of the one-pass gate kernel
    return launch_row_instance<true>({who, who, who}, sgl::row_instance(d, n_hops, u_mask != 0), n_hops, m, [&](dim3 grid, auto L, auto C, auto HM) {
        hipLaunchKernelGGL((hop_rows_scores_kernel<T, L, C, HM>), grid, dim3(256), u_mask ? (size_t)HM * L * C * sizeof(f4) : 0, st, hx, n_hops, n_rows, d_idx, d_u, ldu,
                           (unsigned long long)u_mask, d_vec, h0, h1, d_p, ldp, a_out, m, (int)d);
    });
}

template <typename T>
int wsum_impl(const char *who, int n_hops, const T *const *h_x, const int64_t *h_ldx, int64_t n_rows, const int64_t *d_idx, int64_t m,
              const float *d_w, int64_t ldw, float *d_out, int64_t ldo, int64_t pad_cols, int64_t d, void *stream) {
    Tables<T> hx;
    int rc = fill_source(who, hx, n_hops, h_x, h_ldx, n_rows, d_idx, m, d);
    if (rc != SGL_OK) return rc;
    if (m == 0) return SGL_OK;
    SGL_REQUIRE(d_w && (ldw == 0 || ldw >= n_hops), "%s: bad weights (ldw = 0: one vector for every row, else ldw >= n_hops)", who);
    SGL_REQUIRE(d_out && ldo >= d, "%s: bad output", who);
    rc = sgl::check_pad(who, d, pad_cols, ldo);
    if (rc != SGL_OK) return rc;
    const int dw = (int)(d + pad_cols);
    const bool ovec = ldo % 4 == 0 && aligned_to(d_out, 16);
    const int lpr = sgl::pick_lpr(dw, 4);
    const int64_t blocks = (m + (256 / lpr) - 1) / (256 / lpr);
    if (!sgl::launch_fits(blocks, 256)) return sgl::fail(SGL_ERR_UNSUPPORTED, "%s: too many rows for one launch", who);
    hipStream_t st = sgl::as_stream(stream);
    with_lpr(lpr, [&](auto L) {
        hipLaunchKernelGGL((hop_rows_wsum_kernel<T, L>), dim3((unsigned)blocks), dim3(256), 0, st, hx, n_hops, n_rows, d_idx, d_w, ldw, d_out,
                           ldo, m, (int)d, dw, ovec);
    });
    return launch_check(who);
}

template <typename T>
int wsum_bwd_impl(const char *who, int n_hops, const T *const *h_x, const int64_t *h_ldx, int64_t n_rows, const int64_t *d_idx, int64_t m,
                  const float *d_dout, int64_t lddo, float *d_dw, int64_t lddw, int64_t d, void *stream) {
    Tables<T> hx;
    const int rc = fill_source(who, hx, n_hops, h_x, h_ldx, n_rows, d_idx, m, d);
    if (rc != SGL_OK) return rc;
    if (m == 0) return SGL_OK;
    SGL_REQUIRE(d_dout && lddo >= d && aligned_to(d_dout, 4), "%s: bad dOut", who);
    SGL_REQUIRE(d_dw && lddw >= n_hops, "%s: bad dW", who);
    hipStream_t st = sgl::as_stream(stream);
    return launch_row_instance({who, who, who}, sgl::row_instance(d, n_hops), n_hops, m, [&](dim3 grid, auto L, auto C, auto HM) {
        hipLaunchKernelGGL((hop_rows_wsum_bwd_kernel<T, L, C, HM>), grid, dim3(256), 0, st, hx, n_hops, n_rows, d_idx, d_dout, lddo, d_dw,
                           lddw, m, (int)d);
    });
}

// level one of the column sums: lanes per row x chunks, rows per block, blocks -- functions of (m, d) alone
struct ColsumShape {
    int lpr, ch;
    int64_t per_block, blocks;
};
constexpr int kColsumBlocks = 1024;
ColsumShape colsum_shape(int64_t m, int64_t d) {
    ColsumShape s;
    s.lpr = sgl::pick_lpr(d, 4);
    s.ch = d > (int64_t)s.lpr * 4 ? 2 : 1;
    const int64_t rpb = 256 / s.lpr;
    int64_t per = std::max<int64_t>((m + kColsumBlocks - 1) / kColsumBlocks, rpb * 4);
    s.per_block = (per + rpb - 1) / rpb * rpb;
    s.blocks = std::max<int64_t>(1, (m + s.per_block - 1) / s.per_block);
    return s;
}

template <typename T>
int colsum_impl(const char *who, int n_hops, const T *const *h_x, const int64_t *h_ldx, int64_t n_rows, const int64_t *d_idx, int64_t m,
                const float *d_w, int64_t ldw, int sw, float *d_out, int64_t ldo, float *d_scratch, int64_t d, void *stream) {
    Tables<T> hx;
    const int rc = fill_source(who, hx, n_hops, h_x, h_ldx, n_rows, d_idx, m, d);
    if (rc != SGL_OK) return rc;
    SGL_REQUIRE(sw == 0 || sw == 1, "%s: sw must be 0 (one weight per row) or 1 (one per row and hop)", who);
    if (m == 0) return SGL_OK;
    SGL_REQUIRE(d_w && ldw >= (sw ? n_hops : 1), "%s: bad weights", who);
    SGL_REQUIRE(d_out && ldo >= d, "%s: bad output", who);
    SGL_REQUIRE(d_scratch && aligned_to(d_scratch, 16), "%s: NULL or misaligned scratch (sgl_hop_rows_colsum_scratch floats)", who);
    const ColsumShape cs = colsum_shape(m, d);
    hipStream_t st = sgl::as_stream(stream);
    for (int h_off = 0; h_off < n_hops; h_off += 8) {
        const int nh = std::min(8, n_hops - h_off);
        Tables<T> part;
        for (int h = 0; h < SGL_HOP_ROWS_MAX_HOPS; ++h) {
            part.p[h] = h < nh ? hx.p[h_off + h] : nullptr;
            part.ld[h] = h < nh ? hx.ld[h_off + h] : 0;
        }
        const bool launched = with_lpr(cs.lpr, [&](auto L) {
            with_one_of<1, 2>(cs.ch, [&](auto C) {
                if constexpr (decltype(C)::value == 1 || decltype(L)::value == 64) {
                    with_one_of<4, 8>(nh <= 4 ? 4 : 8, [&](auto HM) {
                        hipLaunchKernelGGL((hop_rows_colsum_partial_kernel<T, L, C, HM>), dim3((unsigned)cs.blocks), dim3(256), 0, st, part, nh,
                                           n_rows, d_idx, d_w, ldw, sw, h_off, n_hops, d_scratch, m, (int)d, cs.per_block);
                    });
                }
            });
        });
        if (!launched) return no_row_instance(who, cs.lpr, cs.ch, n_hops);
        SGL_LAUNCH_CHECK(who);
    }
    const int slots = (int)((d + 3) / 4);
    hipLaunchKernelGGL(hop_rows_colsum_final_kernel, dim3(n_hops * slots), dim3(64), 0, st, d_scratch, (int)cs.blocks, n_hops, slots,
                       cs.lpr * cs.ch * 4, d_out, ldo, (int)d);
    return launch_check(who);
}

}  // namespace

SGL_EXPORT int sgl_hop_rows_scores_f32(int n_hops, const float *const *h_x, const int64_t *h_ldx, int64_t n_rows, const int64_t *d_idx,
                                       int64_t m, const float *d_u, int64_t ldu, uint64_t u_mask, const float *d_vec, int h0, int h1,
                                       float *d_p, int64_t ldp, float *d_a, int64_t d, void *stream) {
    return scores_impl("sgl_hop_rows_scores_f32", n_hops, h_x, h_ldx, n_rows, d_idx, m, d_u, ldu, u_mask, d_vec, h0, h1, d_p, ldp, d_a, d, stream);
}
SGL_EXPORT int sgl_hop_rows_scores_bf16(int n_hops, const uint16_t *const *h_x, const int64_t *h_ldx, int64_t n_rows, const int64_t *d_idx,
                                        int64_t m, const float *d_u, int64_t ldu, uint64_t u_mask, const float *d_vec, int h0, int h1,
                                        float *d_p, int64_t ldp, float *d_a, int64_t d, void *stream) {
    return scores_impl("sgl_hop_rows_scores_bf16", n_hops, h_x, h_ldx, n_rows, d_idx, m, d_u, ldu, u_mask, d_vec, h0, h1, d_p, ldp, d_a, d, stream);
}

SGL_EXPORT int sgl_hop_rows_wsum_f32(int n_hops, const float *const *h_x, const int64_t *h_ldx, int64_t n_rows, const int64_t *d_idx,
                                     int64_t m, const float *d_w, int64_t ldw, float *d_out, int64_t ldo, int64_t pad_cols, int64_t d,
                                     void *stream) {
    return wsum_impl("sgl_hop_rows_wsum_f32", n_hops, h_x, h_ldx, n_rows, d_idx, m, d_w, ldw, d_out, ldo, pad_cols, d, stream);
}
SGL_EXPORT int sgl_hop_rows_wsum_bf16(int n_hops, const uint16_t *const *h_x, const int64_t *h_ldx, int64_t n_rows, const int64_t *d_idx,
                                      int64_t m, const float *d_w, int64_t ldw, float *d_out, int64_t ldo, int64_t pad_cols, int64_t d,
                                      void *stream) {
    return wsum_impl("sgl_hop_rows_wsum_bf16", n_hops, h_x, h_ldx, n_rows, d_idx, m, d_w, ldw, d_out, ldo, pad_cols, d, stream);
}

SGL_EXPORT int sgl_hop_rows_wsum_bwd_f32(int n_hops, const float *const *h_x, const int64_t *h_ldx, int64_t n_rows, const int64_t *d_idx,
                                         int64_t m, const float *d_dout, int64_t lddo, float *d_dw, int64_t lddw, int64_t d, void *stream) {
    return wsum_bwd_impl("sgl_hop_rows_wsum_bwd_f32", n_hops, h_x, h_ldx, n_rows, d_idx, m, d_dout, lddo, d_dw, lddw, d, stream);
}
SGL_EXPORT int sgl_hop_rows_wsum_bwd_bf16(int n_hops, const uint16_t *const *h_x, const int64_t *h_ldx, int64_t n_rows, const int64_t *d_idx,
                                          int64_t m, const float *d_dout, int64_t lddo, float *d_dw, int64_t lddw, int64_t d, void *stream) {
    return wsum_bwd_impl("sgl_hop_rows_wsum_bwd_bf16", n_hops, h_x, h_ldx, n_rows, d_idx, m, d_dout, lddo, d_dw, lddw, d, stream);
}

SGL_EXPORT int64_t sgl_hop_rows_colsum_scratch(int n_hops, int64_t m, int64_t d) {
    if (n_hops < 1 || n_hops > SGL_HOP_ROWS_MAX_HOPS || m < 0 || d < 1 || d > SGL_HOP_ROWS_MAX_D) return 0;
    const ColsumShape cs = colsum_shape(m, d);
    return cs.blocks * n_hops * cs.lpr * cs.ch * 4;
}
SGL_EXPORT int sgl_hop_rows_colsum_f32(int n_hops, const float *const *h_x, const int64_t *h_ldx, int64_t n_rows, const int64_t *d_idx,
                                       int64_t m, const float *d_w, int64_t ldw, int sw, float *d_out, int64_t ldo, float *d_scratch,
                                       int64_t d, void *stream) {
    return colsum_impl("sgl_hop_rows_colsum_f32", n_hops, h_x, h_ldx, n_rows, d_idx, m, d_w, ldw, sw, d_out, ldo, d_scratch, d, stream);
}
SGL_EXPORT int sgl_hop_rows_colsum_bf16(int n_hops, const uint16_t *const *h_x, const int64_t *h_ldx, int64_t n_rows, const int64_t *d_idx,
                                        int64_t m, const float *d_w, int64_t ldw, int sw, float *d_out, int64_t ldo, float *d_scratch,
                                        int64_t d, void *stream) {
    return colsum_impl("sgl_hop_rows_colsum_bf16", n_hops, h_x, h_ldx, n_rows, d_idx, m, d_w, ldw, sw, d_out, ldo, d_scratch, d, stream);
}
