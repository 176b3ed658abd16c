// Device and host pieces that the linear-head kernels share, each written once: sgl_linear_head.hip (K21 / K22: the class kernel and the
// two-launch weight gradient) and sgl_linear_step.hip (K23: the one-pass training step).  The row source <T, ROWS> (load4, widen,
// source_row), the staging of W in LDS, one step group of a logit's chain (logit_group: the ORDER of include/sgl_linear_head.h), K14's
// row work in the accumulator layout (class_epilogue, dz_value), the block rule of the weight gradient and its ordered fold.
#ifndef SGL_LINEAR_COMMON_H
#define SGL_LINEAR_COMMON_H

#include <climits>
#include <cmath>

#include "sgl_rows.h"   // f4, edge_load, store_cols, with_vec, with_chunks, SGL_LAUNCH_CHECK

#include "../../include/sgl_linear_head.h"

namespace {

using f16v = float __attribute__((ext_vector_type(16)));

constexpr int kMaxBlocks = 2048;                     // K9's cap: 256 CUs x 8 resident workgroups, the batches beyond are strided over
constexpr int kPitchPad = 4;                         // floats: makes pitch / 4 odd
constexpr int kNoIndex = INT32_MAX;                  // "no candidate" of the index minimum

// columns col .. col + 3 of a row, zeros from column d on; col < d.  VEC = 1: the four elements one by one
template <int VEC>
__device__ __forceinline__ f4 load4(const float *__restrict__ p, const int col, const int d, const bool last_row) {
    if constexpr (VEC == 4) {
        return edge_load<4>(p, col, d, last_row);
    } else {
        f4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (col + e < d) ? p[col + e] : 0.f;
        return v;
    }
}

// the same of a bfloat16 row, widened exactly.  VEC = 4: one 8-byte access where it stays inside the row's d columns or (not the table's
// last row) inside its pitch
__device__ __forceinline__ float widen(const uint16_t v) { return __uint_as_float((uint32_t)v << 16); }
template <int VEC>
__device__ __forceinline__ f4 load4(const uint16_t *__restrict__ p, const int col, const int d, const bool last_row) {
    f4 v;
    if (VEC == 4 && (col + 4 <= d || !last_row)) {
        const uint2 u = *reinterpret_cast<const uint2 *>(p + col);
        v = f4{__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16), __uint_as_float(u.y & 0xffff0000u)};
#pragma unroll
        for (int e = 1; e < 4; ++e)
            if (col + e >= d) v[e] = 0.f;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (col + e < d) ? widen(p[col + e]) : 0.f;
    }
    return v;
}
__device__ __forceinline__ float widen(const float v) { return v; }

// ROWS: the table row a batch row reads -- idx[row] (NULL: row itself), negative ones count from the end; `bad`: outside [-n_rows, n_rows),
// the row then reads as NaN and row 0 stands in for its address
__device__ __forceinline__ int64_t source_row(const int64_t *__restrict__ idx, const int64_t row, const int64_t n_rows, bool &bad) {
    int64_t s = idx ? idx[row] : row;
    if (s < 0) s += n_rows;
    bad = s < 0 || s >= n_rows;
    return bad ? 0 : s;
}

// a row of NaN in its d columns (a bad index): every logit of the row is NaN, nothing traps
__device__ __forceinline__ f4 nan_cols(const int col, const int d) {
    f4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = (col + e < d) ? __uint_as_float(0x7fc00000u) : 0.f;
    return v;
}

// columns c0 .. c0 + wc - 1 of the c rows of W into the tile, zeros from column d on: one wavefront per row
template <int VEC>
__device__ __forceinline__ void stage_weights(float *__restrict__ tile, const float *__restrict__ wt, const int64_t ldw, const int c,
                                              const int d, const int c0, const int wc, const int p) {
    const int lane = threadIdx.x % 64;
    for (int j = threadIdx.x / 64; j < c; j += 4) {
        const float *wrow = wt + (int64_t)j * ldw;
        for (int lc = lane * 4; lc < wc; lc += 256) {
            const int col = c0 + lc;
            f4 v = {0.f, 0.f, 0.f, 0.f};
            if (col < d) v = load4<VEC>(wrow, col, d, j == c - 1);
            *reinterpret_cast<f4 *>(tile + j * p + lc) = v;
        }
    }
}

__device__ __forceinline__ int imin(const int a, const int b) { return a < b ? a : b; }
// the two halves' values of a lane pair: [0] is half 0's in both lanes, [1] half 1's
__device__ __forceinline__ auto halves(const unsigned v) { return __builtin_amdgcn_permlane32_swap(v, v, false, false); }
__device__ __forceinline__ float halves_sum(const float v) {
    const auto r = halves(__float_as_uint(v));
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
__device__ __forceinline__ int halves_min(const int v) {
    const auto r = halves((unsigned)v);
    return imin((int)r[0], (int)r[1]);
}

// THE CHAIN: one group of 8 columns of every logit of R row tiles.  Lane (i, h) holds xv[r] = columns 8 q + 4 h .. + 3 of its row of
// tile r; lc = that group's first column in the staged tile + 4 h.  Element e is one MFMA step: acc += W[j, 8 q + e] x[., 8 q + e] +
// W[j, 8 q + 4 + e] x[., 8 q + 4 + e]; class slots >= c take zeros
template <int NT, int R>
__device__ __forceinline__ void logit_group(f16v (&acc)[R][NT], const float *__restrict__ tile, const int p, const int c, const int i,
                                            const int lc, const f4 (&xv)[R]) {
#pragma unroll
    for (int ct = 0; ct < NT; ++ct) {
        const int j = ct * 32 + i;
        f4 a = *reinterpret_cast<const f4 *>(tile + (j < c ? j : c - 1) * p + lc);
        if (j >= c) a = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int r = 0; r < R; ++r) acc[r][ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], xv[r][e], acc[r][ct], 0, 0, 0);
    }
}

// THE EPILOGUE, in the accumulator layout: lane (i, h) holds the logits 32 t + 8 g + 4 h + e of row i without their bias, bs the bias
// (zeros from class c on).  Writes z, pred and row_loss (each optional) of a row that is `in`; with want_exp the accumulators leave as
// exp(z - max) (0 in the slots >= c) and the state says what dz_value needs
struct RowState {
    float s;                                         // the sum of the row's exponentials
    int y;                                           // the label of a live row, else -1
    bool live;
};
template <int NT>
__device__ __forceinline__ RowState class_epilogue(f16v (&acc)[NT], const float *__restrict__ bs, const int c, const int h, const bool in,
                                                   const int64_t row, const int64_t *__restrict__ labels, const bool want_exp,
                                                   float *__restrict__ row_loss, int64_t *__restrict__ pred, float *__restrict__ z,
                                                   const int64_t ldz, const bool z_vec) {
    // this lane's logits in ascending class order: the bias, the logits out, K14's candidates
    float top = -INFINITY;
    int at = kNoIndex, nan_at = kNoIndex;
#pragma unroll
    for (int ct = 0; ct < NT; ++ct)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int j0 = ct * 32 + 8 * g + 4 * h;
            const f4 bb = *reinterpret_cast<const f4 *>(bs + j0);
            f4 run;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float v = acc[ct][4 * g + e] + bb[e];
                acc[ct][4 * g + e] = run[e] = v;
                if (j0 + e < c) {
                    if (v != v) {
                        if (nan_at == kNoIndex) nan_at = j0 + e;
                    } else if (at == kNoIndex || v > top) {
                        top = v;
                        at = j0 + e;
                    }
                }
            }
            if (z && in && j0 < c) store_cols<4>(z + row * ldz, j0, c, run, z_vec);
        }
    const auto tt = halves(__float_as_uint(top));
    const float m = fmaxf(__uint_as_float(tt[0]), __uint_as_float(tt[1]));   // of the entries that are not NaN
    if (pred) {
        const int first_nan = halves_min(nan_at);
        const int first_top = halves_min((at != kNoIndex && top == m) ? at : kNoIndex);
        if (in && h == 0) pred[row] = first_nan != kNoIndex ? first_nan : first_top;
    }
    RowState st = {1.f, -1, false};
    if (!want_exp) return st;                        // (uniform: the same for every lane of the launch)
    const int64_t label = in ? labels[row] : -1;
    st.live = label >= 0 && label < c;
    st.y = st.live ? (int)label : -1;
    float part = 0.f, zy = 0.f;
#pragma unroll
    for (int ct = 0; ct < NT; ++ct)
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int j = ct * 32 + 8 * (v / 4) + 4 * h + v % 4;
            const float lz = acc[ct][v];
            const float ex = j < c ? expf(lz - m) : 0.f;
            zy = j == st.y ? lz : zy;
            acc[ct][v] = ex;
            part += ex;
        }
    st.s = halves_sum(part);
    zy = halves_sum(zy);                             // the other half holds 0: exact
    if (in && row_loss && h == 0) row_loss[row] = st.live ? (m + logf(st.s)) - zy : 0.f;
    return st;
}
// dLoss/dLogit of class j from its exponential: w (softmax_j - [j = label]), 0 for a row that is not live
__device__ __forceinline__ float dz_value(const RowState &st, const float wgt, const float ex, const int j) {
    return st.live ? wgt * (ex / st.s - (j == st.y ? 1.f : 0.f)) : 0.f;
}

// ---- the weight gradient's blocks and its fold -----------------------------------------------------------------------------------------
constexpr int kTiles = 8;                            // 32 x 32 accumulator tiles per wavefront: 128 registers
constexpr int kTableFloats = kTiles * 1024;          // one workgroup's table: 32 KiB
constexpr int kRowsPerClass = 40;                    // R >= 40 C (d + 1) / d: the tables, 2 C (d + 1) floats per block, are <= 5 % of X
constexpr int kFold = 32;                            // tables in flight per thread of the fold

struct WgradRule {
    int64_t blocks, rows;                            // B, R
    int ct, ut, slabs;                               // class tiles x column tiles of a slab, S
};
bool wgrad_rule(int64_t n, int64_t d, int64_t c, WgradRule &out) {
    if (c > SGL_LINEAR_HEAD_MAX_C) return false;
    const int ct = c <= 32 ? 1 : (c <= 64 ? 2 : (c <= 128 ? 4 : 8)), ut = kTiles / ct;
    const int64_t tu = (d + 1 + 31) / 32;
    out = {0, 0, ct, ut, (int)((tu + ut - 1) / ut)};
    if (n == 0 || c == 0) return true;
    const int64_t forced = sgl::tuning("loss_blocks", 0);
    const int64_t rmin = d ? (kRowsPerClass * c * (d + 1) + d - 1) / d : kRowsPerClass * c;
    int64_t want = forced > 0 ? forced : (n / rmin > 1 ? n / rmin : 1);
    if (want > kMaxBlocks) want = kMaxBlocks;
    if (want > n) want = n;
    out.rows = (n + want - 1) / want;
    out.blocks = (n + out.rows - 1) / out.rows;
    return true;
}

// ((wave 0 + wave 1) + wave 2) + wave 3 in LDS, then the table [32 CT classes][32 UT columns] of this workgroup to `out`; only classes
// < c and columns <= d are written (and read by the fold).  Element (tile, v, lane) at tile * 1024 + v * 64 + lane: consecutive lanes,
// no conflict.  u0: the slab's first column tile.  Every thread of the workgroup calls it; `table` holds kTableFloats floats
template <int CT, int UT>
__device__ __forceinline__ void add_wavefront_tables(float *__restrict__ table, const f16v (&acc)[CT][UT], const int tiles_c,
                                                     const int tiles_u, const int u0, const int c, const int d, float *__restrict__ out) {
    const int lane = threadIdx.x % 64, wave = threadIdx.x / 64;
    for (int turn = 0; turn < 4; ++turn) {
        if (wave == turn) {
#pragma unroll
            for (int t = 0; t < CT; ++t)
#pragma unroll
                for (int u = 0; u < UT; ++u)
                    if (t < tiles_c && u < tiles_u) {
#pragma unroll
                        for (int v = 0; v < 16; ++v) {
                            float *at = table + (t * UT + u) * 1024 + v * 64 + lane;
                            *at = turn ? *at + acc[t][u][v] : acc[t][u][v];
                        }
                    }
        }
        __syncthreads();
    }
    for (int e = threadIdx.x; e < kTableFloats; e += 256) {
        const int tile = e / 1024, v = e / 64 % 16, l = e % 64, t = tile / UT, u = tile % UT;
        const int jl = 32 * t + 8 * (v / 4) + 4 * (l / 32) + v % 4, cl = 32 * u + l % 32;
        if (jl < c && 32 * u0 + cl <= d) out[jl * (32 * UT) + cl] = table[e];
    }
}

// dw[j, col] / db[j] = the B tables' values in ascending block order, one float32 add each; kFold loads are issued before their adds
__global__ __launch_bounds__(256) void linear_fold_kernel(const float *__restrict__ part, const int64_t blocks, const int slabs, const int ut,
                                                          const int c, const int d, float *__restrict__ dw, const int64_t lddw,
                                                          float *__restrict__ db) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)c * (d + 1)) return;
    const int64_t j = idx / (d + 1);
    const int col = (int)(idx % (d + 1)), s = col / (32 * ut);
    const float *p = part + (int64_t)s * kTableFloats + j * (32 * ut) + (col - s * 32 * ut);
    const int64_t stride = (int64_t)slabs * kTableFloats;
    float a = 0.f;
    int64_t b = 0;
    for (; b + kFold <= blocks; b += kFold) {
        float t[kFold];
#pragma unroll
        for (int e = 0; e < kFold; ++e) t[e] = p[(b + e) * stride];
#pragma unroll
        for (int e = 0; e < kFold; ++e) a = a + t[e];
    }
    for (; b < blocks; ++b) a = a + p[b * stride];
    if (col < d) dw[j * lddw + col] = a;
    else if (db) db[j] = a;
}

// the fold's launch: dw / db from `blocks` x `slabs` tables of 32 (8 / ut) x 32 ut floats
inline int launch_fold(const char *who, hipStream_t st, const float *part, int64_t blocks, int slabs, int ut, int c, int d, float *d_dw,
                       int64_t lddw, float *d_db) {
    const int64_t cells = (int64_t)c * (d + 1);
    if (!sgl::launch_fits((cells + 255) / 256, 256)) return sgl::fail(SGL_ERR_UNSUPPORTED, "%s: the grid does not fit one launch", who);
    hipLaunchKernelGGL(linear_fold_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, part, blocks, slabs, ut, c, d, d_dw, lddw,
                       d_db);
    SGL_LAUNCH_CHECK(who);
    return SGL_OK;
}

}  // namespace
#endif  // SGL_LINEAR_COMMON_H
