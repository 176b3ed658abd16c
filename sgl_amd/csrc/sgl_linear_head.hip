// K21: a linear classification head fused with its loss (include/sgl_linear_head.h states the contract and the bounds).  The unfused
// step writes the logits Z = X W^T + b [n, C], reads them again for the loss (K14) and runs two rocBLAS products in the backward; the
// head's GEMM is skinny (C <= 256) and memory-bound, which is the shape K18 (sgl_kmeans_mfma.hip) serves on v_mfma_f32_32x32x2_f32.
//
// linear_class_kernel.  K18's work split: Z^T[j][i] = sum_col W[j][col] x[i][col], the rows of W are the A operand (staged in LDS, row
// pitch W + 4 floats so that the 16-byte reads of 16 consecutive classes fall into 16 different bank groups; column chunks with carried
// accumulators when C (d + 4) floats exceed the tile), rows of X the B operand straight from memory: lane (i = lane % 32, h = lane / 32)
// takes the float4 at columns 8 q + 4 h of ITS row, element e of it is one MFMA step -- no transpose, and the chain of a logit is the
// same whatever the chunk width (a multiple of 8).  256 threads; a wavefront owns R tiles of 32 rows (R = 2 up to 4 class tiles, else
// 1) and keeps NT = ceil(C / 32) accumulator tiles per row tile (sgl::KmeansMatrixTiles).  Workgroups stride over batches of 4 R x 32
// rows (sgl::loss_batch_grid, K9's cap).
//
// The epilogue works in the accumulator layout: lane (i, h) holds the 16 NT logits 32 t + 8 g + 4 h + e (g, e = 0 .. 3) of row i, its
// partner lane i + 32 (v_permlane32_swap) the other 16 NT.  The bias is added from LDS; the maximum, the first NaN, the first column of
// the maximum (K14's Best, ascending in a lane), the sum of the exponentials and the logit of the label are in-lane loops followed by
// ONE exchange each; slots >= C are left out by a select on the slot.  A lane's logits are runs of 4 consecutive classes: z and dz are
// written as 16-byte stores where the output's base and pitch allow.
//
// linear_wgrad_kernel + linear_fold_kernel.  dW^T is not formed: D[j][col] = sum_i dz[i][j] x[i][col] with dz^T the A operand and X the
// B operand, the MFMA's k index the two rows of a pair -- lane (i, h) reads dz[row 2 s + h][32 t + i] and x[row 2 s + h][32 u + i], both
// 4-byte reads that a half-wave coalesces into one 128-byte piece of a row; edges are zeros by select, column d of X reads as 1 (db).
// K19's two levels: B row blocks x S slabs (blockIdx.x = b S + s: the workgroups that share rows are neighbours), 8 tiles of 32 x 32
// per wavefront resident for the life of the block, the four wavefronts added in LDS in a fixed order, one table per workgroup, a fold
// in ascending block order.
//
// K22 (include/sgl_linear_rows.h): the same two bodies on STORED rows -- the B operand is row idx[i] of a float32 or bfloat16 table, not
// row i of a dense float32 matrix.  The bodies take a row source <T, ROWS>: K21 is <float, false> and compiles to what it was; ROWS
// resolves the source row of a tile row once per batch (class kernel: one coalesced 8-byte read of idx per lane, python's negative wrap,
// a range check that turns a bad index into a row of NaN without a trap) resp. once per row pair (weight gradient: the half-wave reads
// one word), keeps the 64-bit row address, and tests "the table's last row" where K21 tests "the matrix's last row".  bfloat16: a lane's
// four columns are ONE 8-byte access (base 8-byte aligned, pitch a multiple of 4 elements; else four 2-byte ones), each element widened
// exactly (bits << 16) into the float the MFMA takes -- W stays float32 in LDS, so a logit's chain and its bits are those of K21 on the
// widened rows.  In flight per wavefront and look-ahead step (kStep = 32 columns): 4 R row loads per lane, 16 bytes each for float32
// (R x 4 KiB per wavefront), 8 bytes each for bfloat16 (R x 2 KiB).  The lane width of W is a run-time flag here (staging is once per
// workgroup), so a table's wide lanes do not depend on W's pitch as they do in K21.
#include "sgl_linear_common.h"   // the row source, the staging of W, the chain, the epilogue, the block rule and the fold: shared with K23

#include "../../include/sgl_linear_rows.h"

namespace {

constexpr int kTileFloats = 16384;                   // LDS of a workgroup of linear_class_kernel: 64 KiB
constexpr int kStep = 32;                            // columns of X a lane pair takes per step: 4 vectors in each half

constexpr int row_tiles(int nt) { return nt <= 4 ? 2 : 1; }   // R: 2 x NT x 16 accumulator registers stay within 128

struct ClassRule {
    int nt, r, w, p;     // class tiles, row tiles per wavefront, columns staged at once, LDS pitch
};
bool class_rule(int64_t d, int64_t c, ClassRule &out) {
    const sgl::ChunkList tiles = sgl::KmeansMatrixTiles::list();
    const int64_t need = (c + 31) / 32;
    int nt = 0;
    for (int t = tiles.count - 1; t >= 0; --t)
        if (tiles.values[t] >= need) nt = tiles.values[t];
    if (!nt) return false;
    const int64_t dp = (d + 7) / 8 * 8, budget = kTileFloats - nt * 32;
    int64_t w = dp;
    if (c * (dp + kPitchPad) > budget) w = (budget / c - kPitchPad) / 8 * 8;   // >= 48 at c = 256
    out = {nt, row_tiles(nt), (int)w, (int)w + kPitchPad};
    return true;
}

// <float, false>: K21, row i of x [n, d].  ROWS: batch row i is row idx[i] of the table x [n_rows, d] of T; VEC is x's lane width alone
// and w_vec W's
template <typename T, bool ROWS, int VEC, int NT, int R>
__global__ __launch_bounds__(256) void linear_class_kernel(const T *__restrict__ x, const int64_t ldx, const int64_t n, const int d,
                                                           const int64_t *__restrict__ idx, const int64_t n_rows, const bool w_vec,
                                                           const float *__restrict__ wt, const int64_t ldw, const int c,
                                                           const float *__restrict__ bias, const int64_t *__restrict__ labels,
                                                           const float wgt, const int w, const int p, const int64_t n_batches,
                                                           float *__restrict__ row_loss, int64_t *__restrict__ pred,
                                                           float *__restrict__ dz, const int64_t lddz, const bool dz_vec,
                                                           float *__restrict__ z, const int64_t ldz, const bool z_vec) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *tile = lds, *bs = lds + c * p;
    const int lane = threadIdx.x % 64, i = lane % 32, h = lane / 32, wave = threadIdx.x / 64;
    const bool one_chunk = w >= d, want_exp = dz != nullptr || row_loss != nullptr;
    bool staged = false;
    for (int j = threadIdx.x; j < NT * 32; j += 256) bs[j] = (bias && j < c) ? bias[j] : 0.f;
    __syncthreads();
    for (int64_t b = blockIdx.x; b < n_batches; b += gridDim.x) {
        bool in[R], last[R], bad[R];
        const T *xp[R];
        f16v acc[R][NT];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int64_t row = (b * 4 * R + wave * R + r) * 32 + i;
            in[r] = row < n;
            int64_t from = in[r] ? row : 0;          // a tile row beyond the matrix loads nothing and writes nothing
            bad[r] = false;
            if constexpr (ROWS) {
                if (in[r]) from = source_row(idx, row, n_rows, bad[r]);
                last[r] = from == n_rows - 1;        // of the TABLE: the edge vector of any other row stays inside its pitch
            } else {
                last[r] = from == n - 1;
            }
            xp[r] = x + from * ldx;
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int v = 0; v < 16; ++v) acc[r][t][v] = 0.f;
        }
        for (int c0 = 0; c0 < d; c0 += w) {
            const int left = (d - c0 + 7) / 8 * 8, wc = left < w ? left : w;
            if (!(staged && one_chunk)) {            // all columns fit: staged once per workgroup, not once per batch
                __syncthreads();                     // the tile's last readers are done
                if constexpr (!ROWS) stage_weights<VEC>(tile, wt, ldw, c, d, c0, wc, p);
                else if (w_vec) stage_weights<4>(tile, wt, ldw, c, d, c0, wc, p);
                else stage_weights<1>(tile, wt, ldw, c, d, c0, wc, p);
                __syncthreads();
                staged = true;
            }
            for (int q0 = 0; q0 < wc; q0 += kStep) {
                f4 xr[R][4];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int col = c0 + q0 + 8 * t + 4 * h;
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        f4 v = {0.f, 0.f, 0.f, 0.f};
                        if (q0 + 8 * t < wc && in[r] && col < d) v = load4<VEC>(xp[r], col, d, last[r]);
                        if constexpr (ROWS) {
                            if (bad[r]) v = nan_cols(col, d);
                        }
                        xr[r][t] = v;
                    }
                }
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    if (q0 + 8 * t < wc) {           // the same for every lane
                        f4 xv[R];
#pragma unroll
                        for (int r = 0; r < R; ++r) xv[r] = xr[r][t];
                        logit_group<NT, R>(acc, tile, p, c, i, q0 + 8 * t + 4 * h, xv);
                    }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int64_t row = (b * 4 * R + wave * R + r) * 32 + i;
            const RowState st = class_epilogue<NT>(acc[r], bs, c, h, in[r], row, labels, want_exp, row_loss, pred, z, ldz, z_vec);
            if (!want_exp || !in[r]) continue;
            if (dz) {
                float *orow = dz + row * lddz;
#pragma unroll
                for (int ct = 0; ct < NT; ++ct)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int j0 = ct * 32 + 8 * g + 4 * h;
                        f4 o;
#pragma unroll
                        for (int e = 0; e < 4; ++e) o[e] = dz_value(st, wgt, acc[r][ct][4 * g + e], j0 + e);
                        if (j0 < c) store_cols<4>(orow, j0, c, o, dz_vec);
                    }
            }
        }
    }
}

// ---- the weight gradient -------------------------------------------------------------------------------------------------------------
constexpr int kPairs = 8;                            // row pairs a wavefront loads before their MFMA steps

// <float, false>: K21.  ROWS: row `row` of dz meets row idx[row] of the table x [n_rows, d] of T -- the same for a whole half-wave,
// resolved once per pair; 2-byte reads for bfloat16 (64 bytes per half-wave and row), widened exactly
template <typename T, bool ROWS, int CT>
__global__ __launch_bounds__(256) void linear_wgrad_kernel(const T *__restrict__ x, const int64_t ldx, const int64_t n, const int d,
                                                           const int64_t *__restrict__ idx, const int64_t n_rows,
                                                           const float *__restrict__ dz, const int64_t lddz, const int c,
                                                           const int64_t rows, const int slabs, float *__restrict__ part) {
    constexpr int UT = kTiles / CT;
    __shared__ float table[kTableFloats];
    const int lane = threadIdx.x % 64, i = lane % 32, h = lane / 32, wave = threadIdx.x / 64;
    const int64_t b = blockIdx.x / slabs;
    const int s = (int)(blockIdx.x % slabs), u0 = s * UT;
    const int64_t r0 = b * rows, r1 = r0 + rows < n ? r0 + rows : n;
    const int tiles_c = (c + 31) / 32, tiles_u = (d + 1 + 31) / 32 - u0;      // live tiles of the slab (the same for every lane)
    const int64_t pairs = (r1 - r0 + 1) / 2;
    f16v acc[CT][UT];
#pragma unroll
    for (int t = 0; t < CT; ++t)
#pragma unroll
        for (int u = 0; u < UT; ++u)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[t][u][v] = 0.f;

    for (int64_t p0 = wave; p0 < pairs; p0 += 4 * kPairs) {                   // this wavefront's pairs p0, p0 + 4, ...: ascending rows
        float a[kPairs][CT], bb[kPairs][UT];
#pragma unroll
        for (int k = 0; k < kPairs; ++k) {
            const int64_t row = r0 + 2 * (p0 + 4 * k) + h;
            const bool on = row < r1;                // the odd row of a last pair, the pairs beyond the block: zeros
            int64_t src = row;
            bool bad = false;
            if constexpr (ROWS) {
                if (on) src = source_row(idx, row, n_rows, bad);
            }
            const T *xrow = x + src * ldx;
#pragma unroll
            for (int t = 0; t < CT; ++t) {
                const int j = 32 * t + i;
                a[k][t] = (on && j < c) ? dz[row * lddz + j] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < UT; ++u) {
                const int col = 32 * (u0 + u) + i;
                float v = (on && col == d) ? 1.f : 0.f;
                if (on && col < d) v = bad ? __uint_as_float(0x7fc00000u) : widen(xrow[col]);
                bb[k][u] = v;
            }
        }
#pragma unroll
        for (int k = 0; k < kPairs; ++k) {
            if (p0 + 4 * k < pairs) {                // the same for every lane of the wavefront
#pragma unroll
                for (int t = 0; t < CT; ++t)
#pragma unroll
                    for (int u = 0; u < UT; ++u)
                        if (t < tiles_c && u < tiles_u) acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[k][t], bb[k][u], acc[t][u], 0, 0, 0);
            }
        }
    }
    add_wavefront_tables<CT, UT>(table, acc, tiles_c, tiles_u, u0, c, d, part + (int64_t)blockIdx.x * kTableFloats);
}

int check_wgrad(const char *who, int64_t n, int64_t d, int64_t c, WgradRule &rule) {
    if (!(n >= 0 && d >= 0 && d < INT32_MAX && c >= 0)) return sgl::fail(SGL_ERR_INVALID, "%s: bad sizes", who);
    SGL_REQUIRE_WIDTH(who, "d", d);
    if (!wgrad_rule(n, d, c, rule))
        return sgl::fail(SGL_ERR_UNSUPPORTED, "%s: c=%lld is beyond the compiled range (c <= %d)", who, (long long)c, SGL_LINEAR_HEAD_MAX_C);
    return SGL_OK;
}

}  // namespace

SGL_EXPORT int sgl_linear_class_rule(int64_t d, int64_t c, int rule[4]) {
    SGL_REQUIRE(rule, "sgl_linear_class_rule: NULL arguments");
    SGL_REQUIRE(d >= 0 && d < INT32_MAX && c >= 1, "sgl_linear_class_rule: bad sizes");
    SGL_REQUIRE_WIDTH("sgl_linear_class_rule", "d", d);
    ClassRule r;
    if (!class_rule(d, c, r))
        return sgl::fail(SGL_ERR_UNSUPPORTED, "sgl_linear_class_rule: c=%lld is beyond the compiled range (c <= %d)", (long long)c,
                         SGL_LINEAR_HEAD_MAX_C);
    rule[0] = r.nt, rule[1] = r.r, rule[2] = r.w, rule[3] = r.p;
    return SGL_OK;
}

namespace {

// Both headers' class entry points: batch row i is row d_idx[i] of the table x [n_rows, d].  K21 passes its matrix x [n, d] without an
// index (n_rows = n); a float32 table without an index list IS K21's matrix and takes K21's instance
template <typename T>
int linear_class(const char *who, const T *d_x, int64_t ldx, int64_t n_rows, const int64_t *d_idx, int64_t n, int64_t d,
                 const float *d_w, int64_t ldw, int64_t c, const float *d_bias, const int64_t *d_labels, float w, float *d_row_loss,
                 int64_t *d_pred, float *d_dz, int64_t lddz, float *d_z, int64_t ldz, void *stream) {
    SGL_REQUIRE(n >= 0 && n_rows >= 0 && d >= 0 && d < INT32_MAX && c >= 1 && c < INT32_MAX, "%s: bad sizes (n >= 0, d >= 0, c >= 1)", who);
    SGL_REQUIRE_WIDTH(who, "d", d);
    SGL_REQUIRE(d_idx || n == n_rows, "%s: without d_idx every row is taken, m must be n_rows", who);
    SGL_REQUIRE(n_rows > 0 || n == 0, "%s: indices into a table without rows", who);
    SGL_REQUIRE(d_row_loss || d_pred || d_dz || d_z || n == 0, "%s: at least one of d_row_loss, d_pred, d_dz and d_z is needed", who);
    SGL_REQUIRE((d_x || n == 0 || d == 0) && (d_w || d == 0), "%s: NULL arguments", who);
    SGL_REQUIRE(d_labels || n == 0 || !(d_dz || d_row_loss), "%s: d_labels may be NULL only without d_row_loss and d_dz", who);
    SGL_REQUIRE(ldx >= d && ldw >= d && (lddz >= c || !d_dz) && (ldz >= c || !d_z), "%s: row pitch smaller than the row", who);
    SGL_REQUIRE(aligned_to(d_x, sizeof(T)) && aligned_to(d_w, 4) && aligned_to(d_bias, 4) && aligned_to(d_dz, 4) && aligned_to(d_z, 4) &&
                    aligned_to(d_row_loss, 4) && aligned_to(d_labels, 8) && aligned_to(d_pred, 8) && aligned_to(d_idx, 8),
                "%s: pointers must be aligned to their element size", who);
    ClassRule rule;
    if (!class_rule(d, c, rule))
        return sgl::fail(SGL_ERR_UNSUPPORTED, "%s: c=%lld is beyond the compiled range (c <= %d)", who, (long long)c, SGL_LINEAR_HEAD_MAX_C);
    if (n == 0) return SGL_OK;
    hipStream_t st = sgl::as_stream(stream);
    const bool x_vec = ldx % 4 == 0 && aligned_to(d_x, 4 * sizeof(T)), w_vec = ldw % 4 == 0 && aligned_to(d_w, 16);
    const bool dz_vec = d_dz && lddz % 4 == 0 && aligned_to(d_dz, 16), z_vec = d_z && ldz % 4 == 0 && aligned_to(d_z, 16);
    if (!sgl::launch_fits(kMaxBlocks, 256)) return sgl::fail(SGL_ERR_UNSUPPORTED, "%s: the grid does not fit one launch", who);
    const int di = (int)d, ci = (int)c;
    const bool dense = std::is_same<T, float>::value && !d_idx;
    with_chunks(sgl::KmeansMatrixTiles{}, rule.nt, [&](auto N) {
        with_vec(dense ? x_vec && w_vec : x_vec, [&](auto V) {
            constexpr int R = row_tiles(N);
            const sgl::BatchGrid grid = sgl::loss_batch_grid(n, 4, R * 32, kMaxBlocks);
            const size_t lds = ((size_t)ci * rule.p + N * 32) * sizeof(float);
            auto launch = [&](auto kernel) {
                hipLaunchKernelGGL(kernel, dim3((unsigned)grid.blocks), dim3(256), lds, st, d_x, ldx, n, di, d_idx, n_rows, w_vec, d_w, ldw, ci,
                                   d_bias, d_labels, w, rule.w, rule.p, grid.n_batches, d_row_loss, d_pred, d_dz, lddz, dz_vec, d_z, ldz, z_vec);
            };
            if constexpr (std::is_same<T, float>::value) {
                if (dense) launch(linear_class_kernel<float, false, V, N, R>);
                else launch(linear_class_kernel<float, true, V, N, R>);
            } else {
                launch(linear_class_kernel<T, true, V, N, R>);
            }
        });
    });
    SGL_LAUNCH_CHECK(who);
    return SGL_OK;
}

}  // namespace

SGL_EXPORT int sgl_linear_class_f32(const float *d_x, int64_t ldx, int64_t n, int64_t d, const float *d_w, int64_t ldw, int64_t c,
                                    const float *d_bias, const int64_t *d_labels, float w, float *d_row_loss, int64_t *d_pred, float *d_dz,
                                    int64_t lddz, float *d_z, int64_t ldz, void *stream) {
    return linear_class("sgl_linear_class_f32", d_x, ldx, n, nullptr, n, d, d_w, ldw, c, d_bias, d_labels, w, d_row_loss, d_pred, d_dz,
                        lddz, d_z, ldz, stream);
}

SGL_EXPORT int sgl_linear_class_rows_f32(const float *d_x, int64_t ldx, int64_t n_rows, const int64_t *d_idx, int64_t m, int64_t d,
                                         const float *d_w, int64_t ldw, int64_t c, const float *d_bias, const int64_t *d_labels, float w,
                                         float *d_row_loss, int64_t *d_pred, float *d_dz, int64_t lddz, float *d_z, int64_t ldz, void *stream) {
    return linear_class("sgl_linear_class_rows_f32", d_x, ldx, n_rows, d_idx, m, d, d_w, ldw, c, d_bias, d_labels, w, d_row_loss, d_pred,
                        d_dz, lddz, d_z, ldz, stream);
}

SGL_EXPORT int sgl_linear_class_rows_bf16(const uint16_t *d_x, int64_t ldx, int64_t n_rows, const int64_t *d_idx, int64_t m, int64_t d,
                                          const float *d_w, int64_t ldw, int64_t c, const float *d_bias, const int64_t *d_labels, float w,
                                          float *d_row_loss, int64_t *d_pred, float *d_dz, int64_t lddz, float *d_z, int64_t ldz, void *stream) {
    return linear_class("sgl_linear_class_rows_bf16", d_x, ldx, n_rows, d_idx, m, d, d_w, ldw, c, d_bias, d_labels, w, d_row_loss, d_pred,
                        d_dz, lddz, d_z, ldz, stream);
}

SGL_EXPORT int sgl_linear_wgrad_rule(int64_t n, int64_t d, int64_t c, int64_t *out) {
    SGL_REQUIRE(out, "sgl_linear_wgrad_rule: bad arguments");
    WgradRule r;
    const int rc = check_wgrad("sgl_linear_wgrad_rule", n, d, c, r);
    if (rc != SGL_OK) return rc;
    out[0] = r.blocks, out[1] = r.rows, out[2] = r.ct, out[3] = r.ut, out[4] = r.slabs;
    return SGL_OK;
}

SGL_EXPORT int64_t sgl_linear_wgrad_scratch(int64_t n, int64_t d, int64_t c) {
    WgradRule r;
    return check_wgrad("sgl_linear_wgrad_scratch", n, d, c, r) == SGL_OK ? r.blocks * r.slabs * kTableFloats * (int64_t)sizeof(float) : -1;
}

namespace {

// Both headers' weight gradients: the row source as in linear_class; the rule and the scratch are sgl_linear_wgrad_rule's with n = the
// rows of dz
template <typename T>
int linear_wgrad(const char *who, const T *d_x, int64_t ldx, int64_t n_rows, const int64_t *d_idx, int64_t n, int64_t d, const float *d_dz,
                 int64_t lddz, int64_t c, float *d_dw, int64_t lddw, float *d_db, void *d_scratch, void *stream) {
    WgradRule rule;
    const int rc = check_wgrad(who, n, d, c, rule);
    if (rc != SGL_OK) return rc;
    SGL_REQUIRE(n_rows >= 0 && (d_idx || n == n_rows), "%s: without d_idx every row is taken, m must be n_rows", who);
    SGL_REQUIRE(n_rows > 0 || n == 0, "%s: indices into a table without rows", who);
    SGL_REQUIRE((d_x || n == 0 || d == 0) && (d_dz || n == 0 || c == 0) && (d_dw || c == 0 || d == 0) && (d_scratch || rule.blocks == 0),
                "%s: NULL arguments", who);
    SGL_REQUIRE(ldx >= d && lddz >= c && lddw >= d, "%s: row pitch smaller than the row", who);
    SGL_REQUIRE(aligned_to(d_x, sizeof(T)) && aligned_to(d_dz, 4) && aligned_to(d_dw, 4) && aligned_to(d_db, 4) && aligned_to(d_scratch, 16) &&
                    aligned_to(d_idx, 8),
                "%s: pointers must be aligned to their element size (the scratch to 16 bytes)", who);
    if (c == 0) return SGL_OK;
    hipStream_t st = sgl::as_stream(stream);
    const int ci = (int)c, di = (int)d;
    float *part = static_cast<float *>(d_scratch);
    if (rule.blocks) {
        const int64_t grid = rule.blocks * rule.slabs;
        if (!sgl::launch_fits(grid, 256)) return sgl::fail(SGL_ERR_UNSUPPORTED, "%s: the grid does not fit one launch", who);
        with_one_of<1, 2, 4, 8>(rule.ct, [&](auto CT) {
            auto launch = [&](auto kernel) {
                hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(256), 0, st, d_x, ldx, n, di, d_idx, n_rows, d_dz, lddz, ci, rule.rows,
                                   rule.slabs, part);
            };
            if constexpr (std::is_same<T, float>::value) {
                if (!d_idx) launch(linear_wgrad_kernel<float, false, CT>);
                else launch(linear_wgrad_kernel<float, true, CT>);
            } else {
                launch(linear_wgrad_kernel<T, true, CT>);
            }
        });
        SGL_LAUNCH_CHECK(who);
    }
    return launch_fold(who, st, part, rule.blocks, rule.slabs, rule.ut, ci, di, d_dw, lddw, d_db);
}

}  // namespace

SGL_EXPORT int sgl_linear_wgrad_f32(const float *d_x, int64_t ldx, int64_t n, int64_t d, const float *d_dz, int64_t lddz, int64_t c,
                                    float *d_dw, int64_t lddw, float *d_db, void *d_scratch, void *stream) {
    return linear_wgrad("sgl_linear_wgrad_f32", d_x, ldx, n, nullptr, n, d, d_dz, lddz, c, d_dw, lddw, d_db, d_scratch, stream);
}

SGL_EXPORT int sgl_linear_wgrad_rows_f32(const float *d_x, int64_t ldx, int64_t n_rows, const int64_t *d_idx, int64_t m, int64_t d,
                                         const float *d_dz, int64_t lddz, int64_t c, float *d_dw, int64_t lddw, float *d_db, void *d_scratch,
                                         void *stream) {
    return linear_wgrad("sgl_linear_wgrad_rows_f32", d_x, ldx, n_rows, d_idx, m, d, d_dz, lddz, c, d_dw, lddw, d_db, d_scratch, stream);
}

SGL_EXPORT int sgl_linear_wgrad_rows_bf16(const uint16_t *d_x, int64_t ldx, int64_t n_rows, const int64_t *d_idx, int64_t m, int64_t d,
                                          const float *d_dz, int64_t lddz, int64_t c, float *d_dw, int64_t lddw, float *d_db, void *d_scratch,
                                          void *stream) {
    return linear_wgrad("sgl_linear_wgrad_rows_bf16", d_x, ldx, n_rows, d_idx, m, d, d_dz, lddz, c, d_dw, lddw, d_db, d_scratch, stream);
}
