// K23: the training step of the linear head in one pass over X (include/sgl_linear_step.h states the contract, the shapes and the
// bound).  K21's step reads X twice and sends dZ [n, C] through memory: linear_class_kernel writes it, linear_wgrad_kernel reads it and X
// again, 4 bytes per lane.  Here a wavefront keeps a tile of 32 rows in registers from the one wide load to the last use: it forms the
// logits (logit_group: K21's chain, W in LDS), runs K21's epilogue on the accumulators (class_epilogue: row_loss, pred, the
// exponentials), and feeds dz and X -- both transposed through a wavefront-private LDS tile -- to the MFMA steps of (dW | db), whose
// CT x UT tiles of 32 classes x 32 columns stay in the accumulator registers of the wavefront for the whole row block.
//
// linear_step_kernel<T, ROWS, VEC, CT, UT>.  (CT, UT) = (1, 7), (2, 4), (4, 2): the class and column tiles a wavefront holds (the rule
// admits ceil((d + 1) / 32) <= UT; why (1, 8) and (8, 1) are not compiled: the resource table of DESIGN K23).  blockIdx.x = the row
// block b of `rows` rows; wavefront v takes its tiles v, v + 4, ...  Per tile, lane (i = lane % 32, h = lane / 32):
//   1. xk[u][t] = columns 32 u + 8 t + 4 h .. + 3 of row i (load4 of the row source <T, ROWS>): UT x 4 loads in flight, all issued
//      before the first MFMA step -- up to 32 KiB per wavefront.
//   2. acc[ct] += logit_group over the groups of 8 columns in ascending order; class_epilogue; acc leaves as exp(z - max).
//   3. for every live class tile t: lane (i, h) writes dz[i][32 t + 8 g + 4 h .. + 3] (g = 0 .. 3) to its wavefront's tile as 16-byte
//      rows of pitch 36 floats, and reads a[s] = tile[row(s) + 8 h][i], row(s) = 16 (s / 8) + s % 8: the A operand of step s.
//      for every live column tile u: the same with xk[u][.] (column d reads as 1 in a row of the block) gives b[s], then 16 MFMA
//      steps dacc[t][u] += a[s] (x) b[s].  A tile pair costs 4 + 16 LDS accesses per lane for its 16 MFMA steps.
//   Rows beyond the block or n carry dz = 0 and x = 0; a row that is not live carries dz = 0.
// BANKS (64 banks of 4 bytes).  Row-major write: lane (i, h) at word 36 i + 8 g + 4 h; a 16-byte access is served 16 lanes at a time and
// 36 i / 4 = 9 i is a bijection mod 16, so 16 consecutive rows cover the 16 groups of 4 banks once.  Transposed read: lane (i, h) at
// word 36 (row(s) + 8 h) + i; 36 * 8 = 288 = 4 * 64 + 32, so half 1 reads the 32 banks that half 0, 32 consecutive words, leaves free.
// That is why a step pairs rows r and r + 8, not r and r + 1 (36 = 32 + 4 would collide in 4 banks).  The tile is private to its
// wavefront: its accesses are ordered by wave_sync (a fence for the compiler; LDS serves a wavefront in order), not by a barrier.
// After the last tile: __syncthreads, then add_wavefront_tables (K21's) in the first 32 KiB of LDS, over W and the tiles.
#include "sgl_linear_common.h"

#include "../../include/sgl_linear_step.h"

namespace {

constexpr int kTilePitch = 36;                       // floats: 32 + 4 (BANKS)
constexpr int kTileWords = 32 * kTilePitch;          // one wavefront's transposing tile

struct StepRule {
    int64_t blocks, rows;                            // B, R: the weight gradient's
    int ct, tu;                                      // class tiles (1 / 2 / 4 / 8), live column tiles ceil((d + 1) / 32)
    int p;                                           // LDS pitch of W: 8 ceil(d / 8) + 4
    int64_t lds;                                     // bytes
};
constexpr int kStepMaxC = SGL_LINEAR_STEP_MAX_C;
constexpr int column_tiles(int ct) { return ct == 1 ? 7 : kTiles / ct; }   // UT of the instance with ct class tiles

// 0: fine, 1: c beyond the compiled range, 2: the tiles do not fit a wavefront
int step_rule(int64_t n, int64_t d, int64_t c, StepRule &out) {
    WgradRule w;
    if (c > kStepMaxC || !wgrad_rule(n, d, c, w)) return 1;
    const int64_t tu = (d + 1 + 31) / 32;
    if (tu > column_tiles(w.ct)) return 2;
    const int64_t p = (d + 7) / 8 * 8 + kPitchPad, words = c * p + 32 * w.ct + 4 * kTileWords;
    out = {w.blocks, w.rows, w.ct, (int)tu, (int)p, 4 * (words > kTableFloats ? words : (int64_t)kTableFloats)};
    return 0;
}

int check_step(const char *who, int64_t n, int64_t d, int64_t c, StepRule &rule) {
    if (!(n >= 0 && d >= 0 && d < INT32_MAX && c >= 1)) return sgl::fail(SGL_ERR_INVALID, "%s: bad sizes (n >= 0, d >= 0, c >= 1)", who);
    const int rc = step_rule(n, d, c, rule);
    if (rc == 1)
        return sgl::fail(SGL_ERR_UNSUPPORTED, "%s: c=%lld is beyond what sgl_linear_step_rule admits (c <= %d)", who, (long long)c, kStepMaxC);
    if (rc == 2)
        return sgl::fail(SGL_ERR_UNSUPPORTED,
                         "%s: d=%lld, c=%lld needs %lld class tiles x %lld column tiles of 32 x 32; sgl_linear_step_rule admits "
                         "ceil((d + 1) / 32) <= 7 with 1 class tile, <= 4 with 2, <= 2 with 4",
                         who, (long long)d, (long long)c, (long long)(c <= 32 ? 1 : (c <= 64 ? 2 : 4)), (long long)((d + 1 + 31) / 32));
    return SGL_OK;
}

// orders this wavefront's LDS accesses before and after it: the compiler moves none across, the hardware serves them in order
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the operand of the 16 steps of a tile pair from a tile written row-major: out[s] = tile[16 (s / 8) + s % 8 + 8 h][i]
__device__ __forceinline__ void read_transposed(const float *__restrict__ mine, const int i, const int h, float (&out)[16]) {
#pragma unroll
    for (int s = 0; s < 16; ++s) out[s] = mine[(16 * (s / 8) + s % 8 + 8 * h) * kTilePitch + i];
}

template <typename T, bool ROWS, int VEC, int CT, int UT>
__global__ __launch_bounds__(256) void linear_step_kernel(const T *__restrict__ x, const int64_t ldx, const int64_t n, const int d,
                                                          const int64_t *__restrict__ idx, const int64_t n_rows, const bool w_vec,
                                                          const float *__restrict__ wt, const int64_t ldw, const int c,
                                                          const float *__restrict__ bias, const int64_t *__restrict__ labels,
                                                          const float wgt, const int p, const int64_t rows,
                                                          float *__restrict__ row_loss, int64_t *__restrict__ pred,
                                                          float *__restrict__ part) {
    static_assert(CT * UT <= kTiles, "a wavefront's table is 8 tiles");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x % 64, i = lane % 32, h = lane / 32, wave = threadIdx.x / 64;
    float *tile = lds, *bs = lds + c * p, *mine = bs + 32 * CT + wave * kTileWords;
    const int wc = (d + 7) / 8 * 8, tiles_c = (c + 31) / 32, tiles_u = (d + 1 + 31) / 32;   // the same for every lane
    const int64_t r0 = (int64_t)blockIdx.x * rows, r1 = r0 + rows < n ? r0 + rows : n;
    for (int j = threadIdx.x; j < CT * 32; j += 256) bs[j] = (bias && j < c) ? bias[j] : 0.f;
    if (w_vec) stage_weights<4>(tile, wt, ldw, c, d, 0, wc, p);
    else stage_weights<1>(tile, wt, ldw, c, d, 0, wc, p);
    __syncthreads();

    f16v dacc[CT][UT];
#pragma unroll
    for (int t = 0; t < CT; ++t)
#pragma unroll
        for (int u = 0; u < UT; ++u)
#pragma unroll
            for (int v = 0; v < 16; ++v) dacc[t][u][v] = 0.f;

    const int64_t n_tiles = (r1 - r0 + 31) / 32;
    for (int64_t tl = wave; tl < n_tiles; tl += 4) {
        const int64_t row = r0 + tl * 32 + i;
        const bool in = row < r1;
        int64_t from = in ? row : 0;                 // a tile row beyond the block loads nothing and adds nothing
        bool bad = false, last;
        if constexpr (ROWS) {
            if (in) from = source_row(idx, row, n_rows, bad);
            last = from == n_rows - 1;
        } else {
            last = from == n - 1;
        }
        const T *xp = x + from * ldx;
        f4 xk[UT][4];
#pragma unroll
        for (int u = 0; u < UT; ++u)
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int col = 32 * u + 8 * t + 4 * h;
                f4 v = {0.f, 0.f, 0.f, 0.f};
                if constexpr (ROWS) {
                    if (bad) v = nan_cols(col, d);
                }
                if (in && !bad && col < d) v = load4<VEC>(xp, col, d, last);
                xk[u][t] = v;
            }
        f16v acc[1][CT];
#pragma unroll
        for (int t = 0; t < CT; ++t)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[0][t][v] = 0.f;
#pragma unroll
        for (int u = 0; u < UT; ++u)
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (32 * u + 8 * t < wc) {           // the same for every lane
                    const f4 xv[1] = {xk[u][t]};
                    logit_group<CT, 1>(acc, tile, p, c, i, 32 * u + 8 * t + 4 * h, xv);
                    __builtin_amdgcn_sched_barrier(0);   // W's reads stay with their steps: hoisted, they cost 4 registers per group
                }
        const RowState st = class_epilogue<CT>(acc[0], bs, c, h, in, row, labels, true, row_loss, pred, nullptr, 0, false);
        // in place, so that no second copy of either operand is ever live: the exponentials become dz, column d of the row becomes 1
#pragma unroll
        for (int t = 0; t < CT; ++t)
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int j = 32 * t + 8 * (v / 4) + 4 * h + v % 4;
                acc[0][t][v] = (in && j < c) ? dz_value(st, wgt, acc[0][t][v], j) : 0.f;
                if (v % 4 == 3) __builtin_amdgcn_sched_barrier(0);   // four divisions at a time: their temporaries are many
            }
        {
            const int u = d / 32, q = d % 32 / 8, e = d % 4;   // where column d stands: the same for every lane
            if (in && (d % 8) / 4 == h) {
#pragma unroll
                for (int uu = 0; uu < UT; ++uu)
#pragma unroll
                    for (int qq = 0; qq < 4; ++qq)
#pragma unroll
                        for (int ee = 0; ee < 4; ++ee)
                            if (uu == u && qq == q && ee == e) xk[uu][qq][ee] = 1.f;   // the column of ones: db
            }
        }

#pragma unroll
        for (int t = 0; t < CT; ++t) {
            if (t >= tiles_c) continue;
            wave_sync();                             // the tile's last reads are done
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f4 o = {acc[0][t][4 * g], acc[0][t][4 * g + 1], acc[0][t][4 * g + 2], acc[0][t][4 * g + 3]};
                *reinterpret_cast<f4 *>(mine + i * kTilePitch + 8 * g + 4 * h) = o;
            }
            wave_sync();
            float a[16];
            read_transposed(mine, i, h, a);
#pragma unroll
            for (int u = 0; u < UT; ++u) {
                if (u >= tiles_u) continue;
                wave_sync();
#pragma unroll
                for (int q = 0; q < 4; ++q) *reinterpret_cast<f4 *>(mine + i * kTilePitch + 8 * q + 4 * h) = xk[u][q];
                wave_sync();
                float bb[16];
                read_transposed(mine, i, h, bb);
#pragma unroll
                for (int s = 0; s < 16; ++s) dacc[t][u] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], bb[s], dacc[t][u], 0, 0, 0);
            }
        }
    }
    __syncthreads();                                 // W and the tiles have had their last readers: the table takes their place
    add_wavefront_tables<CT, UT>(lds, dacc, tiles_c, tiles_u, 0, c, d, part + (int64_t)blockIdx.x * kTableFloats);
}

// every entry point: batch row i is row d_idx[i] of the table x [n_rows, d]; the dense one passes its matrix without an index
// (n_rows = n), and a float32 table without an index list IS that matrix and takes its instance
template <typename T>
int linear_step(const char *who, const T *d_x, int64_t ldx, int64_t n_rows, const int64_t *d_idx, int64_t n, int64_t d, const float *d_w,
                int64_t ldw, int64_t c, const float *d_bias, const int64_t *d_labels, float w, float *d_row_loss, int64_t *d_pred,
                float *d_dw, int64_t lddw, float *d_db, void *d_scratch, void *stream) {
    SGL_REQUIRE(n_rows >= 0 && c < INT32_MAX, "%s: bad sizes", who);
    SGL_REQUIRE_WIDTH(who, "d", d);
    SGL_REQUIRE(d_dw && d_db, "%s: d_dw and d_db are required", who);
    SGL_REQUIRE(ldx >= d && ldw >= d && lddw >= d, "%s: row pitch smaller than the row", who);
    StepRule rule;
    const int rc = check_step(who, n, d, c, rule);
    if (rc != SGL_OK) return rc;
    SGL_REQUIRE(d_idx || n == n_rows || n == 0, "%s: without d_idx every row is taken, m must be n_rows", who);   // an empty list has no address
    SGL_REQUIRE(n_rows > 0 || n == 0, "%s: indices into a table without rows", who);
    SGL_REQUIRE((d_x || n == 0 || d == 0) && (d_w || d == 0) && (d_labels || n == 0) && (d_scratch || rule.blocks == 0), "%s: NULL arguments",
                who);
    SGL_REQUIRE(aligned_to(d_x, sizeof(T)) && aligned_to(d_w, 4) && aligned_to(d_bias, 4) && aligned_to(d_row_loss, 4) &&
                    aligned_to(d_labels, 8) && aligned_to(d_pred, 8) && aligned_to(d_idx, 8) && aligned_to(d_dw, 4) && aligned_to(d_db, 4) &&
                    aligned_to(d_scratch, 16),
                "%s: pointers must be aligned to their element size (the scratch to 16 bytes)", who);
    hipStream_t st = sgl::as_stream(stream);
    const int ci = (int)c, di = (int)d;
    float *part = static_cast<float *>(d_scratch);
    if (rule.blocks) {
        if (!sgl::launch_fits(rule.blocks, 256)) return sgl::fail(SGL_ERR_UNSUPPORTED, "%s: the grid does not fit one launch", who);
        const bool x_vec = ldx % 4 == 0 && aligned_to(d_x, 4 * sizeof(T)), w_vec = ldw % 4 == 0 && aligned_to(d_w, 16);
        const bool dense = std::is_same<T, float>::value && !d_idx;
        with_one_of<1, 2, 4>(rule.ct, [&](auto CT) {
            constexpr int UT = column_tiles(CT);
            with_vec(x_vec, [&](auto V) {
                auto launch = [&](auto kernel) {
                    hipLaunchKernelGGL(kernel, dim3((unsigned)rule.blocks), dim3(256), (size_t)rule.lds, st, d_x, ldx, n, di, d_idx, n_rows, w_vec,
                                       d_w, ldw, ci, d_bias, d_labels, w, rule.p, rule.rows, d_row_loss, d_pred, part);
                };
                if constexpr (std::is_same<T, float>::value) {
                    if (dense) launch(linear_step_kernel<float, false, V, CT, UT>);
                    else launch(linear_step_kernel<float, true, V, CT, UT>);
                } else {
                    launch(linear_step_kernel<T, true, V, CT, UT>);
                }
            });
        });
        SGL_LAUNCH_CHECK(who);
    }
    return launch_fold(who, st, part, rule.blocks, 1, column_tiles(rule.ct), ci, di, d_dw, lddw, d_db);
}

}  // namespace

SGL_EXPORT int sgl_linear_step_rule(int64_t n, int64_t d, int64_t c, int64_t *out) {
    SGL_REQUIRE(out, "sgl_linear_step_rule: bad arguments");
    SGL_REQUIRE_WIDTH("sgl_linear_step_rule", "d", d);
    StepRule r;
    const int rc = check_step("sgl_linear_step_rule", n, d, c, r);
    if (rc != SGL_OK) return rc;
    out[0] = r.blocks, out[1] = r.rows, out[2] = r.ct, out[3] = r.tu, out[4] = r.lds;
    return SGL_OK;
}

SGL_EXPORT int64_t sgl_linear_step_scratch(int64_t n, int64_t d, int64_t c) {
    StepRule r;
    return check_step("sgl_linear_step_scratch", n, d, c, r) == SGL_OK ? r.blocks * kTableFloats * (int64_t)sizeof(float) : -1;
}

SGL_EXPORT int sgl_linear_step_f32(const float *d_x, int64_t ldx, int64_t n, int64_t d, const float *d_w, int64_t ldw, int64_t c,
                                   const float *d_bias, const int64_t *d_labels, float w, float *d_row_loss, int64_t *d_pred, float *d_dw,
                                   int64_t lddw, float *d_db, void *d_scratch, void *stream) {
    return linear_step("sgl_linear_step_f32", d_x, ldx, n, nullptr, n, d, d_w, ldw, c, d_bias, d_labels, w, d_row_loss, d_pred, d_dw, lddw,
                       d_db, d_scratch, stream);
}

SGL_EXPORT int sgl_linear_step_rows_f32(const float *d_x, int64_t ldx, int64_t n_rows, const int64_t *d_idx, int64_t m, int64_t d,
                                        const float *d_w, int64_t ldw, int64_t c, const float *d_bias, const int64_t *d_labels, float w,
                                        float *d_row_loss, int64_t *d_pred, float *d_dw, int64_t lddw, float *d_db, void *d_scratch,
                                        void *stream) {
    return linear_step("sgl_linear_step_rows_f32", d_x, ldx, n_rows, d_idx, m, d, d_w, ldw, c, d_bias, d_labels, w, d_row_loss, d_pred, d_dw,
                       lddw, d_db, d_scratch, stream);
}

SGL_EXPORT int sgl_linear_step_rows_bf16(const uint16_t *d_x, int64_t ldx, int64_t n_rows, const int64_t *d_idx, int64_t m, int64_t d,
                                         const float *d_w, int64_t ldw, int64_t c, const float *d_bias, const int64_t *d_labels, float w,
                                         float *d_row_loss, int64_t *d_pred, float *d_dw, int64_t lddw, float *d_db, void *d_scratch,
                                         void *stream) {
    return linear_step("sgl_linear_step_rows_bf16", d_x, ldx, n_rows, d_idx, m, d, d_w, ldw, c, d_bias, d_labels, w, d_row_loss, d_pred,
                       d_dw, lddw, d_db, d_scratch, stream);
}
