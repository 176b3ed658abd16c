// K18: the k-means assignment step on the matrix cores (include/sgl_kmeans_mfma.h states the contract).  K9 (sgl_kmeans.hip) sums
// (x - c)^2 on the VALU and is bound by it; here the SEARCH for the nearest centre runs in the centred expanded form
// |c'|^2 - 2 <c', x'> (c' = c - shift, x' = x - shift) on v_mfma_f32_32x32x2_f32, and the returned distance is the direct form for the
// one centre that won.
//
// Operand roles.  D[j][i] = sum_col c'[j][col] x'[i][col]: centres are the A operand (the 32 rows of the tile), rows of X the B operand
// (its 32 columns).  In the 32 x 32 accumulator lane (i = lane % 32, h = lane / 32) then holds ONE row i of X against the 16 centres
// 8 (v / 4) + 4 h + v % 4 (v = 0 .. 15) of the tile: the running (best score, label) over the centres is a per-lane compare and
// select, with no cross-lane step per centre.  The two halves of the wavefront hold disjoint centre sets and merge ONCE per row of X
// (v_permlane32_swap, the rule of K9's merge_rows: the lower score, the lower index among equal ones; a NaN score is never taken).
//
// Columns without a transpose.  A dot product does not care about the order of its terms, so lane (i, h) takes the float4 at columns
// 8 q + 4 h .. 8 q + 4 h + 3 of ITS row, q = 0, 1, ..., and element e of that vector is step 4 q + e of the MFMA chain (the k index of
// an instruction is h).  The centres use the same mapping from LDS: both operands are plain 16-byte row-major reads.  Columns >= d,
// rows >= n and centre slots >= k are zero in the operands; the pads of the caller's buffers never reach an MFMA.
//
// Work split.  256 threads; a wavefront owns R tiles of 32 rows of X (R = 2 up to 4 centre tiles, else 1) and keeps NT = ceil(k / 32)
// accumulator tiles per row tile resident (16 registers each; the compiled NT: sgl::KmeansMatrixTiles).  X streams through registers
// once, 32 columns (four float4 per lane: a row's whole 128-byte line) per step, the shift subtracted on load.  Workgroups stride over
// batches of 4 R x 32 rows (sgl::loss_batch_grid, K9's cap).
//
// Centres in LDS.  Centred at staging time, fl(c - shift), one wavefront per centre row, which also sums |c'_j|^2 in float32 (a
// lane's columns in order, then group_sum<64>).  All columns at once while k rows fit kTileFloats beside the shift and the norms; else
// column chunks of W columns (a multiple of 8) with the accumulators carried across the chunks between barriers, and the norms added
// chunk by chunk.  Row pitch W + 4 floats: (W + 4) / 4 is odd, so the 16-byte reads of 16 consecutive centres (lane i at i * pitch)
// fall into 16 different 16-byte bank groups: free of bank conflicts.
#include "sgl_centres.h"   // kTileFloats; edge_load, group_sum: sgl_rows.h

#include "../../include/sgl_kmeans_mfma.h"

namespace {

using f16v = float __attribute__((ext_vector_type(16)));

constexpr int kMaxBlocks = 2048;                     // K9's cap: 256 CUs x 8 resident workgroups, the batches beyond are strided over
constexpr int kPitchPad = 4;                         // floats: makes pitch / 4 odd
constexpr int kStep = 32;                            // columns of X a lane pair takes per step: 4 vectors in each half

constexpr int row_tiles(int nt) { return nt <= 4 ? 2 : 1; }   // R: 2 x NT x 16 accumulator registers stay within 128

struct MatrixRule {
    int nt, r, w, p;     // centre tiles, row tiles per wavefront, columns staged at once, LDS pitch
};
bool matrix_rule(int64_t d, int64_t k, MatrixRule &out) {
    const sgl::ChunkList tiles = sgl::KmeansMatrixTiles::list();
    const int64_t need = (k + 31) / 32;
    int nt = 0;
    for (int t = tiles.count - 1; t >= 0; --t)
        if (tiles.values[t] >= need) nt = tiles.values[t];
    if (!nt) return false;
    const int64_t dp = (d + 7) / 8 * 8, budget = kTileFloats - nt * 32;
    int64_t w = dp;
    if (k * (dp + kPitchPad) + dp > budget) w = (budget - kPitchPad * k) / (k + 1) / 8 * 8;
    out = {nt, row_tiles(nt), (int)w, (int)w + kPitchPad};
    return true;
}

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

// columns c0 .. c0 + wc - 1 of the k centres, centred, into the tile; the shift of those columns; |c'_j|^2 (started at chunk 0, added
// to after it); zeros from column d on and in the norm slots beyond k
template <int VEC, int NT>
__device__ __forceinline__ void stage_centred(float *__restrict__ tile, float *__restrict__ sh, float *__restrict__ norm,
                                              const float *__restrict__ cen, const int64_t ldc, const int k,
                                              const float *__restrict__ shift, const int d, const int c0, const int wc, const int p) {
    const int lane = threadIdx.x % 64;
    for (int c = threadIdx.x; c < wc; c += 256) sh[c] = (shift && c0 + c < d) ? shift[c0 + c] : 0.f;
    for (int j = k + threadIdx.x; j < NT * 32; j += 256) norm[j] = 0.f;
    for (int j = threadIdx.x / 64; j < k; j += 4) {
        const float *crow = cen + (int64_t)j * ldc;
        float s = 0.f;
        for (int lc = lane * 4; lc < wc; lc += 256) {
            const int col = c0 + lc;
            f4 v = {0.f, 0.f, 0.f, 0.f};
            if (col < d) {
                f4 sv;
#pragma unroll
                for (int e = 0; e < 4; ++e) sv[e] = (shift && col + e < d) ? shift[col + e] : 0.f;
                v = load4<VEC>(crow, col, d, j == k - 1) - sv;
            }
            *reinterpret_cast<f4 *>(tile + j * p + lc) = v;
#pragma unroll
            for (int e = 0; e < 4; ++e) s = fmaf(v[e], v[e], s);
        }
        s = group_sum<64>(s);
        if (lane == 0) norm[j] = (c0 == 0 ? 0.f : norm[j]) + s;
    }
}

template <int VEC, int NT, int R>
__global__ __launch_bounds__(256) void kmeans_matrix_kernel(const float *__restrict__ x, const int64_t ldx, const int64_t n, const int d,
                                                            const float *__restrict__ cen, const int64_t ldc, const int k,
                                                            const float *__restrict__ shift, const int w, const int p,
                                                            const int64_t n_batches, int64_t *__restrict__ labels,
                                                            float *__restrict__ mindist) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *tile = lds, *sh = lds + k * p, *norm = sh + w;
    const int lane = threadIdx.x % 64, i = lane % 32, h = lane / 32, wave = threadIdx.x / 64;
    const bool one_chunk = w >= d;
    bool staged = false;
    for (int64_t b = blockIdx.x; b < n_batches; b += gridDim.x) {
        bool live[R], last[R];
        const float *xp[R];
        f16v acc[R][NT];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int64_t row = (b * 4 * R + wave * R + r) * 32 + i;
            live[r] = row < n;
            const int64_t from = live[r] ? row : 0;  // a tile row beyond the matrix reads row 0 (the epilogue) and writes nothing
            last[r] = from == n - 1;
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
                stage_centred<VEC, NT>(tile, sh, norm, cen, ldc, k, shift, d, c0, wc, p);
                __syncthreads();
                staged = true;
            }
            for (int q0 = 0; q0 < wc; q0 += kStep) {
                f4 xr[R][4];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int lc = q0 + 8 * t + 4 * h, col = c0 + lc;
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        f4 v = {0.f, 0.f, 0.f, 0.f};
                        if (q0 + 8 * t < wc && live[r] && col < d) v = load4<VEC>(xp[r], col, d, last[r]) - *reinterpret_cast<const f4 *>(sh + lc);
                        xr[r][t] = v;
                    }
                }
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    if (q0 + 8 * t < wc) {           // the same for every lane
                        const int lc = q0 + 8 * t + 4 * h;
#pragma unroll
                        for (int ct = 0; ct < NT; ++ct) {
                            const int j = ct * 32 + i;
                            f4 a = *reinterpret_cast<const f4 *>(tile + (j < k ? j : k - 1) * p + lc);
                            if (j >= k) a = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                            for (int e = 0; e < 4; ++e)
#pragma unroll
                                for (int r = 0; r < R; ++r) acc[r][ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], xr[r][t][e], acc[r][ct], 0, 0, 0);
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            float best = __builtin_inff();
            int label = 0;
#pragma unroll
            for (int ct = 0; ct < NT; ++ct)
#pragma unroll
                for (int g = 0; g < 4; ++g) {        // this lane's centres in ascending order: only `<` replaces the best
                    const int j0 = ct * 32 + 8 * g + 4 * h;
                    const f4 nn = *reinterpret_cast<const f4 *>(norm + j0);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float s = fmaf(-2.f, acc[r][ct][4 * g + e], nn[e]);
                        if (j0 + e < k && s < best) {
                            best = s;
                            label = j0 + e;
                        }
                    }
                }
            {                                        // the other half's centres: result [0] is half 0's value in both halves, [1] half 1's
                const auto ss = __builtin_amdgcn_permlane32_swap(__float_as_uint(best), __float_as_uint(best), false, false);
                const auto ll = __builtin_amdgcn_permlane32_swap((unsigned)label, (unsigned)label, false, false);
                const float s0 = __uint_as_float(ss[0]), s1 = __uint_as_float(ss[1]);
                const bool first = s0 < s1 || (s0 == s1 && (int)ll[0] < (int)ll[1]);
                label = (int)(first ? ll[0] : ll[1]);
            }
            const int64_t row = (b * 4 * R + wave * R + r) * 32 + i;
            if (live[r] && h == 0) labels[row] = label;
            if (mindist) {                           // the direct form for the winner, uncentred: this half's vectors, then the halves
                const float *crow = cen + (int64_t)label * ldc;
                float a[4] = {0.f, 0.f, 0.f, 0.f};
                for (int col = 4 * h; col < d; col += 8) {
                    const f4 dv = load4<VEC>(xp[r], col, d, last[r]) - load4<VEC>(crow, col, d, label == k - 1);
#pragma unroll
                    for (int e = 0; e < 4; ++e) a[e] = fmaf(dv[e], dv[e], a[e]);
                }
                const float half = (a[0] + a[1]) + (a[2] + a[3]);
                const auto hh = __builtin_amdgcn_permlane32_swap(__float_as_uint(half), __float_as_uint(half), false, false);
                const float total = __uint_as_float(hh[0]) + __uint_as_float(hh[1]);
                if (live[r] && h == 0) mindist[row] = total;
            }
        }
    }
}

template <int VEC, int NT>
void launch_matrix(hipStream_t st, const MatrixRule &rule, const float *d_x, int64_t ldx, int64_t n, int d, const float *d_c, int64_t ldc,
                   int k, const float *d_shift, int64_t *d_labels, float *d_mindist) {
    constexpr int R = row_tiles(NT);
    const sgl::BatchGrid grid = sgl::loss_batch_grid(n, 4, R * 32, kMaxBlocks);
    const size_t lds = ((size_t)k * rule.p + rule.w + NT * 32) * sizeof(float);
    hipLaunchKernelGGL((kmeans_matrix_kernel<VEC, NT, R>), dim3((unsigned)grid.blocks), dim3(256), lds, st, d_x, ldx, n, d, d_c, ldc, k,
                       d_shift, rule.w, rule.p, grid.n_batches, d_labels, d_mindist);
}

}  // namespace

SGL_EXPORT int sgl_kmeans_assign_matrix_rule(int64_t d, int64_t k, int vec4, int rule[4]) {
    SGL_REQUIRE(rule, "sgl_kmeans_assign_matrix_rule: NULL arguments");
    SGL_REQUIRE(d >= 0 && d < INT32_MAX && k >= 0 && k < INT32_MAX && (vec4 == 0 || vec4 == 1), "sgl_kmeans_assign_matrix_rule: bad sizes");
    SGL_REQUIRE_WIDTH("sgl_kmeans_assign_matrix_rule", "d", d);
    MatrixRule r;
    if (!matrix_rule(d, k, r))
        return sgl::fail(SGL_ERR_UNSUPPORTED, "sgl_kmeans_assign_matrix_rule: k=%lld is beyond the compiled range (k <= %d)", (long long)k,
                         SGL_KMEANS_MATRIX_MAX_K);
    rule[0] = r.nt, rule[1] = r.r, rule[2] = r.w, rule[3] = r.p;
    return SGL_OK;
}

SGL_EXPORT int sgl_kmeans_assign_matrix_f32(const float *d_x, int64_t ldx, int64_t n, int64_t d, const float *d_centres, int64_t ldc,
                                            int64_t k, const float *d_shift, int64_t *d_labels, float *d_mindist, void *stream) {
    SGL_REQUIRE(n >= 0 && d >= 0 && d < INT32_MAX && k >= 0 && k < INT32_MAX && (k >= 1 || n == 0), "sgl_kmeans_assign_matrix_f32: bad sizes");
    SGL_REQUIRE_WIDTH("sgl_kmeans_assign_matrix_f32", "d", d);
    SGL_REQUIRE((d_x || n == 0 || d == 0) && (d_centres || k == 0 || d == 0) && (d_labels || n == 0), "sgl_kmeans_assign_matrix_f32: NULL arguments");
    SGL_REQUIRE(ldx >= d && ldc >= d, "sgl_kmeans_assign_matrix_f32: row pitch smaller than d");
    SGL_REQUIRE(aligned_to(d_x, 4) && aligned_to(d_centres, 4) && aligned_to(d_shift, 4) && aligned_to(d_mindist, 4) && aligned_to(d_labels, 8),
                "sgl_kmeans_assign_matrix_f32: pointers must be aligned to their element size");
    MatrixRule rule;
    if (!matrix_rule(d, k, rule))
        return sgl::fail(SGL_ERR_UNSUPPORTED, "sgl_kmeans_assign_matrix_f32: k=%lld is beyond the compiled range (k <= %d)", (long long)k,
                         SGL_KMEANS_MATRIX_MAX_K);
    if (n == 0) return SGL_OK;
    hipStream_t st = sgl::as_stream(stream);
    if (d == 0) {                                    // empty sums: every distance is 0, centre 0 wins; no kernel
        SGL_HIP_CHECK(hipMemsetAsync(d_labels, 0, (size_t)n * sizeof(int64_t), st));
        if (d_mindist) SGL_HIP_CHECK(hipMemsetAsync(d_mindist, 0, (size_t)n * sizeof(float), st));
        return SGL_OK;
    }
    const bool vec4 = ldx % 4 == 0 && ldc % 4 == 0 && aligned_to(d_x, 16) && aligned_to(d_centres, 16);
    if (!sgl::launch_fits(kMaxBlocks, 256)) return sgl::fail(SGL_ERR_UNSUPPORTED, "sgl_kmeans_assign_matrix_f32: the grid does not fit one launch");
    const int di = (int)d, ki = (int)k;
    with_chunks(sgl::KmeansMatrixTiles{}, rule.nt, [&](auto N) {
        with_vec(vec4, [&](auto V) { launch_matrix<V, N>(st, rule, d_x, ldx, n, di, d_centres, ldc, ki, d_shift, d_labels, d_mindist); });
    });
    SGL_LAUNCH_CHECK("sgl_kmeans_assign_matrix_f32");
    return SGL_OK;
}
