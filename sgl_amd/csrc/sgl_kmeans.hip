// K9: the assignment step of k-means, labels[i] = argmin_j |x_i - c_j|^2 and that minimum -- what sklearn's KMeans spends its time
// on when NodeClusteringNAFS hands it the NAFS features (sgl/tasks/node_clustering.py:254-255).  One read of X, k distances per row.
//
// The distance is the DIRECT form sum_c (x - c)^2, difference first: translation-invariant (no centring copy of X, which sklearn
// makes only because it expands the square), every term >= 0, relative error (d + 3) 2^-24 whatever the offset of the data.  That
// rules out MFMA (it would need the expanded form) and makes one step compute-balanced: 2 N k d flops against N d x 4 bytes.
//
// Layout.  LPR lanes (sgl::slice_instance) own a row and keep their slice of it in REGISTERS across all k centres: CH vectors of VEC floats
// (vector (c * LPR + l) of the row for lane l, chunk c), U rows per lane group so that one LDS read of a centre vector serves U rows
// (at U = 1 the LDS pipe, shared by the four SIMDs, is the limit: one 16-byte read per four VALU instructions).  The centres are
// staged in LDS in tiles of at most 64 KiB (two workgroups per CU), the pad of a tile zeroed; a running (best, label) per row crosses
// the tiles, so any k x d works.  Workgroups stride over batches of 256 / LPR x U rows; when one tile holds all centres it is staged
// once per workgroup, not once per batch.
//
// Summation order of one distance: per lane chunk after chunk -- VEC = 4: two accumulators, (elements 0, 1) then (elements 2, 3) of a
// vector as packed fma, added at the end; VEC = 1: one accumulator -- then the lanes of the group: across the 16-lane rows first
// (lane ^ 32, lane ^ 16: reduce_slots below), then group_sum<16> inside a row.  It depends on (d, LPR, VEC) alone: not on n, k, the
// tile size, U or the position of the row or the centre.  (The streaming kernel for rows beyond the register layouts, d > 2048, sums
// its 64 lanes with group_sum<64>: no width is served by both.)
//
// Ties: centres are visited in ascending order and only `<` replaces the best, so the lowest index wins (numpy's argmin).  A NaN
// distance never wins; a row whose k distances are ALL NaN (a NaN in the row) gets label 0 and mindist NaN.  Nothing traps.
// VEC = 4 needs 16-byte aligned bases and pitches that are multiples of 4 floats on both matrices; pads are zeroed before use and
// nothing beyond column d of a LAST row is read (edge_load).
#include "sgl_centres.h"   // Sq, restage_centres, kTileFloats: shared with sgl_cluster_loss.hip (K12)

namespace {

struct Best {                                        // running minimum of one row over the centres seen so far
    float dist = __builtin_inff();
    int label = 0;
    bool all_nan = true;
    __device__ __forceinline__ void take(const float s, const int j) {
        if (s < dist) {
            dist = s;
            label = j;
        }
        all_nan = all_nan && (s != s);
    }
    __device__ __forceinline__ float min_dist() const { return all_nan ? __uint_as_float(0x7fc00000u) : dist; }
};

// ---- transposing reduction ------------------------------------------------------------------------------------------------------------
// group_sum per (row, centre) costs 6 - 8 VALU instructions at LPR = 32 / 64 and leaves every lane with the same total: more than the
// 4 packed instructions a lane spends on a vector of the distance itself (measured: 13 x one read of X at d = 100).  So a lane group
// takes T centres at a time (T = 4 at LPR = 64, 2 at LPR = 32) and the steps that cross the 16-lane rows TRANSPOSE: v_permlane32_swap /
// v_permlane16_swap exchange one half of the T partial sums for the other, after which each row of 16 lanes holds the sums of ONE of
// the T centres (slot_of_lane) and finishes them with the DPP steps of group_sum<16>.  T - 1 swaps and adds plus 4 DPP adds for T
// centres, and the running minimum is compared once per T centres per lane; the rows' minima are merged once per row of X
// (merge_rows).  Every partial sum goes through the same (low half + high half, even row + odd row) additions whatever its slot, so
// the bits of a distance do not depend on where its centre stands.
template <int LPR>
constexpr int kSlots = LPR == 64 ? 4 : (LPR == 32 ? 2 : 1);

template <int LPR>
__device__ __forceinline__ int slot_of_lane() {      // the slot whose total reduce_slots leaves in this lane
    const int row = (threadIdx.x % 64) / 16;
    if constexpr (LPR == 64) return ((row & 1) << 1) | (row >> 1);
    if constexpr (LPR == 32) return row & 1;
    return 0;
}

__device__ __forceinline__ float swap_add32(const float a, const float b) {   // lanes 0-31: a + a[lane ^ 32], lanes 32-63: b + b[lane ^ 32]
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
__device__ __forceinline__ float swap_add16(const float a, const float b) {   // even rows: a + a[lane ^ 16], odd rows: b + b[lane ^ 16]
    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

template <int LPR>
__device__ __forceinline__ float reduce_slots(const float (&p)[kSlots<LPR>]) {
    if constexpr (LPR == 64) return group_sum<16>(swap_add16(swap_add32(p[0], p[1]), swap_add32(p[2], p[3])));
    else if constexpr (LPR == 32) return group_sum<16>(swap_add16(p[0], p[1]));
    else return group_sum<LPR>(p[0]);
}

// the minimum over the rows of a lane group: each holds the best of other centres, so equal distances have different labels
template <int LPR>
__device__ __forceinline__ void merge_rows(Best &b) {
    auto step = [&](auto swap) {
        const auto dd = swap(__float_as_uint(b.dist)), ll = swap((unsigned)b.label), nn = swap((unsigned)b.all_nan);
        const float d0 = __uint_as_float(dd[0]), d1 = __uint_as_float(dd[1]);
        const bool first = d0 < d1 || (d0 == d1 && (int)ll[0] < (int)ll[1]);
        b.dist = first ? d0 : d1;
        b.label = (int)(first ? ll[0] : ll[1]);
        b.all_nan = nn[0] && nn[1];
    };
    if constexpr (LPR == 64) step([](unsigned v) { return __builtin_amdgcn_permlane32_swap(v, v, false, false); });
    if constexpr (LPR >= 32) step([](unsigned v) { return __builtin_amdgcn_permlane16_swap(v, v, false, false); });
}

template <int LPR, int VEC, int CH, int U>
__global__ __launch_bounds__(256) void kmeans_assign_kernel(const float *__restrict__ x, const int64_t ldx, const int64_t n, const int d,
                                                            const float *__restrict__ cen, const int64_t ldc, const int k,
                                                            const int tile_k, const int dp, const int64_t n_batches,
                                                            int64_t *__restrict__ labels, float *__restrict__ mindist) {
    using V = typename Vt<VEC>::type;
    extern __shared__ __attribute__((aligned(16))) float tile[];
    constexpr int T = kSlots<LPR>;                   // centres per step of the transposing reduction
    const int l = threadIdx.x % LPR;
    const int g = threadIdx.x / LPR;
    bool staged = false;
    for (int64_t b = blockIdx.x; b < n_batches; b += gridDim.x) {
        V xr[U][CH];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t row = batch_row<LPR, U>(b, u, g);
            const float *p = x + (row < n ? row : 0) * ldx;
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                const int col = (c * LPR + l) * VEC;
                V v = vzero<VEC>();
                if (row < n && col < d) v = edge_load<VEC>(p, col, d, row == n - 1);
                xr[u][c] = v;
            }
        }
        Best best[U];
        for (int j0 = 0; j0 < k; j0 += tile_k) {
            const int kt = (k - j0 < tile_k) ? k - j0 : tile_k;
            restage_centres<VEC>(staged, tile, cen, ldc, k, j0, kt, tile_k, d, dp);
            for (int jj = 0; jj < kt; jj += T) {     // T centres at a time; slots beyond the tile repeat its last centre and are not taken
                Sq<VEC> acc[U][T];
#pragma unroll
                for (int c = 0; c < CH; ++c) {
                    const int col = (c * LPR + l) * VEC;
                    if (col < d) {
#pragma unroll
                        for (int t = 0; t < T; ++t) {
                            const int jt = jj + t < kt ? jj + t : kt - 1;
                            const V nc = *reinterpret_cast<const V *>(tile + jt * dp + col);
#pragma unroll
                            for (int u = 0; u < U; ++u) acc[u][t].add_negated(xr[u][c], nc);
                        }
                    }
                }
                const int mine = jj + slot_of_lane<LPR>();
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    float part[T];
#pragma unroll
                    for (int t = 0; t < T; ++t) part[t] = acc[u][t].total();
                    const float s = reduce_slots<LPR>(part);
                    if (mine < kt) best[u].take(s, j0 + mine);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) merge_rows<LPR>(best[u]);
        if (l == 0) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t row = batch_row<LPR, U>(b, u, g);
                if (row < n) {
                    labels[row] = best[u].label;
                    if (mindist) mindist[row] = best[u].min_dist();
                }
            }
        }
    }
}

// rows beyond the register layouts: one row per wavefront, the row and the centres re-read through the caches for every centre;
// the same per-lane order (chunk after chunk, 64 lanes) and the same group_sum
template <int VEC>
__global__ __launch_bounds__(256) void kmeans_assign_stream_kernel(const float *__restrict__ x, const int64_t ldx, const int64_t n,
                                                                   const int d, const float *__restrict__ cen, const int64_t ldc,
                                                                   const int k, int64_t *__restrict__ labels,
                                                                   float *__restrict__ mindist) {
    const int l = threadIdx.x % 64;
    for (int64_t row = (int64_t)blockIdx.x * 4 + threadIdx.x / 64; row < n; row += (int64_t)gridDim.x * 4) {
        const float *p = x + row * ldx;
        Best best;
        for (int j = 0; j < k; ++j) {
            const float *crow = cen + (int64_t)j * ldc;
            Sq<VEC> acc;
            for (int64_t c0 = (int64_t)l * VEC; c0 < d; c0 += (int64_t)kStreamBlock * 64 * VEC) {   // blocks of kStreamBlock chunks (sgl_centres.h)
                const int64_t c1 = min((int64_t)d, c0 + (int64_t)kStreamBlock * 64 * VEC);
                Sq<VEC> part;
                for (int64_t col = c0; col < c1; col += 64 * VEC)
                    part.add(edge_load<VEC>(p, (int)col, d, row == n - 1), edge_load<VEC>(crow, (int)col, d, j == k - 1));
                acc.merge(part);
            }
            best.take(group_sum<64>(acc.total()), j);
        }
        if (l == 0) {
            labels[row] = best.label;
            if (mindist) mindist[row] = best.min_dist();
        }
    }
}

constexpr int kMaxBlocks = 2048;                     // 256 CUs x 8 resident workgroups: the batches beyond are strided over

// rows per lane group: as many as keep the row slices within 64 registers, at most 4
constexpr int rows_per_group(int vec, int ch) { return vec * ch * 4 <= 64 ? 4 : (vec * ch * 2 <= 64 ? 2 : 1); }

template <int LPR, int VEC, int CH>
void launch_assign(hipStream_t st, const float *d_x, int64_t ldx, int64_t n, int d, const float *d_c, int64_t ldc, int k,
                   int64_t *d_labels, float *d_mindist) {
    constexpr int U = rows_per_group(VEC, CH);
    const int dp = (d + VEC - 1) / VEC * VEC;
    const int tile_k = k < kTileFloats / dp ? k : kTileFloats / dp;
    const sgl::BatchGrid grid = sgl::loss_batch_grid(n, 256 / LPR, U, kMaxBlocks);
    hipLaunchKernelGGL((kmeans_assign_kernel<LPR, VEC, CH, U>), dim3((unsigned)grid.blocks), dim3(256), (size_t)tile_k * dp * sizeof(float), st,
                       d_x, ldx, n, d, d_c, ldc, k, tile_k, dp, grid.n_batches, d_labels, d_mindist);
}

}  // namespace

SGL_EXPORT int sgl_kmeans_assign_f32(const float *d_x, int64_t ldx, int64_t n, int64_t d, const float *d_centres, int64_t ldc, int64_t k,
                                     int64_t *d_labels, float *d_mindist, void *stream) {
    SGL_REQUIRE(n >= 0 && d >= 0 && d < INT32_MAX && k >= 0 && k < INT32_MAX && (k >= 1 || n == 0), "sgl_kmeans_assign_f32: bad sizes");
    SGL_REQUIRE_WIDTH("sgl_kmeans_assign_f32", "d", d);
    SGL_REQUIRE_WIDTH("sgl_kmeans_assign_f32", "k", k);
    // (a matrix without rows or without columns has no storage, no rows have no labels: such a pointer is never used)
    SGL_REQUIRE((d_x || n == 0 || d == 0) && (d_centres || k == 0 || d == 0) && (d_labels || n == 0), "sgl_kmeans_assign_f32: NULL arguments");
    SGL_REQUIRE(ldx >= d && ldc >= d, "sgl_kmeans_assign_f32: row pitch smaller than d");
    SGL_REQUIRE(aligned_to(d_x, 4) && aligned_to(d_centres, 4) && aligned_to(d_mindist, 4) && aligned_to(d_labels, 8),
                "sgl_kmeans_assign_f32: pointers must be aligned to their element size");
    if (n == 0) return SGL_OK;
    hipStream_t st = sgl::as_stream(stream);
    if (d == 0) {                                    // empty sums: every distance is 0, centre 0 wins; no kernel
        SGL_HIP_CHECK(hipMemsetAsync(d_labels, 0, (size_t)n * sizeof(int64_t), st));
        if (d_mindist) SGL_HIP_CHECK(hipMemsetAsync(d_mindist, 0, (size_t)n * sizeof(float), st));
        return SGL_OK;
    }
    const bool vec4 = ldx % 4 == 0 && ldc % 4 == 0 && aligned_to(d_x, 16) && aligned_to(d_centres, 16);
    const int vec = vec4 ? 4 : 1;
    const sgl::SliceInstance in = sgl::slice_instance(d, vec, sgl::KmeansSlices::chunks(vec));
    if (!sgl::launch_fits(kMaxBlocks, 256)) return sgl::fail(SGL_ERR_UNSUPPORTED, "sgl_kmeans_assign_f32: the grid does not fit one launch");
    const int di = (int)d, ki = (int)k;
    const bool launched = with_slice_instance<sgl::KmeansSlices>(
        in, vec4, [&](auto L, auto V, auto C) { launch_assign<L, V, C>(st, d_x, ldx, n, di, d_centres, ldc, ki, d_labels, d_mindist); });
    if (!launched) {                                 // ch = 0: rows beyond the register layouts
        const int64_t blocks = sgl::loss_grid((n + 3) / 4, kMaxBlocks);
        with_vec(vec4, [&](auto V) {
            hipLaunchKernelGGL((kmeans_assign_stream_kernel<V>), dim3((unsigned)blocks), dim3(256), 0, st, d_x, ldx, n, di, d_centres, ldc, ki,
                               d_labels, d_mindist);
        });
    }
    SGL_LAUNCH_CHECK("sgl_kmeans_assign_f32");
    return SGL_OK;
}
