// K12: the loss of the trainable clustering task and its gradient in ONE pass over the model output -- what
//   dist = cat(norm(out - c_j) for j); loss = (2 sum_i dist[i, y_i] - dist.mean(1).sum()) / n; loss.backward()
// (cluster_loss, sgl/tasks/utils.py:101-113) computes with k passes over the output, k autograd nodes and a Python loop over the rows.
// With D_ij = |x_i - c_j|_2 and y_i the row's k-means label:
//   l_i  = 2 D_{i, y_i} - (1 / k) sum_j D_ij
//   dX_i = w sum_j a_ij (x_i - c_j),   a_ij = (2 [j = y_i] - 1 / k) / D_ij,   a_ij = 0 where D_ij = 0 (torch.norm's subgradient)
// The centres and the labels carry no gradient.
//
// DIRECT form only: the difference x - c is taken first, for the distance and for the gradient (translation-invariant; the expansion
// x sum a - sum a c is not).  Layout: K9's (sgl_kmeans.hip) -- LPR lanes (sgl::slice_instance) own a row and keep their slice of it in
// registers across all k centres, CH vectors of VEC floats, U rows per lane group; next to it the slice of dX, summed in registers.
// The centres are staged NEGATED in LDS tiles of at most 64 KiB; the running sums of the loss and of dX cross the tiles: any k x d.
//
// Every lane needs every centre's distance before it can scale a difference.  Of the two ways -- keep T centres' differences in
// registers, or sweep the LDS tile a second time -- this is the second, T = 4 centres at a time: sweep one forms the T sums of squares
// of the group's U rows (Sq, then group_sum<LPR>: every lane holds all U T), each (row, centre) pair goes to ONE lane of the group, which
// turns its sum into D and a (one sqrt and one IEEE division per U T pairs per wavefront, sgl_rows.h "one hop per lane") and keeps D in
// running sums of its own; the group reads the coefficients back; sweep two re-reads the T centre vectors and adds a (x + (-c)) to the
// dX slice.  x + (-c) has the bits of x - c both times.  Why not the first: the row slice
// and the dX slice already take 2 U CH VEC registers; T differences per row would add T U CH VEC (DESIGN.md K12 lists the counts).
//
// Order of the sums: a distance per lane chunk after chunk (Sq), then group_sum<LPR>; dX_i centre after centre, j ascending (fmaf);
// sum_j D_ij as T partial sums, slot t over the centres j = t mod T ascending, added in slot order at the end (tiles hold whole steps, so
// a centre's slot does not depend on the tile).  None depends on n, on the row's position, on U or on the tile size: only on (d, LPR,
// VEC, k, the centre order).  No atomics, no scratch: two runs are bit-equal.  (Rows beyond the register layouts, d > 2048: one row per wavefront, X and
// the centres re-read through the caches per centre, the dX row kept in the output row the wavefront owns.)
//
// A label outside [0, k) matches no centre: the 2 D term and its gradient are absent, nothing is indexed by a label.  A non-finite
// row gives non-finite results in that row alone.  Nothing traps.  VEC = 4 needs 16-byte aligned bases and pitches that are multiples
// of 4 floats on X, the centres and dX; nothing beyond column d of a last row is read, nothing beyond column d of any row written.
#include "sgl_centres.h"

namespace {

constexpr int kStep = 4;                             // T: centres per step (<= 8, the smallest lane group: one centre per lane)

// acc + a (x + nc), the difference first
template <int VEC>
__device__ __forceinline__ typename Vt<VEC>::type scaled_diff(const float a, const typename Vt<VEC>::type x, const typename Vt<VEC>::type nc,
                                                              typename Vt<VEC>::type acc) {
    if constexpr (VEC == 4) {
        const f2 aa = {a, a};
        acc.lo = __builtin_elementwise_fma(aa, x.lo + nc.lo, acc.lo);
        acc.hi = __builtin_elementwise_fma(aa, x.hi + nc.hi, acc.hi);
        return acc;
    } else {
        return fmaf(a, x + nc, acc);
    }
}

// (D, a) of one centre from its sum of squares: D = sqrt(s), a = (2 [j = y] - 1 / k) / D, 0 where D = 0
__device__ __forceinline__ void dist_coef(const float s, const bool assigned, const float inv_k, float &dist, float &a) {
    dist = sqrtf(s);
    const float wgt = (assigned ? 2.f : 0.f) - inv_k;
    a = dist == 0.f ? 0.f : wgt / dist;
}

struct RowSums {                                     // running sums of one row over the centres seen so far
    float all = 0.f;                                 // sum_j D_ij, j ascending
    float mine = 0.f;                                // D_{i, y_i}; 0 while no centre matched the label
    __device__ __forceinline__ void take(const float dist, const bool assigned) {
        all += dist;
        if (assigned) mine = dist;
    }
    __device__ __forceinline__ float loss(const float inv_k) const { return 2.f * mine - all * inv_k; }
};

template <int LPR, int VEC, int CH, int U>
__global__ __launch_bounds__(256) void cluster_loss_kernel(const float *__restrict__ x, const int64_t ldx, const int64_t n, const int d,
                                                           const float *__restrict__ cen, const int64_t ldc, const int k,
                                                           const int tile_k, const int dp, const int64_t n_batches,
                                                           const int64_t *__restrict__ labels, const float inv_k, const float w,
                                                           float *__restrict__ dx, const int64_t lddx, float *__restrict__ row_loss) {
    using V = typename Vt<VEC>::type;
    extern __shared__ __attribute__((aligned(16))) float tile[];
    constexpr int T = kStep;
    constexpr int PER = U * T < LPR ? U * T : LPR;  // (row, centre) pairs of a step that are finished at once, one per lane
    constexpr int ROUNDS = U * T / PER;
    const int l = threadIdx.x % LPR;
    const int g = threadIdx.x / LPR;
    bool staged = false;
    for (int64_t b = blockIdx.x; b < n_batches; b += gridDim.x) {
        V xr[U][CH], acc[U][CH];
        int y[U];                                    // the label, -1 when it names no centre
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t row = batch_row<LPR, U>(b, u, g);
            const float *p = x + (row < n ? row : 0) * ldx;
            const int64_t label = row < n ? labels[row] : -1;
            y[u] = (label >= 0 && label < k) ? (int)label : -1;
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                const int col = (c * LPR + l) * VEC;
                V v = vzero<VEC>();
                if (row < n && col < d) v = edge_load<VEC>(p, col, d, row == n - 1);
                xr[u][c] = v;
                acc[u][c] = vzero<VEC>();
            }
        }
        RowSums sums[ROUNDS];                        // of the (row, slot) pairs this lane takes: pair r * PER + l in round r
        for (int j0 = 0; j0 < k; j0 += tile_k) {     // (tile_k is a multiple of T unless it is k: centre j is in slot j % T, whatever the tile)
            const int kt = (k - j0 < tile_k) ? k - j0 : tile_k;
            restage_centres<VEC>(staged, tile, cen, ldc, k, j0, kt, tile_k, d, dp);
            for (int jj = 0; jj < kt; jj += T) {     // T centres at a time; slots beyond the tile repeat its last centre and are not taken
                Sq<VEC> sq[U][T];
#pragma unroll
                for (int c = 0; c < CH; ++c) {
                    const int col = (c * LPR + l) * VEC;
                    if (col < d) {
#pragma unroll
                        for (int t = 0; t < T; ++t) {
                            const int jt = jj + t < kt ? jj + t : kt - 1;
                            const V nc = *reinterpret_cast<const V *>(tile + jt * dp + col);
#pragma unroll
                            for (int u = 0; u < U; ++u) sq[u][t].add_negated(xr[u][c], nc);
                        }
                    }
                }
                float s[U][T], a[U][T];
#pragma unroll
                for (int u = 0; u < U; ++u)
#pragma unroll
                    for (int t = 0; t < T; ++t) s[u][t] = group_sum<LPR>(sq[u][t].total());
                // one (row, centre) pair per lane: lane q of the group turns pair r * PER + q = (row u, slot t) into (D, a) -- ONE sqrt and
                // one IEEE division per PER pairs per wavefront -- keeps the pair's D in its own running sums, and the group reads the
                // coefficients back
                const int t_mine = l % T;            // PER is a multiple of T
#pragma unroll
                for (int r = 0; r < ROUNDS; ++r) {
                    float s_mine = s[(r * PER) / T][(r * PER) % T];
                    int y_mine = y[(r * PER) / T];
#pragma unroll
                    for (int q = 1; q < PER; ++q)
                        if (l == q) {
                            s_mine = s[(r * PER + q) / T][(r * PER + q) % T];
                            y_mine = y[(r * PER + q) / T];
                        }
                    const bool assigned = j0 + jj + t_mine == y_mine;
                    float dist_mine, a_mine;
                    dist_coef(s_mine, assigned, inv_k, dist_mine, a_mine);
                    if (jj + t_mine < kt) sums[r].take(dist_mine, assigned);
#pragma unroll
                    for (int q = 0; q < PER; ++q) a[(r * PER + q) / T][(r * PER + q) % T] = from_lane<LPR>(a_mine, q);
                }
                if (dx) {
#pragma unroll
                    for (int c = 0; c < CH; ++c) {
                        const int col = (c * LPR + l) * VEC;
                        if (col < d) {
#pragma unroll
                            for (int t = 0; t < T; ++t) {
                                if (jj + t < kt) {
                                    const V nc = *reinterpret_cast<const V *>(tile + (jj + t) * dp + col);
#pragma unroll
                                    for (int u = 0; u < U; ++u) acc[u][c] = scaled_diff<VEC>(a[u][t], xr[u][c], nc, acc[u][c]);
                                }
                            }
                        }
                    }
                }
            }
        }
        // l_i: the four slots' sums of row u from the lanes that kept them, added in slot order; at most one slot met the label (the
        // others hold 0).  Gathered by every lane before any leaves: a lane group is live or not as a whole, a wavefront is not.
        float loss[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            RowSums whole;
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const int pair = u * T + t;
                whole.all += from_lane<LPR>(sums[pair / PER].all, pair % PER);
                whole.mine += from_lane<LPR>(sums[pair / PER].mine, pair % PER);
            }
            loss[u] = whole.loss(inv_k);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t row = batch_row<LPR, U>(b, u, g);
            if (row < n) {
                if (dx) {
                    float *orow = dx + row * lddx;
#pragma unroll
                    for (int c = 0; c < CH; ++c) {
                        const int col = (c * LPR + l) * VEC;
                        if (col < d) store_cols<VEC>(orow, col, d, acc[u][c] * w);
                    }
                }
                if (row_loss && l == 0) row_loss[row] = loss[u];
            }
        }
    }
}

// rows beyond the register layouts: one row per wavefront, the row and the centres re-read through the caches for every centre (the
// same per-lane order, 64 lanes, group_sum<64>); the dX row is summed in the output row, every lane re-reading what it alone wrote
template <int VEC>
__global__ __launch_bounds__(256) void cluster_loss_stream_kernel(const float *__restrict__ x, const int64_t ldx, const int64_t n, const int d,
                                                                  const float *__restrict__ cen, const int64_t ldc, const int k,
                                                                  const int64_t *__restrict__ labels, const float inv_k, const float w,
                                                                  float *dx, const int64_t lddx, float *__restrict__ row_loss) {
    const int l = threadIdx.x % 64;
    for (int64_t row = (int64_t)blockIdx.x * 4 + threadIdx.x / 64; row < n; row += (int64_t)gridDim.x * 4) {
        const float *p = x + row * ldx;
        float *orow = dx ? dx + row * lddx : nullptr;
        const bool last = row == n - 1;
        const int64_t y = labels[row];
        if (orow)
            for (int col = l * VEC; col < d; col += 64 * VEC) store_cols<VEC>(orow, col, d, vzero<VEC>());
        RowSums sums;
        for (int j = 0; j < k; ++j) {
            const float *crow = cen + (int64_t)j * ldc;
            const bool last_c = j == k - 1;
            Sq<VEC> sq;
            for (int64_t c0 = (int64_t)l * VEC; c0 < d; c0 += (int64_t)kStreamBlock * 64 * VEC) {   // blocks of kStreamBlock chunks (sgl_centres.h)
                const int64_t c1 = min((int64_t)d, c0 + (int64_t)kStreamBlock * 64 * VEC);
                Sq<VEC> part;
                for (int64_t col = c0; col < c1; col += 64 * VEC)
                    part.add(edge_load<VEC>(p, (int)col, d, last), edge_load<VEC>(crow, (int)col, d, last_c));
                sq.merge(part);
            }
            float dist, a;
            dist_coef(group_sum<64>(sq.total()), j == y, inv_k, dist, a);
            sums.take(dist, j == y);
            if (orow)
                for (int col = l * VEC; col < d; col += 64 * VEC)
                    store_cols<VEC>(orow, col, d,
                                    scaled_diff<VEC>(a, edge_load<VEC>(p, col, d, last), -edge_load<VEC>(crow, col, d, last_c), load_cols<VEC>(orow, col, d)));
        }
        if (orow)
            for (int col = l * VEC; col < d; col += 64 * VEC) store_cols<VEC>(orow, col, d, load_cols<VEC>(orow, col, d) * w);
        if (row_loss && l == 0) row_loss[row] = sums.loss(inv_k);
    }
}

constexpr int kMaxBlocks = 2048;                     // 256 CUs x 8 resident workgroups: the batches beyond are strided over

// rows per lane group: as many as keep the row slices AND the dX slices within 64 registers, at most 4
constexpr int rows_per_group(int vec, int ch) { return vec * ch * 8 <= 64 ? 4 : (vec * ch * 4 <= 64 ? 2 : 1); }

template <int LPR, int VEC, int CH>
void launch_loss(hipStream_t st, const float *d_x, int64_t ldx, int64_t n, int d, const float *d_c, int64_t ldc, int k,
                 const int64_t *d_labels, float inv_k, float w, float *d_dx, int64_t lddx, float *d_row_loss) {
    constexpr int U = rows_per_group(VEC, CH);
    const int dp = (d + VEC - 1) / VEC * VEC;
    const int tile_k = k <= kTileFloats / dp ? k : kTileFloats / dp / kStep * kStep;   // whole steps per tile: a centre's slot is j % T
    const sgl::BatchGrid grid = sgl::loss_batch_grid(n, 256 / LPR, U, kMaxBlocks);
    hipLaunchKernelGGL((cluster_loss_kernel<LPR, VEC, CH, U>), dim3((unsigned)grid.blocks), dim3(256), (size_t)tile_k * dp * sizeof(float), st,
                       d_x, ldx, n, d, d_c, ldc, k, tile_k, dp, grid.n_batches, d_labels, inv_k, w, d_dx, lddx, d_row_loss);
}

}  // namespace

SGL_EXPORT int sgl_cluster_loss_grad_f32(const float *d_x, int64_t ldx, int64_t n, int64_t d, const float *d_centres, int64_t ldc, int64_t k,
                                         const int64_t *d_labels, float w, float *d_dx, int64_t lddx, float *d_row_loss, void *stream) {
    const char *who = "sgl_cluster_loss_grad_f32";
    SGL_REQUIRE(n >= 0 && d >= 0 && d < INT32_MAX && k >= 1 && k < INT32_MAX, "%s: bad sizes (n >= 0, d >= 0, k >= 1)", who);
    SGL_REQUIRE_WIDTH(who, "d", d);
    SGL_REQUIRE_WIDTH(who, "k", k);
    // (a matrix without rows or without columns has no storage, no rows have no labels and no losses: such a pointer is never used)
    SGL_REQUIRE(d_dx || d_row_loss || n == 0, "%s: at least one of d_dx and d_row_loss is needed", who);
    SGL_REQUIRE((d_x || n == 0 || d == 0) && (d_centres || d == 0) && (d_labels || n == 0), "%s: NULL arguments", who);
    SGL_REQUIRE(ldx >= d && ldc >= d && (lddx >= d || !d_dx), "%s: row pitch smaller than d", who);
    SGL_REQUIRE(aligned_to(d_x, 4) && aligned_to(d_centres, 4) && aligned_to(d_dx, 4) && aligned_to(d_row_loss, 4) && aligned_to(d_labels, 8),
                "%s: pointers must be aligned to their element size", who);
    if (n == 0) return SGL_OK;
    hipStream_t st = sgl::as_stream(stream);
    if (d == 0) {                                    // empty sums: every distance is 0, so is every l_i; dX has no columns; no kernel
        if (d_row_loss) SGL_HIP_CHECK(hipMemsetAsync(d_row_loss, 0, (size_t)n * sizeof(float), st));
        return SGL_OK;
    }
    const bool vec4 = ldx % 4 == 0 && ldc % 4 == 0 && aligned_to(d_x, 16) && aligned_to(d_centres, 16) &&
                      (!d_dx || (lddx % 4 == 0 && aligned_to(d_dx, 16)));
    const int vec = vec4 ? 4 : 1;
    const sgl::SliceInstance in = sgl::slice_instance(d, vec, sgl::ClusterLossSlices::chunks(vec));
    if (!sgl::launch_fits(kMaxBlocks, 256)) return sgl::fail(SGL_ERR_UNSUPPORTED, "%s: the grid does not fit one launch", who);
    const int di = (int)d, ki = (int)k;
    const float inv_k = 1.f / (float)ki;
    const bool launched = with_slice_instance<sgl::ClusterLossSlices>(in, vec4, [&](auto L, auto V, auto C) {
        launch_loss<L, V, C>(st, d_x, ldx, n, di, d_centres, ldc, ki, d_labels, inv_k, w, d_dx, lddx, d_row_loss);
    });
    if (!launched) {                                 // ch = 0: rows beyond the register layouts
        const int64_t blocks = sgl::loss_grid((n + 3) / 4, kMaxBlocks);
        with_vec(vec4, [&](auto V) {
            hipLaunchKernelGGL((cluster_loss_stream_kernel<V>), dim3((unsigned)blocks), dim3(256), 0, st, d_x, ldx, n, di, d_centres, ldc, ki,
                               d_labels, inv_k, w, d_dx, lddx, d_row_loss);
        });
    }
    SGL_LAUNCH_CHECK(who);
    return SGL_OK;
}
