// K20: greedy k-means++ seeding, two launches per step (include/sgl_kmeans_seed.h states the contract).  The torch seeding costs a
// read of X and about ten N-sized passes per step -- a float64 cumsum, a searchsorted, a gather, an assignment that writes N labels
// nobody reads, a minimum -- and L candidates per step would cost L reads of X.  Here the L candidate rows sit in LDS, so a step
// reads X once whatever L is.
//
// seed_step.  Block b owns rows b R .. b R + R - 1.  The rows are laid over the lanes as in K9 (sgl_kmeans.hip): LPR lanes keep a row
// in CH vectors of 4 floats, U rows per lane group, and the distance to T = kSlots<LPR> candidates at a time goes through K9's
// transposing lane sum (reduce_slots, sgl_centres.h), after which the 16-lane row `slot_of_lane` holds the total of one candidate:
// its first lane takes the minimum with the row's running distance and stores it.  The instance is ALWAYS the one K9 picks for
// 16-byte lanes, so the bits of a distance are K9's; a matrix whose rows are no 16-byte vectors (VEC16 = false) is read one float at
// a time into the same registers.  Rows beyond the register layouts (d > 2048) take one wavefront each and K9's streaming order
// (blocks of kStreamBlock chunks, group_sum<64>), with the candidates staged in column chunks and the L partial sums of a row in
// registers across them.
//
// After a barrier the block reads its own R x L minima back (they are in its CU's cache) and sums them in float64 in an order that
// depends on its row count alone (block_potentials): the lane layout, which depends on d, leaves no trace in P.
//
// seed_pick.  Sequential float64 sums over at most 2048 blocks and, per draw, over the R rows of one block, by one thread each, over
// values the whole workgroup staged in LDS.  Its last launch has further workgroups that copy trial[best] to near.
#include "sgl_centres.h"   // Sq, reduce_slots, slot_of_lane, kStreamBlock; sgl_rows.h: edge_load, group_sum, nan_min, with_chunks

#include "../../include/sgl_kmeans_seed.h"

namespace {

constexpr int kMaxTrials = SGL_KMEANS_SEED_MAX_TRIALS;
constexpr int kBudgetWords = 16384;                  // LDS of a workgroup: 64 KiB
constexpr int kMaxBlocks = 2048;                     // row blocks: 256 CUs x 8
constexpr int kMinRows = 256;                        // R >= 256: staging L <= 8 rows per block re-reads at most 3 % of X
constexpr int kWideRows = 2;                         // rows per wavefront of the streaming kernel
constexpr int kCopyBlocks = 1024;                    // workgroups of the last pick, which copy trial[best] to near
constexpr int kPickTile = 256;                       // blocks of P (x kMaxTrials float64) the pick stages in LDS at a time
constexpr int kPickRows = 512;                       // rows of a draw's block (x kMaxTrials draws) it stages at a time: the same 16 KiB
static_assert(kMaxTrials * (kPickRows + 1) <= 2 * (kPickTile + 1) * kMaxTrials, "the staged rows fit the staged potentials' buffer");

struct SeedRule {
    int64_t blocks, rows;                            // B, R
    int chunk, chunks;                               // columns of the candidates staged at a time, W; ceil(dp / W)
    int64_t lds;                                     // bytes of a seed_step workgroup
};
void seed_rule(int64_t n, int64_t d, int trials, SeedRule &out) {
    const int64_t dp = (d + 3) / 4 * 4;
    const int64_t chunk = trials * dp <= kBudgetWords ? dp : kBudgetWords / trials / 256 * 256;
    const int64_t tile = trials * chunk * (int64_t)sizeof(float), sums = trials * 256 * (int64_t)sizeof(double);
    out = {0, 0, (int)chunk, chunk ? (int)((dp + chunk - 1) / chunk) : 0, tile > sums ? tile : sums};
    if (n == 0) return;
    const int64_t forced = sgl::tuning("loss_blocks", 0);
    if (forced > 0) {
        const int64_t want = forced < kMaxBlocks ? (forced < n ? forced : n) : (n < kMaxBlocks ? n : kMaxBlocks);
        out.rows = (n + want - 1) / want;
    } else {
        const int64_t spread = (n + kMaxBlocks - 1) / kMaxBlocks;
        out.rows = spread > kMinRows ? spread : kMinRows;
    }
    out.blocks = (n + out.rows - 1) / out.rows;
}

// the scratch, in this order (the header states it)
constexpr int64_t kPotBytes = (int64_t)kMaxBlocks * kMaxTrials * sizeof(double), kCandBytes = kMaxTrials * sizeof(int64_t), kBestBytes = 16;
int64_t table_bytes(int64_t n, int trials) { return ((int64_t)trials * n * (int64_t)sizeof(float) + 15) / 16 * 16; }

struct StepArgs {
    const float *x;
    int64_t ldx, n;
    int d, trials;                                   // trials: candidates of THIS step, L
    int first;                                       // step 0: the candidate is first_row(draws[0]), the running distance +inf
    const int64_t *cand;
    const double *draws;
    const float *prev;                               // the previous step's trial table, [L_prev][n]
    const int *best_prev;
    float *trial;                                    // [L][n]; read back by block_potentials: no __restrict__, no const
    double *pot;                                     // P: [B][kMaxTrials]
    int64_t rows;                                    // R
    int chunk;                                       // W
};

__device__ __forceinline__ int64_t clamp_row(const int64_t r, const int64_t n) { return r < 0 ? 0 : (r < n - 1 ? r : n - 1); }
__device__ __forceinline__ int64_t first_row(const double u, const int64_t n) { return clamp_row((int64_t)(u * (double)n), n); }
__device__ __forceinline__ int64_t cand_row(const StepArgs &a, const int l) { return a.first ? first_row(a.draws[0], a.n) : clamp_row(a.cand[l], a.n); }
__device__ __forceinline__ bool finite(const float v) { return fabsf(v) < __builtin_inff(); }

// columns col .. col + 3 of a row, zeros from column d on; never beyond column d of the last row, never a 16-byte access without VEC16
template <bool VEC16>
__device__ __forceinline__ f4 row_vec(const float *__restrict__ p, const int col, const int d, const bool last_row) {
    if constexpr (VEC16) return edge_load<4>(p, col, d, last_row);
    f4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = (col + e < d) ? p[col + e] : 0.f;
    return v;
}

// columns c0 .. c0 + w - 1 of the L candidate rows, NEGATED (Sq::add_negated), into the tile (pitch `chunk`), the pad zeroed: one
// wavefront per candidate, as stage_centres does
template <bool VEC16>
__device__ __forceinline__ void stage_candidates(float *__restrict__ tile, const StepArgs &a, const int c0, const int w) {
    const int lane = threadIdx.x % 64;
    for (int l = threadIdx.x / 64; l < a.trials; l += 4) {
        const int64_t id = cand_row(a, l);
        const float *p = a.x + id * a.ldx;
        for (int col = lane * 4; col < w; col += 256)
            *reinterpret_cast<f4 *>(tile + l * a.chunk + col) = -row_vec<VEC16>(p, c0 + col, a.d, id == a.n - 1);
    }
}

// P[b][l] = the float64 sum of the finite trial[l][r0 .. r1): thread t adds the entries t, t + 256, ... in ascending order, then the
// 256 sums are halved eight times -- a function of r1 - r0 alone.  `red` is the tile, which nobody reads any more: L x 256 doubles
__device__ __forceinline__ void block_potentials(const StepArgs &a, const int64_t r0, const int64_t r1, double *red) {
    __syncthreads();                                 // the block's stores to trial are visible to it; the tile's readers are done
    const int t = threadIdx.x;
    for (int l = 0; l < a.trials; ++l) {
        const float *m = a.trial + (int64_t)l * a.n;
        double s = 0.0;
        for (int64_t i = r0 + t; i < r1; i += 256) {
            const float v = m[i];
            if (finite(v)) s += (double)v;
        }
        red[l * 256 + t] = s;
    }
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (t < h)
            for (int l = 0; l < a.trials; ++l) red[l * 256 + t] += red[l * 256 + t + h];
        __syncthreads();
    }
    if (t < a.trials) a.pot[(int64_t)blockIdx.x * kMaxTrials + t] = red[t * 256];
}

template <int LPR, int CH, bool VEC16, int U>
__global__ __launch_bounds__(256) void seed_step_kernel(const StepArgs a) {
    extern __shared__ __attribute__((aligned(16))) float tile[];
    constexpr int T = kSlots<LPR>, GPB = 256 / LPR;  // candidates per step of the transposing reduction; lane groups per workgroup
    constexpr int kWriters = LPR < 16 ? LPR : 16;    // the lanes that hold one total after reduce_slots
    const int l = threadIdx.x % LPR, g = threadIdx.x / LPR;
    const int d = a.d, dp = a.chunk, L = a.trials;   // one chunk: the whole padded row
    const int64_t n = a.n, r0 = blockIdx.x * a.rows, r1 = r0 + a.rows < n ? r0 + a.rows : n;
    stage_candidates<VEC16>(tile, a, 0, dp);
    __syncthreads();
    const float *near_tab = a.first ? nullptr : a.prev + (int64_t)(*a.best_prev) * n;
    for (int64_t base = r0; base < r1; base += GPB * U) {
        f4 xr[U][CH];
        float near[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t row = base + u * GPB + g;
            const bool live = row < r1;
            const float *p = a.x + (live ? row : r0) * a.ldx;
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                const int col = (c * LPR + l) * 4;
                f4 v = vzero<4>();
                if (live && col < d) v = row_vec<VEC16>(p, col, d, row == n - 1);
                xr[u][c] = v;
            }
            near[u] = (a.first || !live) ? __builtin_inff() : near_tab[row];
        }
        for (int jj = 0; jj < L; jj += T) {          // slots beyond L repeat the last candidate and are not stored
            Sq<4> acc[U][T];
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                const int col = (c * LPR + l) * 4;
                if (col < d) {
#pragma unroll
                    for (int t = 0; t < T; ++t) {
                        const int jt = jj + t < L ? jj + t : L - 1;
                        const f4 nc = *reinterpret_cast<const f4 *>(tile + jt * dp + col);
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
                const int64_t row = base + u * GPB + g;
                if (mine < L && row < r1 && l % kWriters == 0) a.trial[(int64_t)mine * n + row] = nan_min(near[u], s);
            }
        }
    }
    block_potentials(a, r0, r1, reinterpret_cast<double *>(tile));
}

// rows beyond the register layouts: kWideRows rows per wavefront, K9's streaming order; the candidates in column chunks of W
template <bool VEC16>
__global__ __launch_bounds__(256) void seed_step_wide_kernel(const StepArgs a) {
    extern __shared__ __attribute__((aligned(16))) float tile[];
    const int lane = threadIdx.x % 64, wave = threadIdx.x / 64;
    const int d = a.d, dp = (d + 3) / 4 * 4, W = a.chunk, L = a.trials;
    const int64_t n = a.n, r0 = blockIdx.x * a.rows, r1 = r0 + a.rows < n ? r0 + a.rows : n;
    const float *near_tab = a.first ? nullptr : a.prev + (int64_t)(*a.best_prev) * n;
    bool staged = false;
    for (int64_t base = r0; base < r1; base += 4 * kWideRows) {
        Sq<4> acc[kWideRows][kMaxTrials], part[kWideRows][kMaxTrials];
        int64_t row[kWideRows];
        const float *p[kWideRows];
#pragma unroll
        for (int u = 0; u < kWideRows; ++u) {
            row[u] = base + wave * kWideRows + u;
            p[u] = a.x + (row[u] < r1 ? row[u] : r0) * a.ldx;
        }
        for (int c0 = 0; c0 < dp; c0 += W) {
            const int w = dp - c0 < W ? dp - c0 : W;
            if (!(staged && W >= dp)) {              // candidates that fit whole are staged once per workgroup
                __syncthreads();
                stage_candidates<VEC16>(tile, a, c0, w);
                __syncthreads();
                staged = true;
            }
            for (int col = lane * 4; col < w; col += 256) {
                const int gc = c0 + col;             // gc / 256, the lane's chunk of the row, is the same for the 64 lanes
                if (gc >= kStreamBlock * 256 && (gc / 256) % kStreamBlock == 0) {
#pragma unroll
                    for (int u = 0; u < kWideRows; ++u)
#pragma unroll
                        for (int j = 0; j < kMaxTrials; ++j) acc[u][j].merge(part[u][j]), part[u][j] = Sq<4>();
                }
                f4 xv[kWideRows];
#pragma unroll
                for (int u = 0; u < kWideRows; ++u) xv[u] = row[u] < r1 ? row_vec<VEC16>(p[u], gc, d, row[u] == n - 1) : vzero<4>();
#pragma unroll
                for (int j = 0; j < kMaxTrials; ++j)
                    if (j < L) {
                        const f4 nc = *reinterpret_cast<const f4 *>(tile + j * W + col);
#pragma unroll
                        for (int u = 0; u < kWideRows; ++u) part[u][j].add_negated(xv[u], nc);
                    }
            }
        }
#pragma unroll
        for (int u = 0; u < kWideRows; ++u) {
            const float near = (a.first || row[u] >= r1) ? __builtin_inff() : near_tab[row[u]];
#pragma unroll
            for (int j = 0; j < kMaxTrials; ++j)
                if (j < L) {                         // the same for the 64 lanes
                    acc[u][j].merge(part[u][j]);
                    const float s = group_sum<64>(acc[u][j].total());
                    if (row[u] < r1 && lane == 0) a.trial[(int64_t)j * n + row[u]] = nan_min(near, s);
                }
        }
    }
    block_potentials(a, r0, r1, reinterpret_cast<double *>(tile));
}

struct PickArgs {
    int64_t n, rows, blocks;                         // n, R, B
    int trials, next, first;                         // L of this step; candidates to draw for the next (0: the last step); step 0
    const double *pot;                               // P
    const float *trial;
    int64_t *cand;
    int *best;
    const double *draws, *next_draws;                // the table; its row of the next step
    int64_t *centre_id;                              // &centre_ids[j]
    double *pot_out;                                 // &pot[j]
    float *near;                                     // the last step: trial[best] is copied here by all workgroups
};

// Everything sequential here is one thread's chain over values that ALL threads staged in LDS first: a chain over global memory
// pays a load's latency per term (measured: the step at 4 x one read of X with such chains, profiles/kmeans_seed.json has the run after)
__global__ __launch_bounds__(256) void seed_pick_kernel(const PickArgs a) {
    __shared__ double prefix[kMaxBlocks], stage[(kPickTile + 1) * kMaxTrials], total[kMaxTrials];
    __shared__ int64_t from[kMaxTrials], to[kMaxTrials];
    __shared__ int best_l;
    const int t = threadIdx.x;
    double s = 0.0;                                  // pot_l: ascending b, kPickTile blocks of P at a time
    for (int64_t b0 = 0; b0 < a.blocks; b0 += kPickTile) {
        const int nb = (int)(a.blocks - b0 < kPickTile ? a.blocks - b0 : kPickTile);
        for (int i = t; i < nb * kMaxTrials; i += 256) stage[i] = a.pot[b0 * kMaxTrials + i];
        __syncthreads();
        if (t < a.trials)
            for (int b = 0; b < nb; ++b) s += stage[b * kMaxTrials + t];
        __syncthreads();
    }
    if (t < a.trials) total[t] = s;
    __syncthreads();
    if (t == 0) {
        int best = 0;
        for (int l = 1; l < a.trials; ++l)
            if (total[l] < total[best]) best = l;    // the lowest l on a tie
        best_l = best;
        if (blockIdx.x == 0) {
            *a.best = best;
            *a.centre_id = a.first ? first_row(a.draws[0], a.n) : clamp_row(a.cand[best], a.n);
            *a.pot_out = total[best];
        }
    }
    __syncthreads();                                 // cand[best] was read above: the draws below may replace cand
    const float *m = a.trial + (int64_t)best_l * a.n;
    if (a.near) {
        for (int64_t i = (int64_t)blockIdx.x * 256 + t; i < a.n; i += (int64_t)gridDim.x * 256) a.near[i] = m[i];
        return;
    }
    if (!a.next) return;
    for (int64_t b = t; b < a.blocks; b += 256) prefix[b] = a.pot[b * kMaxTrials + best_l];
    __syncthreads();
    if (t == 0) {                                    // the inclusive prefix of P[.][best], the same chain as total[best]
        double run = 0.0;
        for (int64_t b = 0; b < a.blocks; ++b) prefix[b] = run += prefix[b];
    }
    __syncthreads();
    double target = 0.0, cum = 0.0;
    int64_t pick = a.n - 1;                          // no block: the clamp of the torch seeding
    bool open = false;
    if (t < a.next) {
        target = a.next_draws[t] * total[best_l];
        int64_t lo = 0, hi = a.blocks;               // the first block whose prefix exceeds the target: the prefix never decreases
        while (lo < hi) {
            const int64_t mid = (lo + hi) / 2;
            if (prefix[mid] > target) hi = mid;
            else lo = mid + 1;
        }
        open = lo < a.blocks;
        from[t] = open ? lo * a.rows : 0;
        to[t] = open ? (from[t] + a.rows < a.n ? from[t] + a.rows : a.n) : 0;
        if (open) {
            cum = lo ? prefix[lo - 1] : 0.0;
            pick = to[t] - 1;                        // the block's sum and this chain round differently: its last row when none exceeds
        }
    }
    __syncthreads();
    float *rows = reinterpret_cast<float *>(stage);  // kPickRows rows of every draw's block at a time, pitch kPickRows + 1
    for (int64_t off = 0; off < a.rows; off += kPickRows) {
        for (int q = 0; q < a.next; ++q)
            for (int i = t; i < kPickRows; i += 256)
                if (from[q] + off + i < to[q]) rows[q * (kPickRows + 1) + i] = m[from[q] + off + i];
        __syncthreads();
        if (open) {
            const int64_t left = to[t] - from[t] - off;
            const int count = (int)(left < kPickRows ? left : kPickRows);
            for (int i = 0; i < count; ++i) {
                const float v = rows[t * (kPickRows + 1) + i];
                if (finite(v)) cum += (double)v;
                if (cum > target) {
                    pick = from[t] + off + i;
                    open = false;
                    break;
                }
            }
        }
        __syncthreads();
    }
    if (t < a.next) a.cand[t] = pick;
}

constexpr int rows_per_group(int ch) { return ch <= 4 ? 4 : 2; }   // K9's: the row slices within 64 registers

int check_sizes(const char *who, int64_t n, int64_t d, int trials) {
    if (!(n >= 0 && d >= 0 && d < INT32_MAX)) return sgl::fail(SGL_ERR_INVALID, "%s: bad sizes", who);
    SGL_REQUIRE_WIDTH(who, "d", d);
    if (trials < 1 || trials > kMaxTrials)
        return sgl::fail(SGL_ERR_UNSUPPORTED, "%s: trials=%d is outside [1, %d]", who, trials, kMaxTrials);
    return SGL_OK;
}

}  // namespace

SGL_EXPORT int sgl_kmeans_seed_rule(int64_t n, int64_t d, int trials, int64_t *out) {
    SGL_REQUIRE(out, "sgl_kmeans_seed_rule: bad arguments");
    const int rc = check_sizes("sgl_kmeans_seed_rule", n, d, trials);
    if (rc != SGL_OK) return rc;
    SeedRule r;
    seed_rule(n, d, trials, r);
    out[0] = r.blocks, out[1] = r.rows, out[2] = r.chunk, out[3] = r.chunks, out[4] = r.lds;
    return SGL_OK;
}

SGL_EXPORT int64_t sgl_kmeans_seed_scratch(int64_t n, int trials) {
    if (check_sizes("sgl_kmeans_seed_scratch", n, 0, trials) != SGL_OK) return -1;
    return kPotBytes + kCandBytes + kBestBytes + 2 * table_bytes(n, trials);
}

SGL_EXPORT int sgl_kmeans_seed_f32(const float *d_x, int64_t ldx, int64_t n, int64_t d, int64_t k, int trials, const double *d_draws,
                                   int64_t *d_centre_ids, float *d_near, double *d_pot, void *d_scratch, void *stream) {
    const int rc = check_sizes("sgl_kmeans_seed_f32", n, d, trials);
    if (rc != SGL_OK) return rc;
    SGL_REQUIRE(k >= 1 && n >= k, "sgl_kmeans_seed_f32: n=%lld rows should be >= k=%lld >= 1", (long long)n, (long long)k);
    SGL_REQUIRE((d_x || d == 0) && d_draws && d_centre_ids && d_near && d_pot && d_scratch, "sgl_kmeans_seed_f32: NULL arguments");
    SGL_REQUIRE(ldx >= d, "sgl_kmeans_seed_f32: row pitch smaller than d");
    SGL_REQUIRE(aligned_to(d_x, 4) && aligned_to(d_near, 4) && aligned_to(d_draws, 8) && aligned_to(d_centre_ids, 8) && aligned_to(d_pot, 8) &&
                    aligned_to(d_scratch, 16),
                "sgl_kmeans_seed_f32: pointers must be aligned to their element size (the scratch to 16 bytes)");
    SeedRule rule;
    seed_rule(n, d, trials, rule);
    char *base = static_cast<char *>(d_scratch);
    double *pot = reinterpret_cast<double *>(base);
    int64_t *cand = reinterpret_cast<int64_t *>(base + kPotBytes);
    int *best = reinterpret_cast<int *>(base + kPotBytes + kCandBytes);
    float *table[2];
    table[0] = reinterpret_cast<float *>(base + kPotBytes + kCandBytes + kBestBytes);
    table[1] = reinterpret_cast<float *>(base + kPotBytes + kCandBytes + kBestBytes + table_bytes(n, trials));

    hipStream_t st = sgl::as_stream(stream);
    const bool vec16 = ldx % 4 == 0 && aligned_to(d_x, 16);
    const sgl::SliceInstance in = sgl::slice_instance(d, 4, sgl::KmeansSlices::chunks(4));   // K9's 16-byte-lane instance, whatever the lanes read
    const int64_t copy_blocks = (n + 255) / 256 < kCopyBlocks ? (n + 255) / 256 : kCopyBlocks;
    for (int64_t j = 0; j < k; ++j) {
        const int L = j == 0 ? 1 : trials, next = j + 1 < k ? trials : 0;
        SeedRule step = rule;                        // the blocks are the seeding's; the tile is this step's
        seed_rule(n, d, L, step);
        const StepArgs sa = {d_x, ldx, n, (int)d, L, j == 0, cand, d_draws, table[(j & 1) ^ 1], best, table[j & 1], pot, rule.rows, step.chunk};
        auto start = [&](auto LPR, auto C) {
            with_bool(vec16, [&](auto V16) {
                hipLaunchKernelGGL((seed_step_kernel<LPR, C, decltype(V16)::value, rows_per_group(C)>), dim3((unsigned)rule.blocks), dim3(256),
                                   (size_t)step.lds, st, sa);
            });
        };
        // (with_slice_instance would compile the 4-byte family's chunk counts as well, which this order never takes)
        const bool launched = in.ch == 1 ? with_lpr(in.lpr, [&](auto LPR) { start(LPR, Int<1>{}); })
                                         : with_chunks(sgl::KmeansSlices::Vec4{}, in.ch, [&](auto C) { start(Int<64>{}, C); });
        if (!launched) {                             // ch = 0: rows beyond the register layouts
            with_bool(vec16, [&](auto V16) {
                hipLaunchKernelGGL((seed_step_wide_kernel<decltype(V16)::value>), dim3((unsigned)rule.blocks), dim3(256), (size_t)step.lds, st, sa);
            });
        }
        SGL_LAUNCH_CHECK("sgl_kmeans_seed_f32");
        const PickArgs pa = {n,    rule.rows, rule.blocks, L, next, j == 0, pot, table[j & 1], cand, best, d_draws, d_draws + (j + 1) * trials,
                             d_centre_ids + j, d_pot + j, next ? nullptr : d_near};
        hipLaunchKernelGGL(seed_pick_kernel, dim3((unsigned)(next ? 1 : copy_blocks)), dim3(256), 0, st, pa);
        SGL_LAUNCH_CHECK("sgl_kmeans_seed_f32");
    }
    return SGL_OK;
}
