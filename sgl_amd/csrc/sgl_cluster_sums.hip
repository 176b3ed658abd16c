// K19: the per-cluster column sums and counts of the k-means centre update in one pass over X (include/sgl_cluster_sums.h states the
// contract).  The default update turns the labels into a k x N membership matrix -- a radix sort of N keys, a CSR, a plan -- and runs
// the SpMM over it; here a workgroup adds its rows straight into a k x slab table in LDS.
//
// Ownership instead of atomics.  Grid: B row blocks x S column slabs, blockIdx.x = b S + s, so the workgroups that share rows are
// neighbours.  Thread t of a workgroup of T threads owns the vectors t, t + T, ... (VEC floats each) of the slab, for ALL k clusters
// and for the life of the workgroup: it zeroes them, adds to them and writes them out itself.  No other lane ever touches them, so
// the kernel has no atomics and NO barrier at all, and consecutive lanes read consecutive 16-byte pieces of one LDS row (no bank
// conflict by construction).  T = the slab's vectors rounded up to whole wavefronts, at most 256: one wavefront at d = 100 and 128
// (25 / 32 lanes of it), two at d = 600 (S = 2 slabs of 300).  A thread with more than one vector walks its block's rows once per
// vector, so X is read once overall.
//
// The row loop.  The label of a row is the same for every lane: it is read once per row and kept in a scalar register
// (readfirstlane), as a slot in [0, k) or -1 for "skip".  kU rows make a batch; the loads of the NEXT batch are issued before the
// adds of this one, so kU rows (6.4 KB at d = 100) are in flight per wavefront while it adds.  An add is a plain LDS read, one
// float add, LDS write: acc = acc + x, rows in ascending order, so every (j, c) is the sequential sum of its rows.  A dependent LDS
// round trip per row would be latency-bound, so the rows of a batch whose labels are DISTINCT (the first row of every label) go
// first and kGroup at a time: reads together, adds, writes.  The remaining rows of the batch -- a label that occurred before --
// follow one by one in row order; the LDS executes a wavefront's accesses in order, so each reads what the row before it wrote.
// Every label still gets its rows in ascending order: which rows share a batch changes no bit.  The split is scalar code (a
// 64-bit mask of the labels seen, s_cbranch on its bits).
//
// Counts: the lane that owns column 0 of slab 0 keeps k int32 counts in LDS beside the table, one read-add-write per owner and
// batch.
#include "sgl_rows.h"   // edge_load, Vt, vzero, with_vec, SGL_LAUNCH_CHECK

#include "../../include/sgl_cluster_sums.h"

namespace {

constexpr int kU = 16;                               // rows per batch; the next batch's loads are issued before this one's adds
constexpr int kGroup = 8;                            // LDS round trips issued together
constexpr int kBudgetWords = 16384;                  // LDS of a workgroup, accumulators and counts: 64 KiB
constexpr int kMaxBlocks = 2048;                     // row blocks: 256 CUs x 8
constexpr int kRowsPerCluster = 40;                  // R >= 40 k dp / d: the tables' traffic, 2 k dp floats per block, is <= 5 % of X
constexpr int kFold = 32;                            // tables in flight per thread of the fold

struct SumsRule {
    int64_t blocks, rows;                            // B, R
    int slab, slabs;                                 // columns per slab, S
};
bool sums_rule(int64_t n, int64_t d, int64_t k, SumsRule &out) {
    if (k > SGL_CLUSTER_SUMS_MAX_K) return false;
    const int64_t dp = (d + 3) / 4 * 4;
    const int64_t slab_max = k ? (kBudgetWords - k) / k / 4 * 4 : dp;     // >= 12 for k <= MAX_K
    const int64_t slabs = (dp && slab_max) ? (dp + slab_max - 1) / slab_max : 0;
    const int64_t slab = slabs ? ((dp + slabs - 1) / slabs + 3) / 4 * 4 : 0;
    out = {0, 0, (int)slab, (int)slabs};
    if (n == 0 || d == 0 || k == 0) return true;
    const int64_t forced = sgl::tuning("loss_blocks", 0);
    const int64_t rmin = (kRowsPerCluster * k * dp + d - 1) / d;
    int64_t want = forced > 0 ? forced : (n / rmin > 1 ? n / rmin : 1);
    if (want > kMaxBlocks) want = kMaxBlocks;
    if (want > n) want = n;
    out.rows = (n + want - 1) / want;
    out.blocks = (n + out.rows - 1) / out.rows;
    return true;
}
int threads_of(const SumsRule &r, int64_t d, bool vec4) {
    const int64_t vecs = vec4 ? r.slab / 4 : (r.slab < d ? r.slab : d);
    const int64_t t = (vecs + 63) / 64 * 64;
    return t > 256 ? 256 : (t < 64 ? 64 : (int)t);
}
int64_t scratch_bytes(const SumsRule &r, int64_t k) {
    return r.blocks * r.slabs * k * r.slab * (int64_t)sizeof(float) + r.blocks * k * (int64_t)sizeof(int32_t);
}

// lane u < kU of every wavefront: the slot of the label of row `first + u`, [0, k), or -1 = nothing is added (a label outside [0, k),
// a row from `end` on -- those lanes read row end - 1 again); one 8-byte load per lane for the whole batch
__device__ __forceinline__ int batch_slots(const int64_t *__restrict__ labels, const int64_t first, const int64_t end, const int k) {
    const int64_t row = first + (threadIdx.x & (kU - 1));
    const int64_t l = labels[row < end ? row : end - 1];
    return (row < end && l >= 0 && l < k) ? (int)l : -1;
}

template <int VEC>
__global__ __launch_bounds__(256) void cluster_partial_kernel(const float *__restrict__ x, const int64_t ldx, const int64_t n, const int d,
                                                              const int64_t *__restrict__ labels, const int k, const int64_t rows,
                                                              const int slab, const int slabs, float *__restrict__ part,
                                                              int *__restrict__ pcount) {
    using V = typename Vt<VEC>::type;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    int *cnt = reinterpret_cast<int *>(lds + k * slab);
    const int64_t b = blockIdx.x / slabs;
    const int s = (int)(blockIdx.x % slabs), c_lo = s * slab;
    const int dp = (d + 3) / 4 * 4, cols = VEC == 4 ? dp : d;
    const int width = cols - c_lo < slab ? cols - c_lo : slab;
    const int64_t r0 = b * rows, r1 = r0 + rows < n ? r0 + rows : n;
    // The vector that straddles column d is read whole (its columns beyond d are sums nobody reads) except in the LAST row of x,
    // where nothing beyond column d may be read: that row stays out of the batches and is added after them (edge_load): it is the
    // last row of its block, so the order is still ascending
    const bool apart = VEC == 4 && d % 4 != 0 && r1 == n;
    const int64_t rv = apart ? r1 - 1 : r1;
    float *table = part + ((b * slabs + s) * k) * (int64_t)slab;
    const int wave_c = (int)(threadIdx.x & ~63u) * VEC;

    for (int cb = 0; cb + wave_c < width; cb += blockDim.x * VEC) {      // the same for the 64 lanes of a wavefront
        const int c = cb + threadIdx.x * VEC;
        const bool active = c < width;               // lanes beyond the slab run the scalar code along and touch no memory
        float *acc = lds + c;                        // this lane's columns of cluster j: acc + j * slab
        const float *xc = x + c_lo + c;
        const bool counting = s == 0 && c == 0;      // one lane of every slab-0 workgroup
        if (active)
            for (int j = 0; j < k; ++j) *reinterpret_cast<V *>(acc + j * slab) = vzero<VEC>();
        if (counting)
            for (int j = 0; j < k; ++j) cnt[j] = 0;

        V v[kU], w[kU];                              // this batch, the next one
        int slots = -1;                              // lane u: the slot of row u of the next batch
#pragma unroll
        for (int u = 0; u < kU; ++u) w[u] = vzero<VEC>();
        for (int64_t r = r0 - kU; rv > r0 && r < rv; r += kU) {   // the first turn only loads; rows beyond rv re-read row rv - 1
            // `first`: rows whose label (its low 6 bits: one bit of a 64-bit scalar mask) has not occurred in the batch; `again`:
            // the others that are not skipped.  Two labels that share the bit only send the later one down the second path.
            int lv[kU];
            uint64_t seen = 0;
            unsigned first = 0, again = 0;
#pragma unroll
            for (int u = 0; u < kU; ++u) {
                v[u] = w[u], lv[u] = __builtin_amdgcn_readlane(slots, u);
                const uint64_t bit = (uint64_t)(lv[u] >= 0) << (lv[u] & 63);
                if (lv[u] >= 0) (seen & bit ? again : first) |= 1u << u;
                seen |= bit;
            }
            slots = batch_slots(labels, r + kU, rv, k);
            if (active) {                            // the next batch's rows are in flight during the adds of this one
#pragma unroll
                for (int u = 0; u < kU; ++u) {
                    const int64_t row = r + kU + u;
                    w[u] = *reinterpret_cast<const V *>(xc + (row < rv ? row : rv - 1) * ldx);
                }
#pragma unroll
                for (int g = 0; g < kU; g += kGroup) {   // distinct labels: kGroup LDS round trips overlap
                    V t[kGroup];                     // every row reads (a row that is not `first` reads slot 0 and writes nothing):
                    int ct[kGroup];                  // only the stores are conditional, so the reads are issued back to back
#pragma unroll
                    for (int u = 0; u < kGroup; ++u) t[u] = *reinterpret_cast<const V *>(acc + (lv[g + u] < 0 ? 0 : lv[g + u]) * slab);
                    if (counting) {
#pragma unroll
                        for (int u = 0; u < kGroup; ++u) ct[u] = cnt[lv[g + u] < 0 ? 0 : lv[g + u]];
                    }
#pragma unroll
                    for (int u = 0; u < kGroup; ++u) {
                        const V sum = t[u] + v[g + u];
                        if (first >> (g + u) & 1) *reinterpret_cast<V *>(acc + lv[g + u] * slab) = sum;
                    }
                    if (counting) {
#pragma unroll
                        for (int u = 0; u < kGroup; ++u)
                            if (first >> (g + u) & 1) cnt[lv[g + u]] = ct[u] + 1;
                    }
                }
                if (again) {                         // after every first row, in ascending row order: one round trip each
#pragma unroll
                    for (int u = 1; u < kU; ++u)
                        if (again >> u & 1) {
                            V *a = reinterpret_cast<V *>(acc + lv[u] * slab);
                            *a = *a + v[u];
                            if (counting) cnt[lv[u]] += 1;
                        }
                }
            }
        }
        if (apart && r0 < n) {
            const int l = __builtin_amdgcn_readfirstlane(batch_slots(labels, n - 1, n, k));
            if (active && l >= 0) {
                V *a = reinterpret_cast<V *>(acc + l * slab);
                *a = *a + edge_load<VEC>(x + (n - 1) * ldx, c_lo + c, d, true);
                if (counting) cnt[l] += 1;
            }
        }
        if (active)
            for (int j = 0; j < k; ++j) *reinterpret_cast<V *>(table + (int64_t)j * slab + c) = *reinterpret_cast<const V *>(acc + j * slab);
        if (counting)
            for (int j = 0; j < k; ++j) pcount[b * k + j] = cnt[j];
    }
}

// sums[j, c] = the B tables' values in ascending block order, one float32 add each; counts[j] the same in int64.  kFold loads are
// issued before their adds: the tables are B strided reads per thread
__global__ __launch_bounds__(256) void cluster_fold_kernel(const float *__restrict__ part, const int *__restrict__ pcount, const int64_t blocks,
                                                           const int slab, const int slabs, const int k, const int d,
                                                           float *__restrict__ sums, const int64_t lds, int64_t *__restrict__ counts) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx < (int64_t)k * d) {
        const int64_t j = idx / d;
        const int c = (int)(idx % d), s = c / slab;
        const float *p = part + ((int64_t)s * k + j) * slab + (c - s * slab);
        const int64_t stride = (int64_t)slabs * k * slab;
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
        sums[j * lds + c] = a;
    }
    if (idx < k) {
        int64_t m = 0;
        for (int64_t b = 0; b < blocks; ++b) m += pcount[b * k + idx];
        counts[idx] = m;
    }
}

// d = 0: the counts alone, straight from the labels (one thread per cluster; nothing to sum)
__global__ __launch_bounds__(256) void cluster_count_kernel(const int64_t *__restrict__ labels, const int64_t n, const int k,
                                                            int64_t *__restrict__ counts) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= k) return;
    int64_t m = 0;
    for (int64_t i = 0; i < n; ++i) m += labels[i] == j;
    counts[j] = m;
}

int check_sizes(const char *who, int64_t n, int64_t d, int64_t k, SumsRule &rule) {
    if (!(n >= 0 && d >= 0 && d < INT32_MAX && k >= 0)) return sgl::fail(SGL_ERR_INVALID, "%s: bad sizes", who);
    SGL_REQUIRE_WIDTH(who, "d", d);
    if (!sums_rule(n, d, k, rule))
        return sgl::fail(SGL_ERR_UNSUPPORTED, "%s: k=%lld is beyond the LDS budget (k <= %d)", who, (long long)k, SGL_CLUSTER_SUMS_MAX_K);
    if (rule.rows > INT32_MAX) return sgl::fail(SGL_ERR_UNSUPPORTED, "%s: %lld rows per block overflow the int32 block counts", who, (long long)rule.rows);
    return SGL_OK;
}

}  // namespace

SGL_EXPORT int sgl_cluster_sums_rule(int64_t n, int64_t d, int64_t k, int vec4, int64_t *out) {
    SGL_REQUIRE(out && (vec4 == 0 || vec4 == 1), "sgl_cluster_sums_rule: bad arguments");
    SumsRule r;
    const int rc = check_sizes("sgl_cluster_sums_rule", n, d, k, r);
    if (rc != SGL_OK) return rc;
    out[0] = r.blocks, out[1] = r.rows, out[2] = r.slab, out[3] = r.slabs, out[4] = (k * r.slab + k) * (int64_t)sizeof(float);
    return SGL_OK;
}

SGL_EXPORT int64_t sgl_cluster_sums_scratch(int64_t n, int64_t d, int64_t k) {
    SumsRule r;
    return check_sizes("sgl_cluster_sums_scratch", n, d, k, r) == SGL_OK ? scratch_bytes(r, k) : -1;
}

SGL_EXPORT int sgl_cluster_sums_f32(const float *d_x, int64_t ldx, int64_t n, int64_t d, const int64_t *d_labels, int64_t k, float *d_sums,
                                    int64_t lds, int64_t *d_counts, void *d_scratch, void *stream) {
    SumsRule rule;
    const int rc = check_sizes("sgl_cluster_sums_f32", n, d, k, rule);
    if (rc != SGL_OK) return rc;
    SGL_REQUIRE((d_x || n == 0 || d == 0) && (d_labels || n == 0) && (d_sums || k == 0 || d == 0) && (d_counts || k == 0) &&
                    (d_scratch || rule.blocks == 0),
                "sgl_cluster_sums_f32: NULL arguments");
    SGL_REQUIRE(ldx >= d && lds >= d, "sgl_cluster_sums_f32: row pitch smaller than d");
    SGL_REQUIRE(aligned_to(d_x, 4) && aligned_to(d_sums, 4) && aligned_to(d_labels, 8) && aligned_to(d_counts, 8) && aligned_to(d_scratch, 16),
                "sgl_cluster_sums_f32: pointers must be aligned to their element size (the scratch to 16 bytes)");
    if (k == 0) return SGL_OK;
    hipStream_t st = sgl::as_stream(stream);
    const int ki = (int)k, di = (int)d;
    if (d == 0) {
        hipLaunchKernelGGL(cluster_count_kernel, dim3((unsigned)((k + 255) / 256)), dim3(256), 0, st, d_labels, n, ki, d_counts);
        SGL_LAUNCH_CHECK("sgl_cluster_sums_f32");
        return SGL_OK;
    }
    float *part = static_cast<float *>(d_scratch);
    int *pcount = reinterpret_cast<int *>(part + rule.blocks * rule.slabs * k * rule.slab);
    if (rule.blocks) {
        const bool vec4 = ldx % 4 == 0 && aligned_to(d_x, 16);
        const int64_t grid = rule.blocks * rule.slabs;
        if (!sgl::launch_fits(grid, 256)) return sgl::fail(SGL_ERR_UNSUPPORTED, "sgl_cluster_sums_f32: the grid does not fit one launch");
        const size_t lds_bytes = ((size_t)k * rule.slab + k) * sizeof(float);
        const int threads = threads_of(rule, d, vec4);
        with_vec(vec4, [&](auto V) {
            hipLaunchKernelGGL((cluster_partial_kernel<V>), dim3((unsigned)grid), dim3(threads), lds_bytes, st, d_x, ldx, n, di, d_labels, ki,
                               rule.rows, rule.slab, rule.slabs, part, pcount);
        });
        SGL_LAUNCH_CHECK("sgl_cluster_sums_f32");
    }
    const int64_t cells = k * d;
    if (!sgl::launch_fits((cells + 255) / 256, 256)) return sgl::fail(SGL_ERR_UNSUPPORTED, "sgl_cluster_sums_f32: the grid does not fit one launch");
    hipLaunchKernelGGL(cluster_fold_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, part, pcount, rule.blocks, rule.slab,
                       rule.slabs, ki, di, d_sums, lds, d_counts);
    SGL_LAUNCH_CHECK("sgl_cluster_sums_f32");
    return SGL_OK;
}
