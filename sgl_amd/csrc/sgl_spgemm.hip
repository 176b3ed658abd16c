// K17: the product C = A . B of two canonical CSRs (columns sorted and unique inside a row) as a new canonical CSR -- the one graph
// building step of the reference that needs a sparse x sparse product (sgl/data/base_dataset.py:313-396, sample_by_meta_path, whose
// scipy line is marked "# extremely slow").  include/sgl_spgemm.h states the contract: a structural pattern (a zero sum stays stored),
// values that are the ordered float32 chain acc = fadd_rn(acc, fmul_rn(a, b)) over A's row in storage order (SGL_SPGEMM_SUM) or 1.0
// (SGL_SPGEMM_ONES).  Two passes like K13 / K15: count every row, scan the counts into the row pointer (rocPRIM), fill.  No global
// atomic touches an output, no temporary is entry-sized: the counts, the class lists and the scan's workspace are O(m).
//
// The size of a row of C is unknown until it is computed, one column arrives many times, and rows range from empty to hub rows whose
// candidate list fits no LDS budget.  So every pass starts with spgemm_bound_kernel: ub(i) = sum over A's row i of the lengths of B's
// rows, the number of candidate products, puts the row into a class, and the rows of a class are compacted into a list on the device
// (LDS ranks inside a workgroup, one global add per workgroup and class on the list's length: the order of a list is arbitrary and
// no output depends on it).  The class kernels read the lengths on the device and stride over their list; the host never sees them.
//
//   narrow rows, ub <= narrow_cap: EXPAND, SORT, COMPRESS in LDS.  G lanes per row and a slice of CAP = 8 G keys per group, three
//     compiled instances (G, CAP) = (4, 32), (16, 128), (64, 512) -- 16 KB of keys per workgroup each; a row goes to the smallest
//     slice that holds ub.  The group writes the row's candidates as 64-bit keys (column << 32) | s, s the running number of the
//     product (it grows with A's storage order), a column outside [0, n) as the all-ones key; the fill pass also writes the rounded
//     product to prod[s].  A bitonic network sorts the slice (its power-of-two prefix; the stages are workgroup barriers, so the
//     workgroup runs the stages of its largest row and every group skips the ones beyond its own).  Then the runs of equal columns:
//     the count pass counts run heads; in the fill pass the lane at a run head gets its slot from the heads before it (running count
//     + the wavefront's ballot below the lane, as in K15) and adds the run's products IN KEY ORDER, which is the contract's order.
//   wide rows, ub > narrow_cap: one workgroup of 512 threads per row and an LDS BITMAP over a window of W columns (W = 1024, 32768,
//     524288 compiled).  The walked range is the row's own [min, max] candidate column (first and last column of every B row).  Per
//     window: clear the words, teams of 16 lanes take A's entries in turn and stride over the part of B's row inside the window (two
//     csr_range_lower_bound calls), setting bits with LDS atomic OR -- idempotent, so order cannot matter.  Count: population counts.
//     Fill: a workgroup prefix over the population counts of each thread's contiguous words turns every set bit into its slot, so
//     the columns come out ascending with no sort; under SUM the window's entries are then dealt to the threads in turn and each
//     walks A's row in order, finding its column in every B row by bisection -- the contract's chain again.  ONES writes 1.0.
//
// Both passes of a class are ONE kernel template (FILL = false / true).  Hostile contents never trap: row ranges are clamped into
// [0, nnz], a column of A outside [0, k) is an empty row of B, a column of B outside [0, n) is skipped, a narrow row whose lengths no
// longer fit its slice stops expanding, and a fill never writes outside its output row.
#include "sgl_csr_search.h"
#include "sgl_rows.h"

#include "../../include/sgl_spgemm.h"

#include <rocprim/device/device_scan.hpp>

namespace {

constexpr int kClasses = 4;                  // 0 .. 2: the narrow instances in rising slice size, 3: wide
constexpr int kWide = 3;
constexpr int kWideThreads = 512, kTeam = 16;
constexpr uint64_t kNoKey = ~0ull;           // sorts behind every column

struct Mat {
    const int64_t *rowptr;
    const int32_t *col;
    int64_t nnz;
};

struct Product {
    Mat a, b;
    int64_t m, k, n;
    int mode, narrow_cap;
};

// what the class kernels get besides the product: the values, the class's list and its length, the outputs of either pass
struct Pass {
    const float *a_val, *b_val;
    const int32_t *list;
    const int *list_n;
    int64_t *counts;
    const int64_t *out_rowptr;
    int32_t *out_col;
    float *out_val;
};

// row i of a matrix as [begin, end), inside [0, nnz] whatever the row pointer holds
__device__ __forceinline__ void mat_row(const Mat &s, const int64_t i, int64_t &begin, int64_t &end) {
    const int64_t lo = s.rowptr[i], hi = s.rowptr[i + 1];
    begin = lo < 0 ? 0 : lo > s.nnz ? s.nnz : lo;
    end = hi < begin ? begin : hi > s.nnz ? s.nnz : hi;
}

// the row of B that column j of A selects; empty when j is no row of B
__device__ __forceinline__ void b_row(const Product &P, const int32_t j, int64_t &begin, int64_t &end) {
    begin = end = 0;
    if (j >= 0 && j < P.k) mat_row(P.b, j, begin, end);
}

// the class of a row with ub candidate products, -1: the row is empty.  The one place where that is decided.
__device__ __forceinline__ int row_class(const int64_t ub, const int narrow_cap) {
    if (ub <= 0) return -1;
    if (ub > narrow_cap) return kWide;
    return ub <= 32 ? 0 : ub <= 128 ? 1 : 2;
}

// One thread per row: the bound, the class, the row's place in its class's list.  lists: kClasses arrays of m rows; list_n: their
// lengths, zero on entry.  counts (count pass only): every row's count starts as 0, the class kernels write the others.
__global__ __launch_bounds__(256) void spgemm_bound_kernel(const Product P, int32_t *__restrict__ lists, int *__restrict__ list_n,
                                                           int64_t *__restrict__ counts) {
    __shared__ int s_n[kClasses], s_base[kClasses];
    for (int64_t base = (int64_t)blockIdx.x * 256; base < P.m; base += (int64_t)gridDim.x * 256) {
        const int64_t i = base + threadIdx.x;
        int cls = -1;
        if (i < P.m) {
            int64_t a0, a1, ub = 0;
            mat_row(P.a, i, a0, a1);
            for (int64_t p = a0; p < a1; ++p) {
                int64_t b0, b1;
                b_row(P, P.a.col[p], b0, b1);
                ub += b1 - b0;
            }
            cls = row_class(ub, P.narrow_cap);
            if (counts) counts[i] = 0;
        }
        if (threadIdx.x < kClasses) s_n[threadIdx.x] = 0;
        __syncthreads();
        const int rank = cls >= 0 ? atomicAdd(&s_n[cls], 1) : 0;
        __syncthreads();
        if (threadIdx.x < kClasses && s_n[threadIdx.x] > 0) s_base[threadIdx.x] = atomicAdd(&list_n[threadIdx.x], s_n[threadIdx.x]);
        __syncthreads();
        if (cls >= 0) {
            const int64_t at = (int64_t)s_base[cls] + rank;
            if (at < P.m) lists[cls * P.m + at] = (int32_t)i;
        }
        __syncthreads();                                             // s_n is cleared again by the next round
    }
}

// is t the first key of a run of one column?
__device__ __forceinline__ bool run_head(const uint64_t *key, const int t) {
    const uint64_t k = key[t];
    return k != kNoKey && (t == 0 || (key[t - 1] >> 32) != (k >> 32));
}

template <int G, int CAP, bool FILL>
__global__ __launch_bounds__(256) void spgemm_narrow_kernel(const Product P, const Pass io) {
    static_assert(G >= 1 && G <= 64 && (G & (G - 1)) == 0 && (CAP & (CAP - 1)) == 0, "a group is a power-of-two part of one wavefront");
    constexpr int kRows = 256 / G;
    __shared__ uint64_t keys[kRows * CAP];
    __shared__ float prods[FILL ? kRows * CAP : 1];
    __shared__ int s_stages;
    const int g = threadIdx.x / G, lane = threadIdx.x & (G - 1);
    uint64_t *key = keys + g * CAP;
    float *prod = prods + (FILL ? g * CAP : 0);
    const int shift = (threadIdx.x & 63) & ~(G - 1);                 // the group's first bit in the wavefront's ballot
    const uint64_t group = G == 64 ? ~0ull : ((1ull << (G & 63)) - 1);
    const uint64_t below = (1ull << lane) - 1;
    const bool sum = P.mode == SGL_SPGEMM_SUM;
    int64_t n_list = *io.list_n;
    if (n_list > P.m) n_list = P.m;
    // every thread of the workgroup makes the same number of rounds: the stages of the network are workgroup barriers
    for (int64_t base = (int64_t)blockIdx.x * kRows; base < n_list; base += (int64_t)gridDim.x * kRows) {
        const bool live = base + g < n_list;
        int64_t i = 0;
        int cand = 0;                                                // candidate slots of the row, skipped columns included
        if (live) {
            i = io.list[base + g];
            int64_t a0, a1;
            mat_row(P.a, i, a0, a1);
            for (int64_t p = a0; p < a1; ++p) {
                int64_t b0, b1;
                b_row(P, P.a.col[p], b0, b1);
                if (b1 - b0 > CAP - cand) break;                     // the bound said it fits; memory that changed since must not overflow the slice
                for (int64_t q = b0 + lane; q < b1; q += G) {
                    const int32_t c = P.b.col[q];
                    const int s = cand + (int)(q - b0);
                    const bool stored = c >= 0 && c < P.n;
                    key[s] = stored ? ((uint64_t)(uint32_t)c << 32) | (uint32_t)s : kNoKey;
                    if (FILL && sum && stored) prod[s] = __fmul_rn(io.a_val[p], io.b_val[q]);
                }
                cand += (int)(b1 - b0);
            }
        }
        int n2 = 1;                                                  // the sorted prefix of the slice
        while (n2 < cand) n2 <<= 1;
        if (live)
            for (int s = cand + lane; s < n2; s += G) key[s] = kNoKey;
        if (threadIdx.x == 0) s_stages = 0;
        __syncthreads();
        if (live && lane == 0) atomicMax(&s_stages, n2);
        __syncthreads();
        const int n_max = s_stages;
        for (int kk = 2; kk <= n_max; kk <<= 1) {
            for (int jj = kk >> 1; jj > 0; jj >>= 1) {
                if (live && kk <= n2) {
                    for (int t = lane; t < (n2 >> 1); t += G) {
                        const int lo = ((t & ~(jj - 1)) << 1) | (t & (jj - 1)), hi = lo | jj;
                        const bool rising = (lo & kk) == 0;
                        const uint64_t x = key[lo], y = key[hi];
                        if ((x > y) == rising) {
                            key[lo] = y;
                            key[hi] = x;
                        }
                    }
                }
                __syncthreads();
            }
        }
        if (!FILL) {
            int heads = 0;
            if (live)
                for (int t = lane; t < n2; t += G) heads += run_head(key, t);
            for (int o = G >> 1; o > 0; o >>= 1) heads += __shfl_xor(heads, o, G);
            if (live && lane == 0) io.counts[i] = heads;
        } else {
            int64_t out = 0, out_end = 0;
            if (live) {
                out = io.out_rowptr[i];
                out_end = io.out_rowptr[i + 1];
            }
            for (int t0 = 0; t0 < n_max; t0 += G) {                  // the same trips for every lane of a wavefront: they meet at the ballot
                const int t = t0 + lane;
                const bool head = live && t < n2 && run_head(key, t);
                const uint64_t bits = ((uint64_t)__ballot(head) >> shift) & group;
                if (head) {
                    const int64_t o = out + __popcll(bits & below);
                    if (o < out_end) {
                        const uint64_t k = key[t];
                        float v = 1.0f;
                        if (sum) {
                            v = 0.0f;
                            for (int u = t; u < n2 && (key[u] >> 32) == (k >> 32); ++u) v = __fadd_rn(v, prod[(uint32_t)key[u]]);
                        }
                        io.out_col[o] = (int32_t)(k >> 32);
                        io.out_val[o] = v;
                    }
                }
                out += __popcll(bits);
            }
        }
        __syncthreads();                                             // the slices are written again by the next round
    }
}

// where word x of the bitmap lives: a thread owns contiguous words, so a stride of 32 words between lanes would meet in one LDS bank;
// the word's place inside its group of 32 is turned by the group's number
__device__ __forceinline__ int word_at(const int x) { return x ^ ((x >> 5) & 31); }

template <int W, bool FILL>
__global__ __launch_bounds__(kWideThreads) void spgemm_wide_kernel(const Product P, const Pass io) {
    static_assert(W % 32 == 0, "a window is whole words");
    constexpr int kWaves = kWideThreads / 64, kTeams = kWideThreads / kTeam;
    __shared__ uint32_t bits[W / 32];
    __shared__ int s_wave[kWaves], s_min, s_max;
    const int tid = threadIdx.x, team = tid / kTeam, tl = tid % kTeam;
    const bool sum = P.mode == SGL_SPGEMM_SUM;
    int64_t n_list = *io.list_n;
    if (n_list > P.m) n_list = P.m;
    for (int64_t r = blockIdx.x; r < n_list; r += gridDim.x) {
        const int64_t i = io.list[r];
        int64_t a0, a1;
        mat_row(P.a, i, a0, a1);
        // the row's own candidate range: B's rows are sorted, so their first and last columns bound it
        if (tid == 0) {
            s_min = INT32_MAX;
            s_max = -1;
        }
        __syncthreads();
        int32_t mn = INT32_MAX, mx = -1;
        for (int64_t p = a0 + tid; p < a1; p += kWideThreads) {
            int64_t b0, b1;
            b_row(P, P.a.col[p], b0, b1);
            if (b1 > b0) {
                mn = min(mn, P.b.col[b0]);
                mx = max(mx, P.b.col[b1 - 1]);
            }
        }
        if (mn != INT32_MAX) atomicMin(&s_min, mn);
        if (mx >= 0) atomicMax(&s_max, mx);
        __syncthreads();
        const int64_t lo = s_min < 0 ? 0 : s_min, hi = s_max < P.n ? s_max : P.n - 1;
        int64_t out = 0, out_end = 0, total = 0;
        if (FILL) {
            out = io.out_rowptr[i];
            out_end = io.out_rowptr[i + 1];
        }
        for (int64_t w0 = lo; w0 <= hi; w0 += W) {                   // [w0, w1): one window; w1 <= n fits an int32
            const int64_t w1 = w0 + W < hi + 1 ? w0 + W : hi + 1;
            const int words = (int)((w1 - w0 + 31) >> 5);
            for (int x = tid; x < ((words + 31) & ~31); x += kWideThreads) bits[x] = 0;   // whole groups of 32 words: see word_at
            __syncthreads();
            for (int64_t p = a0 + team; p < a1; p += kTeams) {
                int64_t b0, b1;
                b_row(P, P.a.col[p], b0, b1);
                const int64_t q0 = csr_range_lower_bound(P.b.col, b0, b1 - b0, (int32_t)w0);
                const int64_t q1 = csr_range_lower_bound(P.b.col, q0, b1 - q0, (int32_t)w1);
                for (int64_t q = q0 + tl; q < q1; q += kTeam) {
                    const int64_t c = P.b.col[q];
                    if (c >= w0 && c < w1) atomicOr(&bits[word_at((int)((c - w0) >> 5))], 1u << ((c - w0) & 31));
                }
            }
            __syncthreads();
            // every thread owns `per` contiguous words: its population count, then the workgroup's prefix over them
            const int per = (words + kWideThreads - 1) / kWideThreads;
            const int first = tid * per < words ? tid * per : words, last = first + per < words ? first + per : words;
            int mine = 0;
            for (int x = first; x < last; ++x) mine += __popc(bits[word_at(x)]);
            int upto = mine;                                         // inclusive, inside the wavefront
            for (int o = 1; o < 64; o <<= 1) {
                const int y = __shfl_up(upto, o, 64);
                if ((tid & 63) >= o) upto += y;
            }
            if ((tid & 63) == 63) s_wave[tid >> 6] = upto;
            __syncthreads();
            int before = 0, all = 0;
            for (int w = 0; w < kWaves; ++w) {
                if (w < (tid >> 6)) before += s_wave[w];
                all += s_wave[w];
            }
            if (FILL) {
                int64_t o = out + total + before + upto - mine;
                for (int x = first; x < last; ++x) {
                    for (uint32_t rest = bits[word_at(x)]; rest; rest &= rest - 1, ++o) {
                        if (o < out || o >= out_end) continue;
                        io.out_col[o] = (int32_t)(w0 + ((int64_t)x << 5) + (__ffs(rest) - 1));
                        if (!sum) io.out_val[o] = 1.0f;
                    }
                }
                if (sum) {
                    __syncthreads();                                 // the window's columns are in place: its entries are dealt to the threads
                    int64_t end = out + total + all;
                    if (end > out_end) end = out_end;
                    for (int64_t e = out + total + tid; e < end; e += kWideThreads) {
                        const int32_t c = io.out_col[e];
                        float v = 0.0f;
                        for (int64_t p = a0; p < a1; ++p) {
                            int64_t b0, b1;
                            b_row(P, P.a.col[p], b0, b1);
                            const int64_t q = csr_range_lower_bound(P.b.col, b0, b1 - b0, c);
                            if (q < b1 && P.b.col[q] == c) v = __fadd_rn(v, __fmul_rn(io.a_val[p], io.b_val[q]));
                        }
                        io.out_val[e] = v;
                    }
                }
            }
            total += all;
            __syncthreads();                                         // the words and the wave sums are written again by the next window
        }
        if (!FILL && tid == 0) io.counts[i] = total;
        __syncthreads();                                             // s_min and s_max are read before the next row resets them
    }
}

struct Tmp {
    std::vector<void *> ptrs;
    ~Tmp() {
        for (void *p : ptrs) (void)hipFree(p);
    }
    template <typename T>
    int alloc(const char *who, T **out, size_t count) {
        void *p = nullptr;
        hipError_t e = hipMalloc(&p, std::max<size_t>(count, 1) * sizeof(T));
        if (e != hipSuccess) return sgl::fail((int)e, "%s: hipMalloc failed: %s", who, hipGetErrorString(e));
        ptrs.push_back(p);
        *out = reinterpret_cast<T *>(p);
        return SGL_OK;
    }
};

// what both entries refuse, before any launch
int check_matmul(const char *who, const int64_t *a_rowptr, const int32_t *a_col, int64_t nnz_a, const int64_t *b_rowptr, const int32_t *b_col,
                 int64_t nnz_b, int64_t m, int64_t k, int64_t n, int narrow_cap, int window_cols, sgl::SpgemmRule &rule) {
    SGL_REQUIRE(m >= 0 && k >= 0 && n >= 0 && nnz_a >= 0 && nnz_b >= 0, "%s: bad sizes (negative)", who);
    SGL_REQUIRE(m <= INT32_MAX && k <= INT32_MAX && n <= INT32_MAX, "%s: bad sizes (m, k and n must be < 2^31)", who);
    SGL_REQUIRE(a_rowptr && a_col && b_rowptr && b_col, "%s: NULL arguments (a_rowptr, a_col, b_rowptr, b_col)", who);
    SGL_REQUIRE(aligned_to(a_rowptr, 8) && aligned_to(a_col, 4) && aligned_to(b_rowptr, 8) && aligned_to(b_col, 4),
                "%s: pointers must be aligned to their element size", who);
    return sgl::spgemm_rule(who, narrow_cap, window_cols, n, rule);
}

template <bool FILL>
void launch_narrow(int cls, int64_t m, hipStream_t st, const Product &P, const Pass &io) {
    const int rows_per_block = cls == 0 ? 64 : cls == 1 ? 16 : 4;
    // 256 CUs x 8 workgroups x 4 rounds; the rows beyond are strided
    const dim3 grid((unsigned)sgl::spgemm_grid((m + rows_per_block - 1) / rows_per_block, 8192));
    if (cls == 0)
        hipLaunchKernelGGL((spgemm_narrow_kernel<4, 32, FILL>), grid, dim3(256), 0, st, P, io);
    else if (cls == 1)
        hipLaunchKernelGGL((spgemm_narrow_kernel<16, 128, FILL>), grid, dim3(256), 0, st, P, io);
    else
        hipLaunchKernelGGL((spgemm_narrow_kernel<64, 512, FILL>), grid, dim3(256), 0, st, P, io);
}

template <bool FILL>
void launch_wide(int window_cols, int64_t m, hipStream_t st, const Product &P, const Pass &io) {
    const dim3 grid((unsigned)sgl::spgemm_grid(m, 2048));            // 256 CUs x 2 workgroups x 4 rounds
    if (window_cols == 1024)
        hipLaunchKernelGGL((spgemm_wide_kernel<1024, FILL>), grid, dim3(kWideThreads), 0, st, P, io);
    else if (window_cols == 32768)
        hipLaunchKernelGGL((spgemm_wide_kernel<32768, FILL>), grid, dim3(kWideThreads), 0, st, P, io);
    else
        hipLaunchKernelGGL((spgemm_wide_kernel<524288, FILL>), grid, dim3(kWideThreads), 0, st, P, io);
}

// one pass over every class: the bound and the lists, then each class's kernel on its list
template <bool FILL>
int run_pass(const char *who, Tmp &tmp, hipStream_t st, const Product &P, const sgl::SpgemmRule &rule, Pass io) {
    int rc;
    int32_t *lists = nullptr;
    int *list_n = nullptr;
    if ((rc = tmp.alloc(who, &lists, (size_t)kClasses * (size_t)P.m)) != SGL_OK) return rc;
    if ((rc = tmp.alloc(who, &list_n, kClasses)) != SGL_OK) return rc;
    SGL_HIP_CHECK(hipMemsetAsync(list_n, 0, sizeof(int) * kClasses, st));
    hipLaunchKernelGGL(spgemm_bound_kernel, dim3((unsigned)sgl::spgemm_grid((P.m + 255) / 256, 8192)), dim3(256), 0, st, P, lists, list_n,
                       FILL ? nullptr : io.counts);
    SGL_LAUNCH_CHECK(who);
    static const int caps[] = SGL_SPGEMM_NARROW_CAPS;
    for (int cls = 0; cls < kClasses; ++cls) {
        if (cls != kWide && caps[cls] > rule.narrow_cap) continue;   // no row is in that class
        io.list = lists + (size_t)cls * (size_t)P.m;
        io.list_n = list_n + cls;
        if (cls == kWide)
            launch_wide<FILL>(rule.window_cols, P.m, st, P, io);
        else
            launch_narrow<FILL>(cls, P.m, st, P, io);
        SGL_LAUNCH_CHECK(who);
    }
    return SGL_OK;
}

}  // namespace

SGL_EXPORT int sgl_csr_matmul_rowptr(const int64_t *a_rowptr, const int32_t *a_col, int64_t nnz_a, const int64_t *b_rowptr, const int32_t *b_col,
                                     int64_t nnz_b, int64_t m, int64_t k, int64_t n, int narrow_cap, int window_cols, int64_t *d_out_rowptr,
                                     int64_t *h_nnz_out, void *stream) {
    const char *who = "sgl_csr_matmul_rowptr";
    sgl::SpgemmRule rule;
    int rc = check_matmul(who, a_rowptr, a_col, nnz_a, b_rowptr, b_col, nnz_b, m, k, n, narrow_cap, window_cols, rule);
    if (rc != SGL_OK) return rc;
    SGL_REQUIRE(d_out_rowptr && h_nnz_out, "sgl_csr_matmul_rowptr: NULL arguments (d_out_rowptr, h_nnz_out)");
    SGL_REQUIRE(aligned_to(d_out_rowptr, 8), "sgl_csr_matmul_rowptr: pointers must be aligned to their element size");
    hipStream_t st = sgl::as_stream(stream);
    if (m == 0 || k == 0 || n == 0 || nnz_a == 0 || nnz_b == 0) {
        SGL_HIP_CHECK(hipMemsetAsync(d_out_rowptr, 0, sizeof(int64_t) * (size_t)(m + 1), st));
        SGL_HIP_CHECK(hipStreamSynchronize(st));
        *h_nnz_out = 0;
        return SGL_OK;
    }
    const Product P{{a_rowptr, a_col, nnz_a}, {b_rowptr, b_col, nnz_b}, m, k, n, SGL_SPGEMM_ONES, rule.narrow_cap};
    Tmp tmp;
    int64_t *counts = nullptr;
    const size_t n_scan = (size_t)m + 1;
    if ((rc = tmp.alloc(who, &counts, n_scan)) != SGL_OK) return rc;
    SGL_HIP_CHECK(hipMemsetAsync(counts + m, 0, sizeof(int64_t), st));           // the scan's last input; every row's count is written
    if ((rc = run_pass<false>(who, tmp, st, P, rule, Pass{nullptr, nullptr, nullptr, nullptr, counts, nullptr, nullptr, nullptr})) != SGL_OK) return rc;
    size_t bytes = 0;
    SGL_HIP_CHECK(rocprim::exclusive_scan(nullptr, bytes, counts, d_out_rowptr, (int64_t)0, n_scan, rocprim::plus<int64_t>(), st));
    char *scratch = nullptr;
    if ((rc = tmp.alloc(who, &scratch, bytes)) != SGL_OK) return rc;
    SGL_HIP_CHECK(rocprim::exclusive_scan(scratch, bytes, counts, d_out_rowptr, (int64_t)0, n_scan, rocprim::plus<int64_t>(), st));
    int64_t total = 0;
    SGL_HIP_CHECK(hipMemcpyAsync(&total, d_out_rowptr + m, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    SGL_HIP_CHECK(hipStreamSynchronize(st));
    *h_nnz_out = total;
    return SGL_OK;
}

SGL_EXPORT int sgl_csr_matmul_fill(const int64_t *a_rowptr, const int32_t *a_col, const float *a_val, int64_t nnz_a, const int64_t *b_rowptr,
                                   const int32_t *b_col, const float *b_val, int64_t nnz_b, int64_t m, int64_t k, int64_t n, int mode, int narrow_cap,
                                   int window_cols, const int64_t *d_out_rowptr, int32_t *d_out_col, float *d_out_val, void *stream) {
    const char *who = "sgl_csr_matmul_fill";
    sgl::SpgemmRule rule;
    int rc = check_matmul(who, a_rowptr, a_col, nnz_a, b_rowptr, b_col, nnz_b, m, k, n, narrow_cap, window_cols, rule);
    if (rc != SGL_OK) return rc;
    SGL_REQUIRE(mode == SGL_SPGEMM_SUM || mode == SGL_SPGEMM_ONES, "sgl_csr_matmul_fill: mode must be SGL_SPGEMM_SUM (0) or SGL_SPGEMM_ONES (1)");
    SGL_REQUIRE(mode == SGL_SPGEMM_ONES || (a_val && b_val), "sgl_csr_matmul_fill: NULL arguments (a_val, b_val are read under SGL_SPGEMM_SUM)");
    SGL_REQUIRE(d_out_rowptr && d_out_col && d_out_val, "sgl_csr_matmul_fill: NULL arguments (d_out_rowptr, d_out_col, d_out_val)");
    SGL_REQUIRE(aligned_to(a_val, 4) && aligned_to(b_val, 4) && aligned_to(d_out_rowptr, 8) && aligned_to(d_out_col, 4) && aligned_to(d_out_val, 4),
                "sgl_csr_matmul_fill: pointers must be aligned to their element size");
    if (m == 0 || k == 0 || n == 0 || nnz_a == 0 || nnz_b == 0) return SGL_OK;
    const Product P{{a_rowptr, a_col, nnz_a}, {b_rowptr, b_col, nnz_b}, m, k, n, mode, rule.narrow_cap};
    Tmp tmp;                                                         // freed when the entry returns: hipFree waits for the kernels
    return run_pass<true>(who, tmp, sgl::as_stream(stream), P, rule,
                          Pass{a_val, b_val, nullptr, nullptr, nullptr, d_out_rowptr, d_out_col, d_out_val});
}
