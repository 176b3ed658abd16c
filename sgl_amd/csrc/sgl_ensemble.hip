// K16: the sub-graph ensemble aggregators of the heterogeneous models (include/sgl_ensemble.h).  The reference gathers x[idx] from M
// matrices, stacks them, multiplies by a broadcast weight and takes a mean (simple_models.py:5-84): about 7 M + H matrices of [B, d]
// through memory for M read and H written.  Here a lane owns one 16-byte column chunk of an output row and walks the members of the
// row's group: the loads of a batch of kMembersInFlight members are issued before the first is used, the sum is the fma chain the header
// defines, the output row is written once, whole vectors non-temporal.  Nothing is register-resident per row, so d has no limit of
// its own.
#include <algorithm>

#include "../../include/sgl_ensemble.h"
#include "sgl_common.h"
#include "sgl_rows.h"

namespace {

constexpr int kMembersInFlight = 8;      // row loads of one lane issued before the first use
constexpr int kBwdMaxBlocks = 1024;      // row ranges of the weight gradient's first level
constexpr int kBwdRowStep = 32;          // a range is a whole number of these (the most rows a workgroup takes per step: 8 lanes per row)

// the matrices (or incoming gradients) and the outputs of ONE launch: whole groups, at most SGL_MAX_HOPS members
struct Members {
    const float *p[SGL_MAX_HOPS];
    int64_t ld[SGL_MAX_HOPS];
};
struct Outs {
    float *p[SGL_MAX_HOPS];
    int64_t ld[SGL_MAX_HOPS];
};

// row i of the result reads row `idx[i]` (python-style negative indices) or row i; bad: outside the matrix -- then row 0 is named and
// nothing may be loaded through it (the matrix may have no rows at all)
__device__ __forceinline__ int64_t source_row(const int64_t *__restrict__ idx, const int64_t i, const int64_t n_rows, bool &bad) {
    int64_t s = idx ? idx[i] : i;
    if (s < 0) s += n_rows;
    bad = s < 0 || s >= n_rows;
    return bad ? 0 : s;
}

template <int VEC>
__device__ __forceinline__ typename Vt<VEC>::type splat(const float v) {
    if constexpr (VEC == 4) return (f4){v, v, v, v};
    else return v;
}

// weights of member row `wrow` for the columns from c.  WM 0: one per matrix; 1: one per column, element loads; 2: one per column, a
// 16-byte load (VEC == 4; the table's rows are 16-byte vectors that cover round_up(d, 4) columns)
template <int VEC, int WM>
__device__ __forceinline__ typename Vt<VEC>::type load_weights(const float *__restrict__ wrow, const int c, const int d) {
    if constexpr (WM == 0) {
        return splat<VEC>(wrow[0]);
    } else if constexpr (VEC == 1) {
        return wrow[c];
    } else if constexpr (WM == 2) {
        return *reinterpret_cast<const f4 *>(wrow + c);
    } else {
        f4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (c + e < d) ? wrow[c + e] : 0.f;
        return v;
    }
}

// Forward.  Grid: x strides over blocks of 256 / lpr output rows, y = the group (of this launch).  lg = log2(lanes per row).
template <int VEC, int WM>
__global__ __launch_bounds__(256) void ensemble_combine_kernel(const Members mx, const Outs mo, const int gs, const float *__restrict__ w,
                                                               const int64_t ldw, const float divisor, const int64_t n_rows,
                                                               const int64_t *__restrict__ idx, const int64_t n_out, const int d,
                                                               const int dw, const int lg, const int64_t n_blocks) {
    using V = typename Vt<VEC>::type;
    const int lpr = 1 << lg, rpb = 256 >> lg;
    const int l = threadIdx.x & (lpr - 1);
    const int g = blockIdx.y;
    float *__restrict__ out = mo.p[g];
    const int64_t ldo = mo.ld[g];
    const float *__restrict__ wg = w + (int64_t)g * gs * ldw;
    const bool divide = divisor != 1.f;
    for (int64_t rb = blockIdx.x; rb < n_blocks; rb += gridDim.x) {
        const int64_t i = rb * rpb + (threadIdx.x >> lg);
        if (i >= n_out) continue;
        bool bad;
        const int64_t src = source_row(idx, i, n_rows, bad);
        const bool last = src == n_rows - 1;
        for (int c = l * VEC; c < dw; c += lpr * VEC) {
            V acc = splat<VEC>(0.f);
            if (c < d) {
                if (bad) {
                    acc = splat<VEC>(__uint_as_float(0x7fc00000u));
                } else {
                    for (int sb = 0; sb < gs; sb += kMembersInFlight) {
                        V x[kMembersInFlight], wv[kMembersInFlight];
#pragma unroll
                        for (int k = 0; k < kMembersInFlight; ++k) {
                            const int s = sb + k < gs ? sb + k : gs - 1;      // (clamped: the surplus loads of the last batch are not used)
                            const int m = g * gs + s;
                            x[k] = edge_load<VEC>(mx.p[m] + src * mx.ld[m], c, d, last);
                            wv[k] = load_weights<VEC, WM>(wg + (int64_t)s * ldw, c, d);
                        }
#pragma unroll
                        for (int k = 0; k < kMembersInFlight; ++k) {
                            if (sb + k < gs) {
                                if constexpr (VEC == 4) {
#pragma unroll
                                    for (int e = 0; e < 4; ++e)
                                        acc[e] = (sb + k == 0) ? __fmul_rn(x[k][e], wv[k][e]) : __builtin_fmaf(x[k][e], wv[k][e], acc[e]);
                                } else {
                                    acc = (sb + k == 0) ? __fmul_rn(x[k], wv[k]) : __builtin_fmaf(x[k], wv[k], acc);
                                }
                            }
                        }
                    }
                    if (divide) {
                        if constexpr (VEC == 4) {
#pragma unroll
                            for (int e = 0; e < 4; ++e) acc[e] = acc[e] / divisor;
                        } else {
                            acc = acc / divisor;
                        }
                    }
                }
                if constexpr (VEC == 4) {       // what lies beyond d is the row's padding: zeros, whatever the weight table holds there
                    if (c + 4 > d) {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (c + e >= d) acc[e] = 0.f;
                    }
                }
            }
            float *o = out + i * ldo + c;
            if constexpr (VEC == 4) {
                if (c + 4 <= dw) {
                    __builtin_nontemporal_store(acc, reinterpret_cast<f4 *>(o));
                } else {                        // dw == d, the vector straddles it: never write past the caller's d columns
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (c + e < dw) o[e] = acc[e];
                }
            } else {
                __builtin_nontemporal_store(acc, o);
            }
        }
    }
}

// Weight gradient, first level, one weight per matrix and column.  Workgroup (x, y): rows [x * per_block, ...) of group y.  A lane
// owns a column chunk and keeps the partial sums of a batch of members over its rows (every rpb-th row of the range,
// one fma chain in row order); the rpb lanes of a chunk are then added through LDS in lane order.  scratch: [blocks][m_total][dp].
template <int VEC>
__global__ __launch_bounds__(256) void ensemble_bwd_cols_kernel(const Members mx, const Members mg, const int gs, const int m0,
                                                                const int m_total, const int64_t n_rows, const int64_t *__restrict__ idx,
                                                                const int64_t n_out, const int d, const int dp, const int lg,
                                                                const int64_t per_block, float *__restrict__ scratch) {
    using V = typename Vt<VEC>::type;
    __shared__ V red[256];
    const int t = threadIdx.x;
    const int lpr = 1 << lg, rpb = 256 >> lg;
    const int l = t & (lpr - 1), rl = t >> lg;
    const int g = blockIdx.y;
    const float *__restrict__ gp = mg.p[g];
    const int64_t ldg = mg.ld[g];
    const int64_t r0 = (int64_t)blockIdx.x * per_block, r1 = min(r0 + per_block, n_out);
    const int n_chunks = (d + lpr * VEC - 1) / (lpr * VEC);
    for (int ci = 0; ci < n_chunks; ++ci) {
        const int c = (ci * lpr + l) * VEC;
        const bool on = c < d;
        for (int sb = 0; sb < gs; sb += kMembersInFlight) {
            V acc[kMembersInFlight];
#pragma unroll
            for (int k = 0; k < kMembersInFlight; ++k) acc[k] = splat<VEC>(0.f);
            if (on) {
#pragma unroll 1
                for (int64_t r = r0 + rl; r < r1; r += rpb) {
                    bool bad;
                    const int64_t src = source_row(idx, r, n_rows, bad);
                    const bool last = src == n_rows - 1;
                    const V gv = edge_load<VEC>(gp + r * ldg, c, d, r == n_out - 1);
                    V x[kMembersInFlight];
#pragma unroll
                    for (int k = 0; k < kMembersInFlight; ++k) {
                        const int m = g * gs + (sb + k < gs ? sb + k : gs - 1);
                        x[k] = bad ? splat<VEC>(__uint_as_float(0x7fc00000u)) : edge_load<VEC>(mx.p[m] + src * mx.ld[m], c, d, last);
                    }
#pragma unroll
                    for (int k = 0; k < kMembersInFlight; ++k) {
                        if constexpr (VEC == 4) {
#pragma unroll
                            for (int e = 0; e < 4; ++e) acc[k][e] = __builtin_fmaf(gv[e], x[k][e], acc[k][e]);
                        } else {
                            acc[k] = __builtin_fmaf(gv, x[k], acc[k]);
                        }
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < kMembersInFlight; ++k) {
                if (sb + k < gs) {                  // (the same for every thread of the workgroup)
                    red[t] = acc[k];
                    __syncthreads();
                    if (rl == 0 && on) {
                        V s = red[l];
                        for (int q = 1; q < rpb; ++q) s += red[q * lpr + l];
                        *reinterpret_cast<V *>(scratch + ((int64_t)blockIdx.x * m_total + m0 + g * gs + sb + k) * dp + c) = s;
                    }
                    __syncthreads();
                }
            }
        }
    }
}

// ... one weight per matrix: the lane's chain runs over its columns as well (chunk, row, element order), then the 64 lanes of a
// wavefront (fixed butterfly) and the four wavefronts.  scratch: [blocks][m_total].
template <int VEC>
__global__ __launch_bounds__(256) void ensemble_bwd_scalar_kernel(const Members mx, const Members mg, const int gs, const int m0,
                                                                  const int m_total, const int64_t n_rows, const int64_t *__restrict__ idx,
                                                                  const int64_t n_out, const int d, const int lg, const int64_t per_block,
                                                                  float *__restrict__ scratch) {
    using V = typename Vt<VEC>::type;
    __shared__ float red[4][kMembersInFlight];
    const int t = threadIdx.x;
    const int lpr = 1 << lg, rpb = 256 >> lg;
    const int l = t & (lpr - 1), rl = t >> lg;
    const int g = blockIdx.y;
    const float *__restrict__ gp = mg.p[g];
    const int64_t ldg = mg.ld[g];
    const int64_t r0 = (int64_t)blockIdx.x * per_block, r1 = min(r0 + per_block, n_out);
    const int n_chunks = (d + lpr * VEC - 1) / (lpr * VEC);
    for (int sb = 0; sb < gs; sb += kMembersInFlight) {
        float acc[kMembersInFlight];
#pragma unroll
        for (int k = 0; k < kMembersInFlight; ++k) acc[k] = 0.f;
        for (int ci = 0; ci < n_chunks; ++ci) {
            const int c = (ci * lpr + l) * VEC;
            if (c >= d) continue;
#pragma unroll 1
            for (int64_t r = r0 + rl; r < r1; r += rpb) {
                bool bad;
                const int64_t src = source_row(idx, r, n_rows, bad);
                const bool last = src == n_rows - 1;
                const V gv = edge_load<VEC>(gp + r * ldg, c, d, r == n_out - 1);
                V x[kMembersInFlight];
#pragma unroll
                for (int k = 0; k < kMembersInFlight; ++k) {
                    const int m = g * gs + (sb + k < gs ? sb + k : gs - 1);
                    x[k] = bad ? splat<VEC>(__uint_as_float(0x7fc00000u)) : edge_load<VEC>(mx.p[m] + src * mx.ld[m], c, d, last);
                }
#pragma unroll
                for (int k = 0; k < kMembersInFlight; ++k) {
                    if constexpr (VEC == 4) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc[k] = __builtin_fmaf(gv[e], x[k][e], acc[k]);
                    } else {
                        acc[k] = __builtin_fmaf(gv, x[k], acc[k]);
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < kMembersInFlight; ++k) acc[k] = group_sum<64>(acc[k]);
        __syncthreads();
        if ((t & 63) == 0) {
#pragma unroll
            for (int k = 0; k < kMembersInFlight; ++k) red[t >> 6][k] = acc[k];
        }
        __syncthreads();
        if (t < kMembersInFlight && sb + t < gs)
            scratch[(int64_t)blockIdx.x * m_total + m0 + g * gs + sb + t] = (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]);
    }
}

// second level: one wavefront per (matrix, 16-byte column slot) resp. per matrix: lane l adds the partials of blocks l, l + 64, ... in
// that order, a fixed butterfly folds the 64 lanes, then the one true division -- the same bits for a given block count
__global__ __launch_bounds__(64) void ensemble_bwd_cols_final_kernel(const float *__restrict__ scratch, const int n_blocks, const int m_total,
                                                                     const int slots, const float divisor, float *__restrict__ dw,
                                                                     const int64_t lddw, const int d) {
    const int m = blockIdx.x / slots, slot = blockIdx.x - m * slots;
    const int dp = slots * 4;
    f4 s = (f4){0.f, 0.f, 0.f, 0.f};
    for (int b = threadIdx.x; b < n_blocks; b += 64) {
        const f4 o = *reinterpret_cast<const f4 *>(scratch + ((int64_t)b * m_total + m) * dp + slot * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) s[e] += o[e];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) s[e] = group_sum<64>(s[e]);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (slot * 4 + e < d) dw[(int64_t)m * lddw + slot * 4 + e] = divisor != 1.f ? s[e] / divisor : s[e];
    }
}
__global__ __launch_bounds__(64) void ensemble_bwd_scalar_final_kernel(const float *__restrict__ scratch, const int n_blocks, const int m_total,
                                                                       const float divisor, float *__restrict__ dw, const int64_t lddw) {
    const int m = blockIdx.x;
    float s = 0.f;
    for (int b = threadIdx.x; b < n_blocks; b += 64) s += scratch[(int64_t)b * m_total + m];
    s = group_sum<64>(s);
    if (threadIdx.x == 0) dw[(int64_t)m * lddw] = divisor != 1.f ? s / divisor : s;
}

int log2_of(int lpr) { return lpr == 8 ? 3 : lpr == 16 ? 4 : lpr == 32 ? 5 : 6; }

// rows of one first-level range and the number of ranges: functions of n_idx alone (the scratch query knows nothing else)
int64_t bwd_per_block(int64_t n_idx) {
    const int64_t per = (n_idx + kBwdMaxBlocks - 1) / kBwdMaxBlocks;
    return per <= kBwdRowStep ? kBwdRowStep : (per + kBwdRowStep - 1) / kBwdRowStep * kBwdRowStep;
}
int64_t bwd_blocks(int64_t n_idx) { return (n_idx + bwd_per_block(n_idx) - 1) / bwd_per_block(n_idx); }

// what both entry points ask of their common arguments; M by name
int check_shape(const char *who, int n_groups, int group_size, int64_t n_rows, const int64_t *d_idx, int64_t n_idx, int cs, float divisor,
                int64_t d, int64_t pad) {
    SGL_REQUIRE(n_groups >= 1 && group_size >= 1, "%s: n_groups=%d and group_size=%d must be positive", who, n_groups, group_size);
    if (group_size > SGL_ENSEMBLE_MAX_GROUP)
        return sgl::fail(SGL_ERR_UNSUPPORTED, "%s: group_size=%d is more than SGL_ENSEMBLE_MAX_GROUP=%d (split the group)", who, group_size,
                         SGL_ENSEMBLE_MAX_GROUP);
    if ((int64_t)n_groups * group_size > SGL_ENSEMBLE_MAX_MEMBERS)
        return sgl::fail(SGL_ERR_UNSUPPORTED, "%s: n_groups * group_size=%lld matrices are more than SGL_ENSEMBLE_MAX_MEMBERS=%d (split by group)",
                         who, (long long)n_groups * group_size, SGL_ENSEMBLE_MAX_MEMBERS);
    SGL_REQUIRE(n_rows >= 0 && n_idx >= 0 && d >= 0 && pad >= 0, "%s: bad sizes", who);
    SGL_REQUIRE_WIDTH(who, pad ? "d + pad_cols" : "d", d + pad);
    SGL_REQUIRE(cs == 0 || cs == 1, "%s: cs=%d is neither 0 nor 1", who, cs);
    SGL_REQUIRE(divisor == divisor && divisor != 0.f, "%s: divisor must be a non-zero number", who);
    SGL_REQUIRE(d_idx || n_idx == n_rows, "%s: without an index n_idx must be n_rows", who);
    SGL_REQUIRE(aligned_to(d_idx, 8), "%s: d_idx not 8-byte aligned", who);
    return SGL_OK;
}

// The table of one launch from the caller's arrays, entries [first, first + count): fill_hops' checks and its row-layout rule
// (sgl_rows.h: *vec4 is cleared where a matrix's rows are not 16-byte vectors)
template <typename Table, typename T>
int fill_table(const char *who, Table &t, int first, int count, const T *const *h_p, const int64_t *h_ld, int64_t d, bool *vec4) {
    return fill_hops(who, t, count, h_p + first, h_ld ? h_ld + first : nullptr, d, 4, vec4);
}

}  // namespace

SGL_EXPORT int sgl_ensemble_combine_f32(int n_groups, int group_size, const float *const *h_x, const int64_t *h_ldx, int64_t n_rows,
                                        const int64_t *d_idx, int64_t n_idx, const float *d_w, int64_t ldw, int cs, float divisor,
                                        float *const *h_out, const int64_t *h_ldo, int64_t pad_cols, int64_t d, void *stream) {
    const char *who = "sgl_ensemble_combine_f32";
    int rc = check_shape(who, n_groups, group_size, n_rows, d_idx, n_idx, cs, divisor, d, pad_cols);
    if (rc != SGL_OK) return rc;
    if (n_idx == 0 || d == 0) return SGL_OK;
    const int m_total = n_groups * group_size;
    SGL_REQUIRE(h_x && h_out && d_w, "%s: NULL arguments", who);
    SGL_REQUIRE(aligned_to(d_w, 4) && ldw >= (cs ? d : 1), "%s: weight table misaligned or ldw=%lld too small", who, (long long)ldw);
    const int64_t dw = d + pad_cols;
    // the layout of the whole call, before the first launch: every matrix and every output by the one rule
    bool vec4 = true;
    for (int g = 0; g < n_groups; ++g) {
        SGL_REQUIRE(h_out[g] && aligned_to(h_out[g], 4), "%s: output %d: NULL or misaligned", who, g);
        const int64_t ldo = h_ldo ? h_ldo[g] : dw;
        rc = sgl::check_pad(who, d, pad_cols, ldo);
        if (rc != SGL_OK) return rc;
        if (ldo % 4 != 0 || !aligned_to(h_out[g], 16)) vec4 = false;
    }
    {
        Members probe;
        for (int a = 0; a < m_total; a += SGL_MAX_HOPS) {
            rc = fill_table(who, probe, a, std::min(SGL_MAX_HOPS, m_total - a), h_x, h_ldx, d, &vec4);
            if (rc != SGL_OK) return rc;
        }
    }
    const int wm = cs == 0 ? 0 : ((vec4 && ldw % 4 == 0 && ldw >= (d + 3) / 4 * 4 && aligned_to(d_w, 16)) ? 2 : 1);
    const int vec = vec4 ? 4 : 1;
    const int lpr = sgl::pick_lpr(dw, vec);
    const int lg = log2_of(lpr);
    const int64_t n_blocks = (n_idx + (256 / lpr) - 1) / (256 / lpr);
    const int64_t gx = stream_grid(n_blocks * 256);            // capped like the streaming aggregators (tuning key agg_blocks): the kernel strides
    hipStream_t st = sgl::as_stream(stream);
    const int groups_per_launch = SGL_MAX_HOPS / group_size;   // whole groups, at most SGL_MAX_HOPS matrices in a launch's table
    for (int g0 = 0; g0 < n_groups; g0 += groups_per_launch) {
        const int ng = std::min(groups_per_launch, n_groups - g0);
        Members mx;
        Outs mo;
        bool ignored = true;
        rc = fill_table(who, mx, g0 * group_size, ng * group_size, h_x, h_ldx, d, &ignored);
        if (rc != SGL_OK) return rc;
        for (int k = 0; k < SGL_MAX_HOPS; ++k) {
            mo.p[k] = k < ng ? h_out[g0 + k] : nullptr;
            mo.ld[k] = k < ng ? (h_ldo ? h_ldo[g0 + k] : dw) : 0;
        }
        if (!sgl::launch_fits(gx * ng, 256)) return sgl::fail(SGL_ERR_UNSUPPORTED, "%s: too many rows for one launch", who);
        const float *w0 = d_w + (int64_t)g0 * group_size * ldw;
        const dim3 grid((unsigned)gx, (unsigned)ng);
        with_vec(vec4, [&](auto V) {
            with_one_of<0, 1, 2>(wm, [&](auto WM) {
                if constexpr (decltype(V)::value == 1 && decltype(WM)::value == 2) return;       // (wm = 2 only with 16-byte rows)
                else
                    hipLaunchKernelGGL((ensemble_combine_kernel<V, WM>), grid, dim3(256), 0, st, mx, mo, group_size, w0, ldw, divisor, n_rows, d_idx,
                                       n_idx, (int)d, (int)dw, lg, n_blocks);
            });
        });
        SGL_LAUNCH_CHECK(who);
    }
    return SGL_OK;
}

SGL_EXPORT int64_t sgl_ensemble_combine_bwd_scratch(int n_groups, int group_size, int64_t n_idx, int64_t d, int cs) {
    if (n_groups < 1 || group_size < 1 || n_idx < 1 || d < 1) return 4;
    return bwd_blocks(n_idx) * n_groups * group_size * (cs ? (d + 3) / 4 * 4 : 1);
}

SGL_EXPORT int sgl_ensemble_combine_bwd_f32(int n_groups, int group_size, const float *const *h_x, const int64_t *h_ldx, int64_t n_rows,
                                            const int64_t *d_idx, int64_t n_idx, const float *const *h_dout, const int64_t *h_lddo, int cs,
                                            float divisor, float *d_dw, int64_t lddw, float *d_scratch, int64_t d, void *stream) {
    const char *who = "sgl_ensemble_combine_bwd_f32";
    int rc = check_shape(who, n_groups, group_size, n_rows, d_idx, n_idx, cs, divisor, d, 0);
    if (rc != SGL_OK) return rc;
    const int m_total = n_groups * group_size;
    SGL_REQUIRE(d_dw && aligned_to(d_dw, 4) && lddw >= (cs ? d : 1), "%s: d_dw NULL, misaligned or lddw=%lld too small", who, (long long)lddw);
    hipStream_t st = sgl::as_stream(stream);
    if (d == 0) return SGL_OK;
    if (n_idx == 0) {                                          // empty sums
        SGL_HIP_CHECK(hipMemset2DAsync(d_dw, (size_t)lddw * sizeof(float), 0, (size_t)(cs ? d : 1) * sizeof(float), (size_t)m_total, st));
        return SGL_OK;
    }
    SGL_REQUIRE(h_x && h_dout && d_scratch && aligned_to(d_scratch, 16), "%s: NULL arguments or d_scratch not 16-byte aligned", who);
    bool vec4 = true;
    {
        Members probe;
        for (int a = 0; a < m_total; a += SGL_MAX_HOPS) {
            rc = fill_table(who, probe, a, std::min(SGL_MAX_HOPS, m_total - a), h_x, h_ldx, d, &vec4);
            if (rc != SGL_OK) return rc;
        }
        for (int a = 0; a < n_groups; a += SGL_MAX_HOPS) {
            rc = fill_table(who, probe, a, std::min(SGL_MAX_HOPS, n_groups - a), h_dout, h_lddo, d, &vec4);
            if (rc != SGL_OK) return rc;
        }
    }
    const int vec = vec4 ? 4 : 1;
    const int lpr = sgl::pick_lpr(d, vec);
    const int lg = log2_of(lpr);
    const int64_t per_block = bwd_per_block(n_idx), blocks = bwd_blocks(n_idx);
    const int64_t dp = (d + 3) / 4 * 4;
    const int64_t finals = cs ? (int64_t)m_total * (dp / 4) : m_total;
    if (!sgl::launch_fits(finals, 64)) return sgl::fail(SGL_ERR_UNSUPPORTED, "%s: d=%lld is too wide for one launch of the second level", who, (long long)d);
    const int groups_per_launch = SGL_MAX_HOPS / group_size;
    for (int g0 = 0; g0 < n_groups; g0 += groups_per_launch) {
        const int ng = std::min(groups_per_launch, n_groups - g0);
        Members mx, mg;
        bool ignored = true;
        rc = fill_table(who, mx, g0 * group_size, ng * group_size, h_x, h_ldx, d, &ignored);
        if (rc != SGL_OK) return rc;
        rc = fill_table(who, mg, g0, ng, h_dout, h_lddo, d, &ignored);
        if (rc != SGL_OK) return rc;
        const dim3 grid((unsigned)blocks, (unsigned)ng);
        with_vec(vec4, [&](auto V) {
            if (cs)
                hipLaunchKernelGGL((ensemble_bwd_cols_kernel<V>), grid, dim3(256), 0, st, mx, mg, group_size, g0 * group_size, m_total, n_rows, d_idx,
                                   n_idx, (int)d, (int)dp, lg, per_block, d_scratch);
            else
                hipLaunchKernelGGL((ensemble_bwd_scalar_kernel<V>), grid, dim3(256), 0, st, mx, mg, group_size, g0 * group_size, m_total, n_rows, d_idx,
                                   n_idx, (int)d, lg, per_block, d_scratch);
        });
        SGL_LAUNCH_CHECK(who);
    }
    if (cs)
        hipLaunchKernelGGL(ensemble_bwd_cols_final_kernel, dim3((unsigned)finals), dim3(64), 0, st, d_scratch, (int)blocks, m_total, (int)(dp / 4), divisor,
                           d_dw, lddw, (int)d);
    else
        hipLaunchKernelGGL(ensemble_bwd_scalar_final_kernel, dim3((unsigned)finals), dim3(64), 0, st, d_scratch, (int)blocks, m_total, divisor, d_dw, lddw);
    SGL_LAUNCH_CHECK(who);
    return SGL_OK;
}
