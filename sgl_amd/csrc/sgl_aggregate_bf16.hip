// Full-matrix aggregators over bfloat16 hop matrices (GraphOp(hop_dtype="bfloat16")): element-wise reductions,
// concat and the fused NAFS kernel read the stored bf16 hops in place -- no float32 copy of any hop is made.
//
// Numerics: a gathered element is widened exactly (bits << 16); from there on every kernel performs the operations of its float32
// counterpart in sgl_aggregate.hip in the same order (the NAFS kernel also in the same lane layout, sgl_rows.h), so each result is
// bit-identical to "widen every hop to float32, then run the float32 kernel".  Columns beyond d of a source row are the caller's
// padding: they may be read where a lane vector straddles column d inside the row's pitch, but are masked before any arithmetic.
#include "sgl_common.h"
#include "sgl_rows.h"

namespace {

typedef float f2 __attribute__((ext_vector_type(2)));
typedef uint32_t u2 __attribute__((ext_vector_type(2)));
typedef uint32_t u4 __attribute__((ext_vector_type(4)));

struct HopsB {
    const uint16_t *p[SGL_MAX_HOPS];
    int64_t ld[SGL_MAX_HOPS];
};

__device__ __forceinline__ float widen1(uint16_t b) { return __uint_as_float((uint32_t)b << 16); }
__device__ __forceinline__ float widen_lo(uint32_t w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float widen_hi(uint32_t w) { return __uint_as_float(w & 0xffff0000u); }

// BV consecutive bf16 of a row as one lane access: 16 / 8 / 4 / 2 bytes
template <int BV>
struct RawT;
template <>
struct RawT<8> {
    using type = u4;
};
template <>
struct RawT<4> {
    using type = u2;
};
template <>
struct RawT<2> {
    using type = uint32_t;
};
template <>
struct RawT<1> {
    using type = uint16_t;
};

// x[e] = float(p[col + e]) for col + e < d, 0 beyond.  `whole`: the BV elements from col on lie inside memory that belongs to the
// matrix (inside the d columns, or inside the pitch of a row that has a successor): one streaming vector load; otherwise (the
// vector that straddles column d in the LAST row) element by element, never past column d.
template <int BV>
__device__ __forceinline__ void load_bf16(const uint16_t *__restrict__ p, const int col, const int d, const bool whole, float (&x)[BV]) {
    if constexpr (BV == 1) {
        x[0] = widen1(__builtin_nontemporal_load(p + col));
    } else {
        if (whole) {
            const typename RawT<BV>::type r = __builtin_nontemporal_load(reinterpret_cast<const typename RawT<BV>::type *>(p + col));
            if constexpr (BV == 2) {
                x[0] = widen_lo(r);
                x[1] = widen_hi(r);
            } else {
#pragma unroll
                for (int k = 0; k < BV / 2; ++k) {
                    x[2 * k] = widen_lo(r[k]);
                    x[2 * k + 1] = widen_hi(r[k]);
                }
            }
            if (col + BV > d) {
#pragma unroll
                for (int e = 0; e < BV; ++e)
                    if (col + e >= d) x[e] = 0.f;
            }
        } else {
#pragma unroll
            for (int e = 0; e < BV; ++e) x[e] = (col + e < d) ? widen1(p[col + e]) : 0.f;
        }
    }
}

// BV floats to columns col .. col + BV of an output row, nothing at or beyond column dw; whole 16-byte (BV = 2: 8-byte) vectors where
// they fit (the launcher picked BV from the output's alignment), streaming stores
template <int BV>
__device__ __forceinline__ void store_f32(float *__restrict__ orow, const int col, const int dw, const float (&v)[BV]) {
    if constexpr (BV == 1) {
        __builtin_nontemporal_store(v[0], orow + col);
    } else if constexpr (BV == 2) {
        if (col + 2 <= dw) __builtin_nontemporal_store((f2){v[0], v[1]}, reinterpret_cast<f2 *>(orow + col));
        else orow[col] = v[0];
    } else {
#pragma unroll
        for (int k = 0; k < BV / 4; ++k) {
            const int c = col + 4 * k;
            if (c + 4 <= dw) {
                __builtin_nontemporal_store((f4){v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]}, reinterpret_cast<f4 *>(orow + c));
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (c + e < dw) orow[c + e] = v[4 * k + e];
            }
        }
    }
}

// ---- element-wise reductions over hops: hop_reduce_kernel (sgl_aggregate.hip) on bf16 inputs ---------------------------------------
// d data columns, dw >= d columns written: [d, dw) is the output row's own padding and is written as zeros.
template <int OP, int BV>
__global__ __launch_bounds__(256) void hop_reduce_bf16_kernel(const HopsB hx, const int n_hops, const float *__restrict__ w,
                                                              float *__restrict__ out, const int64_t ldo, const int64_t n,
                                                              const int d, const int dw) {
    const int lanes = (dw + BV - 1) / BV;
    const int64_t total = n * (int64_t)lanes;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int64_t row = i / lanes;
        const int col = (int)(i - row * lanes) * BV;
        float acc[BV];
#pragma unroll
        for (int e = 0; e < BV; ++e) acc[e] = 0.f;
        if (col < d) {
            const bool whole = col + BV <= d || row + 1 < n;
            float x[BV];
            load_bf16<BV>(hx.p[0] + row * hx.ld[0], col, d, whole, x);
            if constexpr (OP == SGL_REDUCE_SUM || OP == SGL_REDUCE_MEAN) {
                // Python sum() starts from int 0: 0 + X_s  (sum_message_op.py:10)
#pragma unroll
                for (int e = 0; e < BV; ++e) acc[e] = __fadd_rn(0.f, x[e]);
            } else if constexpr (OP == SGL_REDUCE_WSUM) {
                const float w0 = w[0];
#pragma unroll
                for (int e = 0; e < BV; ++e) acc[e] = __fmul_rn(x[e], w0);
            } else {
#pragma unroll
                for (int e = 0; e < BV; ++e) acc[e] = x[e];
            }
            for (int h = 1; h < n_hops; ++h) {
                load_bf16<BV>(hx.p[h] + row * hx.ld[h], col, d, whole, x);
                if constexpr (OP == SGL_REDUCE_SUM || OP == SGL_REDUCE_MEAN) {
#pragma unroll
                    for (int e = 0; e < BV; ++e) acc[e] = __fadd_rn(acc[e], x[e]);
                } else if constexpr (OP == SGL_REDUCE_MAX) {
#pragma unroll
                    for (int e = 0; e < BV; ++e) acc[e] = nan_max(acc[e], x[e]);
                } else if constexpr (OP == SGL_REDUCE_MIN) {
#pragma unroll
                    for (int e = 0; e < BV; ++e) acc[e] = nan_min(acc[e], x[e]);
                } else {  // WSUM: rounded product, then add (operators/utils.py:100-101: mul, then sum)
                    const float wh = w[h];
#pragma unroll
                    for (int e = 0; e < BV; ++e) acc[e] = __fadd_rn(acc[e], __fmul_rn(x[e], wh));
                }
            }
            if constexpr (OP == SGL_REDUCE_MEAN) {
                const float hf = (float)n_hops;
#pragma unroll
                for (int e = 0; e < BV; ++e) acc[e] = __fdiv_rn(acc[e], hf);  // true division
            }
            if (col + BV > d) {         // the output's pad columns are zeros whatever the weights are (0 * inf)
#pragma unroll
                for (int e = 0; e < BV; ++e)
                    if (col + e >= d) acc[e] = 0.f;
            }
        }
        store_f32<BV>(out + row * ldo, col, dw, acc);
    }
}

// ---- concat: out[:, h*d + k] = X_h[:, k], bf16 -> bf16 (bit patterns) or bf16 -> float32 (exact) -----------------------------------
// OB = bytes of an output element.  VEC = 4: a thread owns four consecutive output columns starting at a multiple of 4, stored as
// one 8-byte (bf16) / 16-byte (float32) vector.  Their sources are four consecutive elements of ONE hop row unless the group cuts a
// hop boundary; when d is not a multiple of 4 they start anywhere in that row: the two aligned 8-byte words that hold them are
// loaded and funnel-shifted (source rows are 8-byte aligned, pitches multiples of 4, so both words lie inside the row's pitch).
// Groups that cut a boundary, reach into the pad columns, or would read past column d of the last row go element by element.
// VEC = 1: one element per thread, any alignment.  width = n_hops * d, dw >= width: the columns written, [width, dw) as zeros.
template <int OB, int VEC>
__global__ __launch_bounds__(256) void hop_concat_bf16_kernel(const HopsB hx, void *__restrict__ out_, const int64_t ldo, const int64_t n,
                                                              const int d, const int width, const int dw) {
    const int lanes = (dw + VEC - 1) / VEC;
    const int64_t total = n * (int64_t)lanes;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int64_t row = i / lanes;
        const int c = (int)(i - row * lanes) * VEC;
        if constexpr (VEC == 1) {
            uint16_t b = 0;
            if (c < width) {
                const int h = c / d;
                b = hx.p[h][row * hx.ld[h] + (c - h * d)];
            }
            if constexpr (OB == 2) reinterpret_cast<uint16_t *>(out_)[row * ldo + c] = b;
            else reinterpret_cast<float *>(out_)[row * ldo + c] = widen1(b);
        } else {
            uint64_t bits = 0;      // element e of the group in bits 16 e .. 16 e + 15
            bool done = false;
            const int h = c / d;
            const int s = c - h * d;
            if (c + 4 <= width && s + 4 <= d) {
                const uint16_t *__restrict__ xr = hx.p[h] + row * hx.ld[h];
                const int s0 = s & ~3, sh = (s & 3) * 16;
                if (sh == 0) {
                    bits = *reinterpret_cast<const uint64_t *>(xr + s0);
                    done = true;
                } else if (s0 + 8 <= d || row + 1 < n) {
                    const uint64_t lo = *reinterpret_cast<const uint64_t *>(xr + s0);
                    const uint64_t hi = *reinterpret_cast<const uint64_t *>(xr + s0 + 4);
                    bits = (lo >> sh) | (hi << (64 - sh));
                    done = true;
                }
            }
            if (!done) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int cc = c + e;
                    if (cc < width) {
                        const int hh = cc / d;
                        bits |= (uint64_t)hx.p[hh][row * hx.ld[hh] + (cc - hh * d)] << (16 * e);
                    }
                }
            }
            const uint32_t b0 = (uint32_t)bits, b1 = (uint32_t)(bits >> 32);
            if constexpr (OB == 2) {
                uint16_t *__restrict__ orow = reinterpret_cast<uint16_t *>(out_) + row * ldo;
                if (c + 4 <= dw) {
                    __builtin_nontemporal_store((u2){b0, b1}, reinterpret_cast<u2 *>(orow + c));
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (c + e < dw) orow[c + e] = (uint16_t)(bits >> (16 * e));
                }
            } else {
                float *__restrict__ orow = reinterpret_cast<float *>(out_) + row * ldo;
                const float v[4] = {widen_lo(b0), widen_hi(b0), widen_lo(b1), widen_hi(b1)};
                store_f32<4>(orow, c, dw, v);
            }
        }
    }
}

// ---- fused NAFS: nafs_fused_kernel (sgl_aggregate.hip) reading bf16 hop rows ----------------------------------------------------------
// The same lane layout (lane l, chunk c owns the four elements of slot c * LPR + l -- here one 8-byte load, widened), the same
// reductions, per-row scalars, hop-ordered sums and store_row: out and W are bit-identical to the float32 kernel over widened
// copies of the hops.  (16-byte lanes of 8 elements would halve the load instructions but change which lane sums which products.)
__device__ __forceinline__ f4 load_bf16x4_masked(const uint16_t *__restrict__ p, const int c, const int d) {
    const u2 r = __builtin_nontemporal_load(reinterpret_cast<const u2 *>(p + c));
    f4 v = (f4){widen_lo(r[0]), widen_hi(r[0]), widen_lo(r[1]), widen_hi(r[1])};
    if (c + 4 > d) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (c + e >= d) v[e] = 0.f;
    }
    return v;
}

template <int LPR, int CH, int HMAX>
__global__ __launch_bounds__(256, ROWREG_MIN_BLOCKS(HMAX, CH)) void nafs_bf16_fused_kernel(const HopsB hx, const int n_hops, float *__restrict__ out,
                                                         const int64_t ldo, float *__restrict__ wout, const int64_t ldw,
                                                         const int64_t n, const int d, const int dw) {
    const auto [l, r, live] = row_lane<LPR>(n);
    f4 x[HMAX][CH];
    bool on[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) on[c] = chunk_on<LPR>(c, l, live, d);
    load_hop_rows<load_bf16x4_masked, LPR>(x, hx, n_hops, r, on, l, d);
    f4 acc[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) acc[c] = (f4){0.f, 0.f, 0.f, 0.f};
    if constexpr (HMAX <= LPR) {
        // lane l of the row's group collects <x_0, x_l> and |x_l|^2 and owns hop l from here on ("one hop per lane", sgl_rows.h)
        float dl = 0.f, ql = 0.f;
#pragma unroll
        for (int h = 0; h < HMAX; ++h)
            if (h < n_hops) {
                float dot, sq;
                dot_sq_chunks(x[0], x[h], dot, sq);
                dot = group_sum<LPR>(dot);
                sq = group_sum<LPR>(sq);
                dl = (l == h) ? dot : dl;
                ql = (l == h) ? sq : ql;
            }
        const bool mine = l < n_hops;
        const float nh = __fadd_rn(__fsqrt_rn(ql), 1e-10f);
        const float n0 = from_lane<LPR>(nh, 0);
        const float sc = mine ? __fdiv_rn(__fdiv_rn(dl, nh), n0) : -INFINITY;
        const float run_max = group_max<LPR>(sc);
        const float ex = mine ? expf(sc - run_max) : 0.f;
        float sum = 0.f;
#pragma unroll
        for (int h = 0; h < HMAX; ++h)
            if (h < n_hops) sum += from_lane<LPR>(ex, h);     // in hop order, like the sequential formulation
        const float wl = __fdiv_rn(ex, sum);
        if (wout && live && mine) wout[r * ldw + l] = wl;
#pragma unroll
        for (int h = 0; h < HMAX; ++h)
            if (h < n_hops) {
                const float w = from_lane<LPR>(wl, h);
#pragma unroll
                for (int c = 0; c < CH; ++c) acc[c] = mul_add4(acc[c], w, x[h][c]);
            }
    } else {
        float score[HMAX];
        float n0 = 0.f, run_max = -INFINITY;
#pragma unroll
        for (int h = 0; h < HMAX; ++h) {
            score[h] = -INFINITY;
            if (h < n_hops) {
                float dot, sq;
                dot_sq_chunks(x[0], x[h], dot, sq);
                dot = group_sum<LPR>(dot);
                sq = group_sum<LPR>(sq);
                const float nh = __fadd_rn(__fsqrt_rn(sq), 1e-10f);
                if (h == 0) n0 = nh;
                score[h] = __fdiv_rn(__fdiv_rn(dot, nh), n0);
                run_max = fmaxf(run_max, score[h]);
            }
        }
        float sum = 0.f;
#pragma unroll
        for (int h = 0; h < HMAX; ++h)
            if (h < n_hops) {
                score[h] = expf(score[h] - run_max);
                sum += score[h];
            }
#pragma unroll
        for (int h = 0; h < HMAX; ++h)
            if (h < n_hops) {
                const float w = __fdiv_rn(score[h], sum);
                if (wout && live && l == 0) wout[r * ldw + h] = w;
#pragma unroll
                for (int c = 0; c < CH; ++c) acc[c] = mul_add4(acc[c], w, x[h][c]);
            }
    }
    store_row<LPR, CH>(out + r * ldo, acc, l, live, d, dw);
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------
// what every entry checks before anything touches a device; the hop table for the kernels
int fill_hops_bf16(const char *who, HopsB &hx, int n_hops, const uint16_t *const *h_x, const int64_t *h_ldx, int64_t n, int64_t d) {
    if (n < 0 || d <= 0 || d >= INT32_MAX) return sgl::fail(SGL_ERR_INVALID, "%s: bad sizes (n=%lld, d=%lld)", who, (long long)n, (long long)d);
    SGL_REQUIRE_WIDTH(who, "d", d);
    return fill_hops(who, hx, n_hops, h_x, h_ldx, d, 2, nullptr);
}

// every hop row starts on a multiple of `bytes` (2 * elems): pointers aligned, pitches multiples of elems
bool hop_rows_aligned(const HopsB &hx, int n_hops, int elems) {
    for (int h = 0; h < n_hops; ++h)
        if (hx.ld[h] % elems != 0 || !aligned_to(hx.p[h], 2 * (size_t)elems)) return false;
    return true;
}

int concat_impl(const char *who, int ob, int n_hops, const uint16_t *const *h_x, const int64_t *h_ldx, void *d_out, int64_t ldo,
                int64_t pad_cols, int64_t n, int64_t d, void *stream) {
    HopsB hx;
    int rc = fill_hops_bf16(who, hx, n_hops, h_x, h_ldx, n, d);
    if (rc != SGL_OK) return rc;
    const int64_t width = d * n_hops;
    if (width >= INT32_MAX || pad_cols >= INT32_MAX - width) return sgl::fail(SGL_ERR_INVALID, "%s: rows of %lld columns are too wide", who, (long long)width);
    if (pad_cols >= 0) SGL_REQUIRE_WIDTH(who, "n_hops * d + pad_cols", width + pad_cols);
    if (pad_cols < 0 || width + pad_cols > ldo) return sgl::fail(SGL_ERR_INVALID, "%s: pad_cols=%lld does not fit the output pitch", who, (long long)pad_cols);
    if (!d_out || !aligned_to(d_out, (size_t)ob)) return sgl::fail(SGL_ERR_INVALID, "%s: bad output", who);
    for (int h = 0; h < n_hops; ++h)
        if ((const void *)hx.p[h] == (const void *)d_out) return sgl::fail(SGL_ERR_INVALID, "%s: the output aliases hop %d", who, h);
    if (n == 0) return SGL_OK;
    const int64_t dw = width + pad_cols;
    const bool fast = hop_rows_aligned(hx, n_hops, 4) && ldo % 4 == 0 && aligned_to(d_out, 4 * (size_t)ob);
    hipStream_t st = sgl::as_stream(stream);
    const int grid = stream_grid(n * (fast ? (dw + 3) / 4 : dw));
    with_one_of<2, 4>(ob, [&](auto OB) {
        with_vec(fast, [&](auto V) {
            hipLaunchKernelGGL((hop_concat_bf16_kernel<OB, V>), dim3(grid), dim3(256), 0, st, hx, d_out, ldo, n, (int)d, (int)width, (int)dw);
        });
    });
    return launch_check(who);
}

}  // namespace

SGL_EXPORT int sgl_hop_reduce_bf16_f32(int op, int n_hops, const uint16_t *const *h_x, const int64_t *h_ldx, const float *d_w,
                                       float *d_out, int64_t ldo, int64_t pad_cols, int64_t n, int64_t d, void *stream) {
    static const char *who = "sgl_hop_reduce_bf16_f32";
    SGL_REQUIRE(op >= SGL_REDUCE_SUM && op <= SGL_REDUCE_WSUM, "%s: unknown op %d", who, op);
    HopsB hx;
    int rc = fill_hops_bf16(who, hx, n_hops, h_x, h_ldx, n, d);
    if (rc != SGL_OK) return rc;
    SGL_REQUIRE(op != SGL_REDUCE_WSUM || d_w, "%s: WSUM needs device weights", who);
    SGL_REQUIRE(pad_cols >= 0 && pad_cols < INT32_MAX - d && d + pad_cols <= ldo, "%s: pad_cols=%lld does not fit the output pitch", who, (long long)pad_cols);
    SGL_REQUIRE(d_out && aligned_to(d_out, 4), "%s: bad output", who);
    SGL_REQUIRE_WIDTH(who, "d + pad_cols", d + pad_cols);
    if (n == 0) return SGL_OK;
    const int64_t dw = d + pad_cols;
    // lane width from alignment alone: the lane that straddles column d masks what lies beyond it
    int bv = 1;
    for (int b = 8; b > 1; b >>= 1) {
        const int ov = b < 4 ? b : 4;           // floats per output vector
        if (hop_rows_aligned(hx, n_hops, b) && ldo % ov == 0 && aligned_to(d_out, 4 * (size_t)ov)) {
            bv = b;
            break;
        }
    }
    hipStream_t st = sgl::as_stream(stream);
    const int grid = stream_grid(n * ((dw + bv - 1) / bv));
    with_one_of<SGL_REDUCE_SUM, SGL_REDUCE_MEAN, SGL_REDUCE_MAX, SGL_REDUCE_MIN, SGL_REDUCE_WSUM>(op, [&](auto OP) {
        with_one_of<8, 4, 2, 1>(bv, [&](auto BV) {
            hipLaunchKernelGGL((hop_reduce_bf16_kernel<OP, BV>), dim3(grid), dim3(256), 0, st, hx, n_hops, d_w, d_out, ldo, n, (int)d, (int)dw);
        });
    });
    SGL_LAUNCH_CHECK("sgl_hop_reduce_bf16_f32");
    return SGL_OK;
}

SGL_EXPORT int sgl_hop_concat_bf16(int n_hops, const uint16_t *const *h_x, const int64_t *h_ldx, uint16_t *d_out, int64_t ldo,
                                   int64_t pad_cols, int64_t n, int64_t d, void *stream) {
    return concat_impl("sgl_hop_concat_bf16", 2, n_hops, h_x, h_ldx, d_out, ldo, pad_cols, n, d, stream);
}

SGL_EXPORT int sgl_hop_concat_bf16_f32(int n_hops, const uint16_t *const *h_x, const int64_t *h_ldx, float *d_out, int64_t ldo,
                                       int64_t pad_cols, int64_t n, int64_t d, void *stream) {
    return concat_impl("sgl_hop_concat_bf16_f32", 4, n_hops, h_x, h_ldx, d_out, ldo, pad_cols, n, d, stream);
}

SGL_EXPORT int sgl_nafs_bf16_f32(int n_hops, const uint16_t *const *h_x, const int64_t *h_ldx, float *d_out, int64_t ldo,
                                 int64_t pad_cols, float *d_w_out, int64_t ldw, int64_t n, int64_t d, void *stream) {
    static const char *who = "sgl_nafs_bf16_f32";
    HopsB hx;
    int rc = fill_hops_bf16(who, hx, n_hops, h_x, h_ldx, n, d);
    if (rc != SGL_OK) return rc;
    rc = sgl::check_pad(who, d, pad_cols, ldo);
    if (rc != SGL_OK) return rc;
    SGL_REQUIRE(d_out && aligned_to(d_out, 4), "%s: bad output", who);
    SGL_REQUIRE(!d_w_out || ldw >= n_hops, "%s: the weight matrix needs a pitch of at least n_hops", who);
    if (n == 0) return SGL_OK;
    // the register-resident kernel or nothing: there is no two-pass bf16 form
    if (n_hops > 16 || d > 512)
        return sgl::fail(SGL_ERR_UNSUPPORTED, "%s: more than 16 hops or rows of more than 512 columns: widen the hops and use sgl_nafs_padded_f32", who);
    if (!hop_rows_aligned(hx, n_hops, 4))
        return sgl::fail(SGL_ERR_UNSUPPORTED, "%s: hop rows must be 8-byte aligned on pitches that are multiples of 4: widen the hops and use sgl_nafs_padded_f32", who);
    if (ldo % 4 != 0 || !aligned_to(d_out, 16))
        return sgl::fail(SGL_ERR_UNSUPPORTED, "%s: the output needs 16-byte aligned rows on a pitch that is a multiple of 4: widen the hops and use sgl_nafs_padded_f32", who);
    if (sgl::tuning("nafs_fused", 1) == 0)
        return sgl::fail(SGL_ERR_UNSUPPORTED, "%s: the fused kernel is switched off (nafs_fused = 0): widen the hops and use sgl_nafs_padded_f32", who);
    hipStream_t st = sgl::as_stream(stream);
    return launch_row_instance({who, who, who}, sgl::row_instance(d, n_hops), n_hops, n, [&](dim3 grid, auto L, auto C, auto HM) {
        hipLaunchKernelGGL((nafs_bf16_fused_kernel<L, C, HM>), grid, dim3(256), 0, st, hx, n_hops, d_out, ldo, d_w_out, ldw, n, (int)d,
                           sgl::out_cols(d, pad_cols, L * C * 4));
    });
}
