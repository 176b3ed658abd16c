// Device helpers and typed launch dispatch of the row kernels, shared by sgl_aggregate.hip (float32 hops), sgl_aggregate_bf16.hip
// (bfloat16 hops), sgl_edge.hip and the loss / k-means kernels (K9, K11, K12, K14): both aggregator files must pick the same lane
// layout and sum in the same lane order for their results to be bit-identical, so the in-wavefront reductions exist once, here, and
// the layout rules once in sgl_core.cpp (sgl::row_layout / sgl::row_instance / sgl::slice_instance: pure host arithmetic, checked on
// the CPU).  Not part of the ABI.
#pragma once
#include <type_traits>

#include "sgl_common.h"

namespace {

using f4 = float __attribute__((ext_vector_type(4)));

template <int VEC>
struct Vt;
template <>
struct Vt<1> {
    using type = float;
};
template <>
struct Vt<4> {
    using type = f4;
};

__device__ __forceinline__ float nan_max(float r, float x) { return (x > r || x != x) ? x : r; }
__device__ __forceinline__ float nan_min(float r, float x) { return (x < r || x != x) ? x : r; }

// 16-byte row accesses are legal for any d when every row pitch is a multiple of 4 floats (the vector that
// straddles column d stays inside the row's own padding); the elements beyond d are masked out of reductions.
// NT: streaming (non-temporal) hint -- every hop element is read exactly once; measured +3-10 % on the elementwise and
// fused-NAFS kernels, neutral-to-negative on the row-dot and concat kernels, which therefore do not use it
// (profiles/r02_aggregators.log).
template <int VEC, bool NT = false>
__device__ __forceinline__ typename Vt<VEC>::type load_masked(const float *p, int c, int d) {
    using V = typename Vt<VEC>::type;
    V v = NT ? __builtin_nontemporal_load(reinterpret_cast<const V *>(p + c)) : *reinterpret_cast<const V *>(p + c);
    if constexpr (VEC == 4) {
        if (c + 4 > d) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (c + e >= d) v[e] = 0.f;
        }
    }
    return v;
}

// The vector of row `p` at column c where the pad may not be read (sgl_edge.hip, sgl_kmeans.hip): whole when it lies inside the row's d columns or (not the last row) inside its pitch
template <int VEC>
__device__ __forceinline__ typename Vt<VEC>::type edge_load(const float *__restrict__ p, const int c, const int d, const bool last_row) {
    if constexpr (VEC == 4) {
        f4 v;
        if (c + 4 <= d) {
            v = *reinterpret_cast<const f4 *>(p + c);
        } else if (!last_row) {
            v = *reinterpret_cast<const f4 *>(p + c);
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (c + e >= d) v[e] = 0.f;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = (c + e < d) ? p[c + e] : 0.f;
        }
        return v;
    } else {
        return p[c];
    }
}

// ---- the per-VEC column helpers of the loss / k-means kernels (K9, K11, K12, K14) ---------------------------------------------------
template <int VEC>
__device__ __forceinline__ typename Vt<VEC>::type vzero() {
    if constexpr (VEC == 4) return f4{0.f, 0.f, 0.f, 0.f};
    else return 0.f;
}

// columns col .. col + VEC - 1 of an output row, never beyond column d; `ovec`: the row is made of 16-byte vectors
template <int VEC>
__device__ __forceinline__ void store_cols(float *__restrict__ orow, const int col, const int d, const typename Vt<VEC>::type v,
                                           const bool ovec = true) {
    if constexpr (VEC == 4) {
        if (ovec && col + 4 <= d) {
            *reinterpret_cast<f4 *>(orow + col) = v;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (col + e < d) orow[col + e] = v[e];
        }
    } else {
        orow[col] = v;
    }
}
template <int VEC>
__device__ __forceinline__ typename Vt<VEC>::type load_cols(const float *orow, const int col, const int d, const bool ovec = true) {
    if constexpr (VEC == 4) {
        if (ovec && col + 4 <= d) return *reinterpret_cast<const f4 *>(orow + col);
        f4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (col + e < d) ? orow[col + e] : 0.f;
        return v;
    } else {
        return orow[col];
    }
}

// The register kernels of K9, K12 and K14 walk batches of 256 / LPR lane groups x U rows: row u of batch b for lane group g.  The
// loads and the stores of a batch in K9 and K12 form it with this one expression (K14 writes it out: DESIGN.md K14).
template <int LPR, int U>
__device__ __forceinline__ int64_t batch_row(const int64_t b, const int u, const int g) {
    constexpr int GPB = 256 / LPR;
    return (b * U + u) * GPB + g;
}

// ---- row-wise reductions: LPR lanes cooperate on one row, 64/LPR rows per wavefront ------------------------
// All-lanes sum over groups of LPR consecutive lanes.  Inside a 16-lane row the exchange is done by the VALU's DPP
// modifiers (quad permutes, half-row / row mirrors) -- no LDS-crossbar instruction; only the steps that cross rows
// (LPR = 32, 64) use gfx950's v_permlane16_swap / v_permlane32_swap (VALU as well).  (With all steps on ds_bpermute the fused NAFS kernel, 2H reductions per row, ran at
// 0.48-0.52 of the streaming rate.)
template <int CTRL>
__device__ __forceinline__ float dpp_xchg(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}

template <int LPR>
__device__ __forceinline__ float group_sum(float v) {
    static_assert(LPR == 8 || LPR == 16 || LPR == 32 || LPR == 64, "groups of 8 / 16 / 32 / 64 lanes");
    v += dpp_xchg<0xB1>(v);                        // quad_perm [1,0,3,2]: lane ^ 1
    v += dpp_xchg<0x4E>(v);                        // quad_perm [2,3,0,1]: lane ^ 2
    v += dpp_xchg<0x141>(v);                       // row_half_mirror: lane i <-> 7 - i (the other quad of the 8)
    if constexpr (LPR >= 16) v += dpp_xchg<0x140>(v);   // row_mirror: lane i <-> 15 - i (the other half of the row)
    if constexpr (LPR >= 32) {   // gfx950 v_permlane16_swap: odd rows of the first operand <-> even rows of the second;
        const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
        v = __uint_as_float(r[0]) + __uint_as_float(r[1]);      // with both operands = v the two results are v[lane] and v[lane ^ 16]
    }
    if constexpr (LPR >= 64) {   // v_permlane32_swap: upper half of the first operand <-> lower half of the second
        const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
        v = __uint_as_float(r[0]) + __uint_as_float(r[1]);
    }
    return v;
}

// Register budget of the register-resident row kernels: few hop vectors per lane -> insist on 8 workgroups per CU (<= 64 VGPRs);
// left at 4 the scheduler spends the 128 registers it is allowed on speculation (HMAX = 6: 128 VGPRs, 4 waves per SIMD) instead of
// the ~46 the kernel needs: NAFS at d = 128, H = 6 0.715 -> 0.739 of peak.  At MANY hops these kernels were VALU-issue-bound (see
// "one hop per lane" below), which is why two restructurings that bought wavefronts with extra instructions lost (round 3): an
// online softmax without a score array (0.58 vs 0.67) and one row per wavefront with the hops split over the half-waves
// (v_permlane32_swap exchanges; 8 waves, but 0.57 / 0.48 vs 0.67 / 0.62) -- profiles/r03_aggregators_{online_gate,hop_split}_experiment.log.
#define ROWREG_MIN_BLOCKS(HMAX, CH) (((HMAX) * (CH) <= 8) ? 8 : (((HMAX) * (CH) <= 16) ? 4 : 2))

// ---- per-row scalars, one hop per lane -------------------------------------------------------------------------------------
// After the row reductions every lane of a row's group holds all H per-hop scalars.  Evaluating sigmoid / softmax / the IEEE
// divisions hop after hop costs H instruction sequences per WAVEFRONT (every lane repeats them): ~1 050 VALU instructions at
// H = 11, i.e. 85 % of the VALU issue slots at the streaming rate (profiles/r03_agg_pmc.md) -- the row kernels were issue-bound.
// With H <= LPR lane l of the group takes hop l (it keeps hop l's reduced scalars as they are produced): ONE sequence per
// wavefront, then the weights are broadcast back -- and no per-hop score array stays in registers (NAFS at 12 hop vectors:
// 82 -> 62 VGPRs, 5 -> 8 wavefronts per SIMD).  The
// arithmetic (operations, their order, IEEE division, the hop-ordered sum) is unchanged: results are bit-identical.
template <int LPR>
__device__ __forceinline__ float from_lane(const float v, const int h) {   // value of lane h of this lane's group
    if constexpr (LPR == 64) {
        return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), h));
    } else {
        const int lane = (int)(threadIdx.x & 63);
        return __int_as_float(__builtin_amdgcn_ds_bpermute(((lane & ~(LPR - 1)) + h) << 2, __float_as_int(v)));
    }
}
template <int LPR>
__device__ __forceinline__ float group_max(float v) {
    v = fmaxf(v, dpp_xchg<0xB1>(v));
    v = fmaxf(v, dpp_xchg<0x4E>(v));
    v = fmaxf(v, dpp_xchg<0x141>(v));
    if constexpr (LPR >= 16) v = fmaxf(v, dpp_xchg<0x140>(v));
    if constexpr (LPR >= 32) {
        const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
        v = fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
    }
    if constexpr (LPR >= 64) {
        const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
        v = fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
    }
    return v;
}

// Output row of a register-resident row kernel.  dw = the columns the kernel writes: exactly d, or -- when the caller declared the
// tail of the row's pitch to be padding (sgl::out_cols) -- d + pad, the pad columns as zeros.  Why: a row of d = 147 floats on a
// 160-float pitch ends 52 bytes short of its last 128-byte line, and a line that is only partly written costs a read-modify-write in
// the ECC-protected HBM: the output write of the gate / NAFS kernels ran at 2.7 TB/s at d = 147 against 5.8 TB/s at d = 160
// (profiles/r04_aggregators.log; the element-wise kernels always streamed whole pitches).
template <int LPR, int CH>
__device__ __forceinline__ void store_row(float *__restrict__ orow, const f4 (&acc)[CH], const int l, const bool live, const int d,
                                          const int dw) {
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const int col = (c * LPR + l) * 4;
        if (live && col < dw) {
            f4 v = acc[c];
            if (col + 4 <= dw) {                    // whole vector; what lies beyond d is padding the kernel owns: zeros
                if (col + 4 > d) {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (col + e >= d) v[e] = 0.f;
                }
                // non-temporal: with plain (write-back) stores these kernels are 7-20 % slower at every width -- also at widths whose
                // rows share lines with their neighbours (d = 100: 0.906 -> 0.935 ms, d = 147: 1.98 -> 2.42 ms, d = 128: 1.51 -> 1.65 ms;
                // profiles/r04_aggregators_plain_stores_experiment.log)
                __builtin_nontemporal_store(v, reinterpret_cast<f4 *>(orow + col));
            } else {                                // dw == d, the vector straddles it: never write past the caller's d columns
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (col + e < dw) orow[col + e] = v[e];
            }
        }
    }
}

// ---- the steps of a row kernel: LPR lanes per row, 256 / LPR rows per workgroup, CH 16-byte chunks per lane -------------------------
// Each step is written once, here.  The register-resident kernels sit at register boundaries that the source layout disturbs, and a
// forced-inline helper is optimised on its own before it is inlined, so the shape of each one was chosen against the per-kernel
// register table of the hand-written loops: the mask and the accumulate work on ONE chunk by value (filling
// `bool (&on)[CH]` in a helper moved 48 instances, `acc[CH]` by reference in mul_add 19), the hop table is passed by value.
struct RowLane {
    int l;         // this lane's place in the row's group of LPR lanes
    int64_t r;     // the group's row; row 0 where the group lies beyond the matrix, so that every address formed from it is valid
    bool live;     // the group has a row
};
template <int LPR>
__device__ __forceinline__ RowLane row_lane(const int64_t n) {
    constexpr int RPB = 256 / LPR;  // rows per block
    const int l = threadIdx.x % LPR;
    const int64_t row = (int64_t)blockIdx.x * RPB + threadIdx.x / LPR;
    const bool live = row < n;
    return {l, live ? row : 0, live};
}

// chunk c of this lane (the four columns from (c * LPR + l) * 4) belongs to a row and starts inside its d columns
template <int LPR>
__device__ __forceinline__ bool chunk_on(const int c, const int l, const bool live, const int d) {
    return live && ((c * LPR + l) * 4 < d);
}

// x[h][c] = chunk c of row r of hop h for the first n_hops hops of the table, zeros elsewhere.  LOAD(row, col, d): the masked 16-byte
// access of the table's element type (load_masked<4, NT>; sgl_aggregate_bf16.hip has the widening one).  The row address is formed
// under `h < n_hops` only: formed for every h < HMAX it cost 21 instances occupancy and put 3 into scratch.  hop_rowdot_reg_kernel
// and hop_rowdot2_reg_kernel keep their own chunk-outer loop: this hop-outer one raised their registers in every instance.
template <auto LOAD, int LPR, int CH, int HMAX, typename Table>
__device__ __forceinline__ void load_hop_rows(f4 (&x)[HMAX][CH], const Table hx, const int n_hops, const int64_t r, const bool (&on)[CH],
                                              const int l, const int d) {
#pragma unroll
    for (int h = 0; h < HMAX; ++h) {
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            x[h][c] = (f4){0.f, 0.f, 0.f, 0.f};
            if (h < n_hops && on[c]) x[h][c] = LOAD(hx.p[h] + r * hx.ld[h], (c * LPR + l) * 4, d);
        }
    }
}

// this lane's part of <a, b> on top of s: one FMA chain in chunk and element order (the group_sum over the row's lanes follows)
__device__ __forceinline__ float dot4(const f4 a, const f4 b, float s) {
#pragma unroll
    for (int e = 0; e < 4; ++e) s = __builtin_fmaf(a[e], b[e], s);
    return s;
}
template <int CH>
__device__ __forceinline__ float dot_chunks(const f4 (&a)[CH], const f4 (&b)[CH]) {
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < CH; ++c) s = dot4(a[c], b[c], s);
    return s;
}
// dot = <a, b> and sq = <b, b>, the two chains interleaved element by element
template <int CH>
__device__ __forceinline__ void dot_sq_chunks(const f4 (&a)[CH], const f4 (&b)[CH], float &dot, float &sq) {
    dot = 0.f;
    sq = 0.f;
#pragma unroll
    for (int c = 0; c < CH; ++c)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            dot = __builtin_fmaf(a[c][e], b[c][e], dot);
            sq = __builtin_fmaf(b[c][e], b[c][e], sq);
        }
}
// s0 = <a0, b> and s1 = <a1, b>: two vectors against one row, interleaved
template <int CH>
__device__ __forceinline__ void dot2_chunks(const f4 (&a0)[CH], const f4 (&a1)[CH], const f4 (&b)[CH], float &s0, float &s1) {
    s0 = 0.f;
    s1 = 0.f;
#pragma unroll
    for (int c = 0; c < CH; ++c)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            s0 = __builtin_fmaf(a0[c][e], b[c][e], s0);
            s1 = __builtin_fmaf(a1[c][e], b[c][e], s1);
        }
}

// acc + w x on one chunk, in the two forms the operators define -- they round differently and are not interchangeable:
// one FMA per element (the learnable gates: the chain of hop_wsum2d_kernel) ...
__device__ __forceinline__ f4 fma4(f4 acc, const float w, const f4 x) {
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] = __builtin_fmaf(w, x[e], acc[e]);
    return acc;
}
// ... or a rounded product, then the add (NAFS, by contract: over_smooth_distance_op.py:27-31 multiplies, then sums)
__device__ __forceinline__ f4 mul_add4(f4 acc, const float w, const f4 x) {
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] = __fadd_rn(acc[e], __fmul_rn(w, x[e]));
    return acc;
}

// ---- host side: run-time values as compile-time arguments of a generic lambda ----------------------------------------------------
// Each helper calls f with std::integral_constant arguments (usable as template arguments inside the lambda) and returns whether it
// called it: a value with no compiled instance launches nothing and the entry point reports it.
template <int V>
using Int = std::integral_constant<int, V>;

template <int... Vs, typename F>
bool with_one_of(int v, F &&f) {   // f(Int<V>) for the V of the list that equals v
    return ((v == Vs ? (f(Int<Vs>{}), true) : false) || ...);
}
template <typename F>
bool with_lpr(int lpr, F &&f) {   // lanes per row
    return with_one_of<8, 16, 32, 64>(lpr, f);
}
template <typename F>
bool with_lpr_vec(int lpr, bool vec4, F &&f) {   // f(lanes per row, floats per lane access)
    return vec4 ? with_lpr(lpr, [&](auto L) { f(L, Int<4>{}); }) : with_lpr(lpr, [&](auto L) { f(L, Int<1>{}); });
}
template <typename F>
bool with_bool(bool b, F &&f) {
    b ? f(std::true_type{}) : f(std::false_type{});
    return true;
}
template <typename F>
bool with_vec(bool vec4, F &&f) {   // floats per lane access
    vec4 ? f(Int<4>{}) : f(Int<1>{});
    return true;
}
template <typename F>
bool with_hop_capacity(int n, F &&f) {   // kernels that keep per-hop values of up to 4 / 8 / 12 / 16 hops in registers
    return with_one_of<4, 8, 12, 16>(n <= 4 ? 4 : (n + 3) / 4 * 4, f);
}

// f(LPR, VEC, CH) for an instance of sgl::slice_instance: one vector per lane with any lane count, then 64 lanes with a count of the
// family's list for the lane size (sgl_common.h: the list the rule read); MORE: counts the family compiles besides (K11's 0)
template <int... MORE, int... Cs, typename F>
bool with_chunks(sgl::Chunks<Cs...>, int ch, F &&f) {
    return with_one_of<MORE..., Cs...>(ch, f);
}
template <typename Family, int... MORE, typename F>
bool with_slice_instance(const sgl::SliceInstance &in, bool vec4, F &&f) {
    if (in.ch == 1) return with_lpr_vec(in.lpr, vec4, [&](auto L, auto V) { f(L, V, Int<1>{}); });
    if (vec4) return with_chunks<MORE...>(typename Family::Vec4{}, in.ch, [&](auto C) { f(Int<64>{}, Int<4>{}, C); });
    return with_chunks<MORE...>(typename Family::Vec1{}, in.ch, [&](auto C) { f(Int<64>{}, Int<1>{}, C); });
}

// f(LPR, CH) for a layout of sgl::row_layout.  HAS_8X5: the kernel family has 8 x 5 instances (hop_rowdot2_reg_kernel alone).
template <bool HAS_8X5, typename F>
bool with_row_layout(int lpr, int ch, F &&f) {
    if (ch == 5) {
        if constexpr (HAS_8X5) return with_one_of<8>(lpr, [&](auto L) { f(L, Int<5>{}); });
        return false;
    }
    if (ch == 3) return with_one_of<16>(lpr, [&](auto L) { f(L, Int<3>{}); });
    if (ch == 2) return with_one_of<32, 64>(lpr, [&](auto L) { f(L, Int<2>{}); });
    return ch == 1 && with_lpr(lpr, [&](auto L) { f(L, Int<1>{}); });
}
// f(LPR, CH, HMAX) for an instance of sgl::row_instance: every even capacity up to 16, 12 (16 x 3) or 6 (8 x 5) hop vectors
template <bool HAS_8X5, typename F>
bool with_row_instance(const sgl::RowInstance &in, F &&f) {
    bool called = false;
    with_row_layout<HAS_8X5>(in.lpr, in.ch, [&](auto L, auto C) {
        if constexpr (C == 5) called = with_one_of<2, 4, 6>(in.hmax, [&](auto HM) { f(L, C, HM); });
        else if constexpr (C == 3) called = with_one_of<2, 4, 6, 8, 10, 12>(in.hmax, [&](auto HM) { f(L, C, HM); });
        else called = with_one_of<2, 4, 6, 8, 10, 12, 14, 16>(in.hmax, [&](auto HM) { f(L, C, HM); });
    });
    return called;
}
// what an entry point answers when one of the two did not call its lambda
inline int no_row_instance(const char *who, int lpr, int ch, int n_hops) {
    return sgl::fail(SGL_ERR_UNSUPPORTED, "%s: no kernel instance is compiled for the %d x %d lane layout with %d hops", who, lpr, ch, n_hops);
}

// The hop table of a kernel (Hops, HopsB: p[], ld[]) from the caller's arrays.  who: prefix of the error texts (NULL: none);
// align: bytes of one element; *vec4 (optional) is cleared where the rows of a float hop are not 16-byte vectors.
template <typename Table, typename T>
int fill_hops(const char *who, Table &hx, int n_hops, const T *const *h_x, const int64_t *h_ldx, int64_t d, int align, bool *vec4) {
    const char *sep = who ? ": " : "";
    if (!who) who = "";
    if (n_hops < 1 || n_hops > SGL_MAX_HOPS) return sgl::fail(SGL_ERR_INVALID, "%s%sn_hops=%d outside [1,%d]", who, sep, n_hops, SGL_MAX_HOPS);
    if (!h_x) return sgl::fail(SGL_ERR_INVALID, "%s%sNULL hop pointer array", who, sep);
    for (int h = 0; h < n_hops; ++h) {
        hx.p[h] = h_x[h];
        hx.ld[h] = h_ldx ? h_ldx[h] : d;
        if (!hx.p[h]) return sgl::fail(SGL_ERR_INVALID, "%s%shop %d: NULL pointer", who, sep, h);
        if (hx.ld[h] < d) return sgl::fail(SGL_ERR_INVALID, "%s%shop %d: leading dimension %lld < d", who, sep, h, (long long)hx.ld[h]);
        if (!aligned_to(hx.p[h], (size_t)align)) return sgl::fail(SGL_ERR_INVALID, "%s%shop %d: pointer not %d-byte aligned", who, sep, h, align);
        if (vec4 && (hx.ld[h] % 4 != 0 || !aligned_to(hx.p[h], 16))) *vec4 = false;
    }
    for (int h = n_hops; h < SGL_MAX_HOPS; ++h) {
        hx.p[h] = nullptr;
        hx.ld[h] = 0;
    }
    return SGL_OK;
}

inline int stream_grid(int64_t total_threads) {
    // memory-bound elementwise: one 16-byte element per thread.  Measured on MI355X (products shape, 5 streams): a
    // 2048-block grid-stride launch reaches 5.3 TB/s, one element per thread 5.9 TB/s (torch's add: 6.0); the
    // grid-stride loop only remains as the overflow path for > 2^22 blocks.
    int64_t blocks = (total_threads + 255) / 256;
    const int64_t cap = sgl::tuning("agg_blocks", 0) > 0 ? sgl::tuning("agg_blocks", 0) : ((int64_t)1 << 22);
    if (blocks > cap) blocks = cap;
    if (blocks < 1) blocks = 1;
    return (int)blocks;
}

inline int launch_check(const char *who) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return sgl::fail((int)e, "%s: kernel launch failed: %s", who, hipGetErrorString(e));
    return SGL_OK;
}
#define SGL_LAUNCH_CHECK(who)               \
    do {                                    \
        const int _rc = launch_check(who);  \
        if (_rc != SGL_OK) return _rc;      \
    } while (0)

// The launch of a register-resident row kernel over n rows, from the instance (or layout) that sgl_core.cpp picked to the checked
// launch: grid of 256 / lpr rows per workgroup, launch_fits, typed dispatch, no_row_instance, launch check.  launch(grid, LPR, CH[,
// HMAX]) starts the kernel.  The texts are the entry point's own: `rows` names it in "too many rows", `who` in "no kernel instance",
// `check` in "kernel launch failed".
struct RowLaunchNames {
    const char *rows, *who, *check;
};
template <typename Dispatch>
int launch_rows_with(const RowLaunchNames &names, int lpr, int ch, int n_hops, int64_t n, Dispatch &&dispatch) {
    const int64_t blocks = (n + (256 / lpr) - 1) / (256 / lpr);
    if (!sgl::launch_fits(blocks, 256)) return sgl::fail(SGL_ERR_UNSUPPORTED, "%s: too many rows for one launch (shard the matrix)", names.rows);
    if (!dispatch(dim3((unsigned)blocks))) return no_row_instance(names.who, lpr, ch, n_hops);
    return launch_check(names.check);
}
template <bool HAS_8X5 = false, typename F>
int launch_row_instance(const RowLaunchNames &names, const sgl::RowInstance &in, int n_hops, int64_t n, F &&launch) {
    return launch_rows_with(names, in.lpr, in.ch, n_hops, n, [&](dim3 grid) {
        return with_row_instance<HAS_8X5>(in, [&](auto L, auto C, auto HM) { launch(grid, L, C, HM); });
    });
}
template <typename F>
int launch_row_layout(const RowLaunchNames &names, const sgl::RowLayout &lay, int n_hops, int64_t n, F &&launch) {
    return launch_rows_with(names, lay.lpr, lay.ch, n_hops, n, [&](dim3 grid) {
        return with_row_layout<false>(lay.lpr, lay.ch, [&](auto L, auto C) { launch(grid, L, C); });
    });
}

}  // namespace
