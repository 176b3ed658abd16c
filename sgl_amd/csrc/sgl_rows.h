// Lanes, layouts and launch tables of the register-resident row kernels, shared by sgl_aggregate.hip (float32 hops) and
// sgl_aggregate_bf16.hip (bfloat16 hops): both files must pick the same lane layout and sum in the same lane order for their
// results to be bit-identical, so the rule and the in-wavefront reductions exist once, here.  Not part of the ABI.
#pragma once
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

// ---- lanes x chunks of a register-resident row kernel ------------------------------------------------------------------------
// A row of d floats is ceil(d / 4) 16-byte slots; LPR lanes take CH slots each (slot (c * LPR + l) of the row for lane l, chunk c),
// 64 / LPR rows per wavefront.  Power-of-two groups leave slots idle when the row is not a power of two wide, and idle slots still
// cost their share of every load and VALU instruction: d = 147 (BASELINE config 3: 100 features + 47 label columns = 37 slots) on
// 32 lanes x 2 chunks idles 27 of 64.  Narrow groups with more chunks per lane fit such rows far better -- 8 lanes x 5 chunks
// (40 slots, 8 rows per wavefront, every load instruction of a lane group is one whole 128-byte line) or 16 x 3 (48 slots) -- at
// the price of CH x HMAX hop vectors in registers, so they are instantiated for few hops only (<= 6 / <= 12) and chosen when they
// at least halve the idle slots.  Measured at d = 147 (profiles/r04_aggregators_layouts.log): 16 x 3 is as fast as 32 x 2 at 6 hops
// and 12-15 % faster at 11 (row-dot 0.597 -> 0.661 of peak, gate 0.539 -> 0.613, NAFS 0.536 -> 0.612); 8 x 5 (151 VGPRs, 3 waves
// per SIMD) pays only in the jk-score kernel (0.585 -> 0.657 at 6 hops) and is instantiated for that kernel alone.  At 6 hops the
// gate / NAFS kernels are NOT issue-bound -- halving their VALU instructions and quartering their wavefronts changed nothing
// (profiles/r04_agg_pmc.md) -- what they lost against the plain sum was the partly written last line of the output row
// (store_row below).
struct RowLayout {
    int lpr, ch;
};

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
// tail of the row's pitch to be padding (out_cols() below) -- d + pad, the pad columns as zeros.  Why: a row of d = 147 floats on a
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

int pick_lpr(int64_t d, int vec) {
    const int64_t lanes = (d + vec - 1) / vec;
    int lpr = 8;
    while (lpr < lanes && lpr < 64) lpr <<= 1;
    return lpr;
}

// Columns a row-producing kernel writes: the d data columns plus the `pad` columns after them that the CALLER declared to be the
// row's own padding (the *_padded_f32 entry points; sgl_amd.device passes the tail of the pitch of the outputs it allocates) --
// written as zeros, so that every line of the row is written whole.  The kernels never guess: with pad = 0 nothing beyond column
// d is touched.  `room` = the columns the lane layout reaches.
int out_cols(int64_t d, int64_t pad, int64_t room) {
    int64_t dw = sgl::tuning("row_whole_lines", 1) != 0 ? d + pad : d;
    if (dw > room) dw = room > d ? room / 4 * 4 : d;
    if (dw > d && dw % 4 != 0) dw = d;              // (validated by the entry points: d + pad is a whole number of vectors)
    return (int)dw;
}

int check_pad(const char *who, int64_t width, int64_t pad, int64_t ldo) {
    if (pad < 0 || width + pad > ldo) return sgl::fail(SGL_ERR_INVALID, "%s: pad_cols=%lld does not fit the output pitch", who, (long long)pad);
    if (pad > 0 && ((width + pad) % 4 != 0 || ldo % 4 != 0))
        return sgl::fail(SGL_ERR_INVALID, "%s: padded rows must be whole 16-byte vectors (width + pad_cols and ldo multiples of 4)", who);
    return SGL_OK;
}

RowLayout pick_row_layout(int64_t d, int n_hops, bool allow_8x5 = false) {
    RowLayout r;
    r.lpr = pick_lpr(d, 4);
    r.ch = (d > r.lpr * 4) ? 2 : 1;
    if (r.lpr == 64 && r.ch == 1 && d > 128 && sgl::tuning("row_lpr32x2", 1) != 0) {   // 2 rows per wavefront
        r.lpr = 32;
        r.ch = 2;
    }
    if (sgl::tuning("row_narrow_groups", 1) != 0 && d <= r.lpr * 4 * r.ch) {
        const int slots = (int)((d + 3) / 4);
        static const int cand[2][3] = {{16, 3, 12}, {8, 5, 6}};       // lanes, chunks, most hops instantiated
        const int64_t mode = sgl::tuning("row_narrow_groups", 1);       // 1: both candidates, 2: 16 x 3 only, 3: 8 x 5 only (measurements)
        for (const auto &c : cand) {
            const int idle = c[0] * c[1] - slots;
            if (((mode == 2 || !allow_8x5) && c[0] == 8) || (mode == 3 && c[0] == 16)) continue;
            if (idle >= 0 && n_hops <= c[2] && 2 * idle <= r.lpr * r.ch - slots) {
                r.lpr = c[0];
                r.ch = c[1];
            }
        }
    }
    return r;
}

// KH(L, C): all even hop counts up to 16; KH12 / KH6: the narrow-group layouts, instantiated up to 12 / 6 hop vectors
#define SGL_ROWREG_DISPATCH(KH, KH12, KH6, lay)                        \
    do {                                                               \
        if ((lay).lpr == 8 && (lay).ch == 5) KH6(8, 5);                \
        else if ((lay).lpr == 16 && (lay).ch == 3) KH12(16, 3);        \
        else if ((lay).lpr == 32 && (lay).ch == 2) KH(32, 2);          \
        else if ((lay).ch == 2) KH(64, 2);                             \
        else if ((lay).lpr == 8) KH(8, 1);                             \
        else if ((lay).lpr == 16) KH(16, 1);                           \
        else if ((lay).lpr == 32) KH(32, 1);                           \
        else KH(64, 1);                                                \
    } while (0)
#define SGL_HOPS_UP_TO_16(K, L, C)                 \
    do {                                           \
        if (n_hops <= 2) K(L, C, 2);               \
        else if (n_hops <= 4) K(L, C, 4);          \
        else if (n_hops <= 6) K(L, C, 6);          \
        else if (n_hops <= 8) K(L, C, 8);          \
        else if (n_hops <= 10) K(L, C, 10);        \
        else if (n_hops <= 12) K(L, C, 12);        \
        else if (n_hops <= 14) K(L, C, 14);        \
        else K(L, C, 16);                          \
    } while (0)
#define SGL_HOPS_UP_TO_12(K, L, C)                 \
    do {                                           \
        if (n_hops <= 2) K(L, C, 2);               \
        else if (n_hops <= 4) K(L, C, 4);          \
        else if (n_hops <= 6) K(L, C, 6);          \
        else if (n_hops <= 8) K(L, C, 8);          \
        else if (n_hops <= 10) K(L, C, 10);        \
        else K(L, C, 12);                          \
    } while (0)
#define SGL_HOPS_UP_TO_6(K, L, C)                  \
    do {                                           \
        if (n_hops <= 2) K(L, C, 2);               \
        else if (n_hops <= 4) K(L, C, 4);          \
        else K(L, C, 6);                           \
    } while (0)

#define SGL_LAUNCH_CHECK(what)                                                                                  \
    do {                                                                                                        \
        hipError_t _e = hipGetLastError();                                                                      \
        if (_e != hipSuccess) return sgl::fail((int)_e, what ": kernel launch failed: %s", hipGetErrorString(_e)); \
    } while (0)

}  // namespace
