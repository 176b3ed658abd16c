// CSR (fp32 values) x dense bfloat16 SpMM for gfx950 (MI355X): the opt-in reduced-precision STORAGE of hop matrices
// (GraphOp(hop_dtype="bfloat16")), and the row gathers that widen stored bf16 hops back to fp32.
//
// The fp32 kernel (sgl_spmm.hip) is bound by the 128-byte lines its gathers pull through the fabric; a bf16 row is
// half as many bytes, so a gathered neighbour costs half the lines.  Everything else is the fp32 kernel's design, on the same
// handle and plan: one wavefront per work item, R non-zero slots x GROUP feature lanes, the (col, val) stream broadcast from
// registers, U gathers in flight per lane, split rows combined by a deterministic fix-up pass, XCD-aware block order, row maps.
//
// Numerics: a gathered element is widened exactly (bits << 16), accumulated with fmaf in fp32 in the fp32 kernel's term order
// (strict order: one sequential chain per row; otherwise a non-zero's slot is its index within the row mod R), split-row partial
// sums stay fp32, and the finished sum is rounded ONCE to bf16, round-to-nearest-even (v_cvt_pk_bf16_f32: NaN stays NaN, +-inf
// stays +-inf, overflow rounds to inf, subnormals are kept).  The running aggregate of sgl_spmm_acc_bf16 is fp32 and takes the
// rounded value widened again, i.e. exactly what a later pass over the stored hop would read.
#include "sgl_spmm_common.h"

namespace {

typedef float f2 __attribute__((ext_vector_type(2)));
typedef float f4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf2 __attribute__((ext_vector_type(2)));
typedef uint32_t u2 __attribute__((ext_vector_type(2)));
typedef uint32_t u4 __attribute__((ext_vector_type(4)));

// two floats -> two bf16 in one 32-bit word (element 0 in the low half), round-to-nearest-even
__device__ __forceinline__ uint32_t pack2(float a, float b) {
    const f2 v = {a, b};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf2));
}
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

template <int BV>
__device__ __forceinline__ typename RawT<BV>::type rzero() {
    if constexpr (BV == 8)
        return (u4){0u, 0u, 0u, 0u};
    else if constexpr (BV == 4)
        return (u2){0u, 0u};
    else
        return 0;
}

template <int BV>
__device__ __forceinline__ void widen(const typename RawT<BV>::type &r, float (&f)[BV]) {
    if constexpr (BV == 1) {
        f[0] = __uint_as_float((uint32_t)r << 16);
    } else if constexpr (BV == 2) {
        f[0] = widen_lo(r);
        f[1] = widen_hi(r);
    } else {
#pragma unroll
        for (int w = 0; w < BV / 2; ++w) {
            f[2 * w] = widen_lo(r[w]);
            f[2 * w + 1] = widen_hi(r[w]);
        }
    }
}

template <int BV>
__device__ __forceinline__ typename RawT<BV>::type narrow(const float (&f)[BV]) {
    if constexpr (BV == 1) {
        return (uint16_t)(pack2(f[0], 0.f) & 0xffffu);
    } else if constexpr (BV == 2) {
        return pack2(f[0], f[1]);
    } else {
        typename RawT<BV>::type r;
#pragma unroll
        for (int w = 0; w < BV / 2; ++w) r[w] = pack2(f[2 * w], f[2 * w + 1]);
        return r;
    }
}

// BV consecutive floats (split-row partial sums, the running aggregate): 16-byte accesses from BV = 4 up
template <int BV>
__device__ __forceinline__ void load_f(const float *p, float (&f)[BV]) {
    if constexpr (BV >= 4) {
#pragma unroll
        for (int q = 0; q < BV / 4; ++q) {
            const f4 t = *reinterpret_cast<const f4 *>(p + 4 * q);
#pragma unroll
            for (int e = 0; e < 4; ++e) f[4 * q + e] = t[e];
        }
    } else if constexpr (BV == 2) {
        const f2 t = *reinterpret_cast<const f2 *>(p);
        f[0] = t[0];
        f[1] = t[1];
    } else {
        f[0] = *p;
    }
}

template <int BV>
__device__ __forceinline__ void store_f(float *p, const float (&f)[BV]) {
    if constexpr (BV >= 4) {
#pragma unroll
        for (int q = 0; q < BV / 4; ++q) {
            const f4 t = {f[4 * q], f[4 * q + 1], f[4 * q + 2], f[4 * q + 3]};
            *reinterpret_cast<f4 *>(p + 4 * q) = t;
        }
    } else if constexpr (BV == 2) {
        const f2 t = {f[0], f[1]};
        *reinterpret_cast<f2 *>(p) = t;
    } else {
        *p = f[0];
    }
}

template <int BV>
__device__ __forceinline__ void vfma(float (&acc)[BV], float v, const typename RawT<BV>::type &x) {
    float xf[BV];
    widen<BV>(x, xf);
#pragma unroll
    for (int e = 0; e < BV; ++e) acc[e] = __builtin_fmaf(v, xf[e], acc[e]);
}

// running fp32 aggregate over hops: the modes and arithmetic of sgl_spmm_acc_f32 (acc_apply, sgl_spmm_common.h)
struct AccEpi {
    float *acc = nullptr;   // nullptr = off
    int64_t ldacc = 0;
    float acc_w = 1.f, acc_div = 1.f;
    int acc_mode = 0;
};

__device__ __forceinline__ float acc_apply(float a, float y, const AccEpi &e) { return acc_apply(a, y, e.acc_mode, e.acc_w, e.acc_div); }

struct Bf16Args {
    const int32_t *items;       // (row_begin,row_end) pairs
    const sgl::Piece *pieces;   // long-row pieces
    const int64_t *rowptr;
    const int32_t *col;
    const float *val;
    const uint16_t *x;
    uint16_t *y;
    float *partial;
    int64_t ldx, ldy, ldp;
    int32_t n_items, n_pieces, d;
    BlockMap map;
    AccEpi epi;                 // epi.acc: matrix base
    const int32_t *rowmap;      // optional [n_rows]: storage row -> output row (sgl_csr_set_rowmap); NULL = identity
};

// One wavefront walks `nrows` consecutive rows whose non-zeros are colb/valb[0 .. tot); lane i of `my_rel` holds the offset of row
// i's first non-zero (lane nrows holds tot).  PARTIAL: the row is a piece of a split row, its fp32 sum goes to `pout` unrounded.
// Otherwise the sum is rounded to bf16 into `yout` and the rounded value, widened, enters the running aggregate.
template <int BV, int GROUP, int NCH, int U, bool PARTIAL>
__device__ __forceinline__ void run_rows(const int32_t *__restrict__ colb, const float *__restrict__ valb, const int my_rel,
                                         const int nrows, const int tot, const uint16_t *__restrict__ x, const int64_t ldx,
                                         uint16_t *__restrict__ yout, float *__restrict__ pout, const int64_t ldo, const int d,
                                         const int lane, const AccEpi epi, const RowMap rm = RowMap()) {
    using Raw = typename RawT<BV>::type;
    constexpr int R = 64 / GROUP;
    const int s = (R == 1) ? 0 : (lane / GROUP);
    const int l = lane % GROUP;
    int colofs[NCH];
    bool on[NCH];
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
        colofs[ch] = (ch * GROUP + l) * BV;
        on[ch] = colofs[ch] < d;      // d is a multiple of BV: a lane's vector is whole or absent
    }
    // current / next 64-element slice of the (col,val) stream, one element per lane
    int cbr = 0;
    int my_c = 0, nx_c = 0;
    float my_v = 0.f, nx_v = 0.f;
    if (lane < tot) {
        my_c = colb[lane];
        my_v = valb[lane];
    }
    if (64 + lane < tot) {
        nx_c = colb[64 + lane];
        nx_v = valb[64 + lane];
    }

    for (int ri = 0; ri < nrows; ++ri) {
        const int jb = __builtin_amdgcn_readlane(my_rel, ri);
        const int je = __builtin_amdgcn_readlane(my_rel, ri + 1);
        const int64_t ro = rm.on ? (int64_t)__builtin_amdgcn_readlane(rm.my_map, ri) : (int64_t)ri;   // output row
        float acc[NCH][BV];
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
            for (int e = 0; e < BV; ++e) acc[ch][e] = 0.f;
        int j = jb;
        while (j < je) {
            const int lim = min(je, cbr + 64);
            const int o = j - cbr;
            const int cnt = lim - j;
            // slot of a non-zero = its index WITHIN ITS ROW mod R (the rule of the fp32 kernel): every slot adds the same terms in
            // the same order under any plan and any processing order of the rows
            const int sh = (R == 1) ? 0 : ((s - (j - jb)) & (R - 1));
            int t = 0;
            for (; t + R * U <= cnt; t += R * U) {
                int c[U];
                float v[U];
                Raw xv[U][NCH];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int idx = o + t + u * R + sh;
                    c[u] = bcast_i<R>(my_c, idx);
                    v[u] = bcast_f<R>(my_v, idx);
                }
#pragma unroll
                for (int ch = 0; ch < NCH; ++ch) {
                    if (on[ch]) {
#pragma unroll
                        for (int u = 0; u < U; ++u)
                            xv[u][ch] = *reinterpret_cast<const Raw *>(x + (int64_t)c[u] * ldx + colofs[ch]);
                    } else {
#pragma unroll
                        for (int u = 0; u < U; ++u) xv[u][ch] = rzero<BV>();
                    }
                }
#pragma unroll
                for (int u = 0; u < U; ++u)
#pragma unroll
                    for (int ch = 0; ch < NCH; ++ch) vfma<BV>(acc[ch], v[u], xv[u][ch]);
            }
            if (t < cnt) {
                // the remainder (< R * U non-zeros) as ONE predicated batch: its gathers are issued together like a full batch's,
                // not one dependent load after the other; a slot still adds its terms in index order
                int c[U];
                float v[U];
                bool valid[U];
                Raw xv[U][NCH];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    valid[u] = (t + u * R + sh) < cnt;
                    const int idx = (o + t + u * R + sh) & 63;
                    c[u] = bcast_i<R>(my_c, idx);
                    v[u] = bcast_f<R>(my_v, idx);
                }
#pragma unroll
                for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        xv[u][ch] = rzero<BV>();
                        if (valid[u] && on[ch]) xv[u][ch] = *reinterpret_cast<const Raw *>(x + (int64_t)c[u] * ldx + colofs[ch]);
                    }
#pragma unroll
                for (int u = 0; u < U; ++u)
                    if (valid[u]) {
#pragma unroll
                        for (int ch = 0; ch < NCH; ++ch) vfma<BV>(acc[ch], v[u], xv[u][ch]);
                    }
            }
            j = lim;
            if (lim == cbr + 64) {  // slice exhausted: rotate, prefetch the one after next
                cbr += 64;
                my_c = nx_c;
                my_v = nx_v;
                if (cbr + 64 + lane < tot) {
                    nx_c = colb[cbr + 64 + lane];
                    nx_v = valb[cbr + 64 + lane];
                }
            }
        }
        if constexpr (R > 1) {
#pragma unroll
            for (int off = GROUP; off < 64; off <<= 1)
#pragma unroll
                for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
                    for (int e = 0; e < BV; ++e) acc[ch][e] += __shfl_xor(acc[ch][e], off, 64);
        }
        if (s == 0) {
#pragma unroll
            for (int ch = 0; ch < NCH; ++ch)
                if (on[ch]) {
                    if constexpr (PARTIAL) {
                        store_f<BV>(pout + ro * ldo + colofs[ch], acc[ch]);
                    } else {
                        const Raw r = narrow<BV>(acc[ch]);
                        if (epi.acc) {
                            float yv[BV], a[BV];
                            widen<BV>(r, yv);       // the STORED value: what a pass over the hop matrix would read
                            float *ap = epi.acc + ro * epi.ldacc + colofs[ch];
                            load_f<BV>(ap, a);
#pragma unroll
                            for (int e = 0; e < BV; ++e) a[e] = acc_apply(a[e], yv[e], epi);
                            store_f<BV>(ap, a);
                        }
                        *reinterpret_cast<Raw *>(yout + ro * ldo + colofs[ch]) = r;
                    }
                }
        }
    }
}

template <int BV, int GROUP, int NCH, int U>
__global__ __launch_bounds__(256) void spmm_bf16_kernel(const Bf16Args a) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.x;
    if (b < a.map.piece_blocks) {
        const int p = b * a.map.waves + wave;
        if (p >= a.n_pieces) return;
        const sgl::Piece pc = a.pieces[p];
        const int my_rel = (lane == 0) ? 0 : pc.len;
        const AccEpi none;     // pieces hold partial sums: rounding and the aggregate happen in the fix-up kernel
        run_rows<BV, GROUP, NCH, U, true>(a.col + pc.begin, a.val + pc.begin, my_rel, 1, pc.len, a.x, a.ldx, nullptr,
                                          a.partial + (int64_t)p * a.ldp, a.ldp, a.d, lane, none);
    } else {
        int ib = b - a.map.piece_blocks;
        if (a.map.xcd_remap) ib = xcd_block(ib, a.map.item_blocks_per_xcd);
        const int item = ib * a.map.waves + wave;
        if (item >= a.n_items) return;
        const int row_begin = a.items[2 * item], row_end = a.items[2 * item + 1];
        const int nrows = row_end - row_begin;
        const ItemWindow w = item_window(a.rowptr, row_begin, nrows, lane);
        const RowMap rm = item_rowmap(a.rowmap, row_begin, nrows, lane);
        const int64_t first = rm.on ? 0 : row_begin;
        AccEpi epi = a.epi;
        if (epi.acc) epi.acc += first * epi.ldacc;
        run_rows<BV, GROUP, NCH, U, false>(a.col + w.base, a.val + w.base, w.my_rel, nrows, w.tot, a.x, a.ldx, a.y + first * a.ldy,
                                           nullptr, a.ldy, a.d, lane, epi, rm);
    }
}

// Y[row, :] = bf16(sum of the row's fp32 piece partials, in storage order): the one rounding of a split row
__global__ __launch_bounds__(256) void spmm_bf16_fixup_kernel(const int32_t *__restrict__ long_row,
                                                              const int32_t *__restrict__ long_first,
                                                              const float *__restrict__ partial, int64_t ldp,
                                                              uint16_t *__restrict__ y, int64_t ldy, int d, AccEpi epi) {
    const int kblocks = (d + 255) / 256;
    const int lr = blockIdx.x / kblocks;
    const int k = (blockIdx.x % kblocks) * 256 + threadIdx.x;
    if (k >= d) return;
    const int row = long_row[lr];
    const int p0 = long_first[lr], p1 = long_first[lr + 1];
    float acc = 0.f;
    for (int p = p0; p < p1; ++p) acc += partial[(int64_t)p * ldp + k];
    const uint16_t r = (uint16_t)(pack2(acc, 0.f) & 0xffffu);
    if (epi.acc) {   // here epi.acc is the matrix base (rows are absolute in the fix-up)
        float *ap = epi.acc + (int64_t)row * epi.ldacc + k;
        *ap = acc_apply(*ap, __uint_as_float((uint32_t)r << 16), epi);
    }
    y[(int64_t)row * ldy + k] = r;
}

template <int BV, int GROUP, int NCH, int U>
hipError_t launch_variant(const Bf16Args &a, int grid, hipStream_t st) {
    hipLaunchKernelGGL((spmm_bf16_kernel<BV, GROUP, NCH, U>), dim3(grid), dim3(64 * a.map.waves), 0, st, a);
    return hipGetLastError();
}

template <int BV, int GROUP, int NCH>
hipError_t launch_u(const Bf16Args &a, int grid, hipStream_t st, int ulevel) {
    using sgl::unroll_of;
    if (ulevel == 2) return launch_variant<BV, GROUP, NCH, unroll_of(GROUP, NCH, 2)>(a, grid, st);
    return ulevel == 0 ? launch_variant<BV, GROUP, NCH, unroll_of(GROUP, NCH, 0)>(a, grid, st)
                       : launch_variant<BV, GROUP, NCH, unroll_of(GROUP, NCH, 1)>(a, grid, st);
}

template <int BV>
hipError_t launch_group(const Bf16Args &a, int grid, hipStream_t st, int ulevel, int group, int nch) {
    if (nch == 1) {
        switch (group) {
            case 8:
                return launch_u<BV, 8, 1>(a, grid, st, ulevel);
            case 16:
                return launch_u<BV, 16, 1>(a, grid, st, ulevel);
            case 32:
                return launch_u<BV, 32, 1>(a, grid, st, ulevel);
            default:
                return launch_u<BV, 64, 1>(a, grid, st, ulevel);
        }
    }
    if (nch == 2) return launch_u<BV, 64, 2>(a, grid, st, ulevel);
    return launch_u<BV, 64, 4>(a, grid, st, ulevel);
}

// lane width from alignment: every lane reads / writes BV consecutive bf16 of a row
int pick_bv(const uint16_t *d_x, int64_t ldx, const uint16_t *d_y, int64_t ldy, int64_t d) {
    for (int bv = 8; bv > 1; bv >>= 1)
        if (d % bv == 0 && ldx % bv == 0 && ldy % bv == 0 && aligned_to(d_x, 2 * bv) && aligned_to(d_y, 2 * bv)) return bv;
    return 1;
}

int spmm_slice(sgl_csr_t *h, const uint16_t *d_x, int64_t ldx, uint16_t *d_y, int64_t ldy, int d, int bv, hipStream_t st,
               const AccEpi &ah, const char *who) {
    SpmmLaunch L;
    int rc = spmm_launch(L, h, d / bv, d, true, who);
    if (rc == SGL_OK) rc = grow_partial(h, L.ldp);
    if (rc != SGL_OK) return rc;
    if (L.grid == 0) return SGL_OK;

    Bf16Args a;
    a.items = h->d_items;
    a.pieces = h->d_pieces;
    a.rowptr = h->d_rowptr;
    a.col = h->d_col;
    a.val = h->d_val;
    a.x = d_x;
    a.y = d_y;
    a.ldx = ldx;
    a.ldy = ldy;
    a.ldp = L.ldp;
    a.n_items = (int32_t)h->n_items;
    a.n_pieces = (int32_t)h->n_pieces;
    a.d = d;
    a.epi = ah;
    a.rowmap = h->d_rowmap;
    a.map = L.map;
    a.partial = h->d_partial;
    hipError_t e;
    if (bv == 8)
        e = launch_group<8>(a, L.grid, st, L.ulevel, L.group, L.nch);
    else if (bv == 4)
        e = launch_group<4>(a, L.grid, st, L.ulevel, L.group, L.nch);
    else if (bv == 2)
        e = launch_group<2>(a, L.grid, st, L.ulevel, L.group, L.nch);
    else
        e = launch_group<1>(a, L.grid, st, L.ulevel, L.group, L.nch);
    if (e != hipSuccess) return sgl::fail((int)e, "%s: kernel launch failed: %s", who, hipGetErrorString(e));
    if (L.fixup_grid > 0) {
        hipLaunchKernelGGL(spmm_bf16_fixup_kernel, dim3((unsigned)L.fixup_grid), dim3(256), 0, st, h->d_rowmap ? h->d_long_out : h->d_long_row,
                           h->d_long_first, h->d_partial, a.ldp, d_y, ldy, d, a.epi);
        e = hipGetLastError();
        if (e != hipSuccess) return sgl::fail((int)e, "%s: fix-up launch failed: %s", who, hipGetErrorString(e));
    }
    return SGL_OK;
}

int spmm_impl(sgl_csr_t *h, const uint16_t *d_x, int64_t ldx, uint16_t *d_y, int64_t ldy, int64_t d, void *stream, AccEpi ah,
              const char *who) {
    if (!h) return sgl::fail(SGL_ERR_INVALID, "%s: NULL handle", who);
    SGL_REQUIRE(d >= 0 && d < INT32_MAX, "%s: bad d", who);
    SGL_REQUIRE_WIDTH(who, "d", d);
    if (d == 0 || h->n_rows == 0) return SGL_OK;
    SGL_REQUIRE(d_x && d_y, "%s: NULL X or Y", who);
    SGL_REQUIRE(ldx >= d && ldy >= d, "%s: leading dimension smaller than d", who);
    SGL_REQUIRE(aligned_to(d_x, 2) && aligned_to(d_y, 2), "%s: X/Y not 2-byte aligned", who);
    hipStream_t st = sgl::as_stream(stream);
    int bv = pick_bv(d_x, ldx, d_y, ldy, d);
    if (ah.acc) {
        SGL_REQUIRE(ah.ldacc >= d && aligned_to(ah.acc, 4), "%s: bad accumulator matrix", who);
        // the aggregate is read and written as 16-byte (BV >= 4) / 8-byte (BV = 2) vectors of floats
        if (bv >= 4 && !(ah.ldacc % 4 == 0 && aligned_to(ah.acc, 16))) bv = 2;
        if (bv == 2 && !(ah.ldacc % 2 == 0 && aligned_to(ah.acc, 8))) bv = 1;
    }
    const int64_t vcap = sgl::tuning("spmm_vec", 0);   // experiments: cap the lane width (2 or 1 elements)
    if ((vcap == 1 || vcap == 2) && vcap < bv) bv = (int)vcap;
    // one launch covers up to 64 lanes x 4 chunks x BV columns; wider matrices go in column slices
    const int64_t max_cols = 64 * 4 * bv;
    for (int64_t c0 = 0; c0 < d; c0 += max_cols) {
        const int dc = (int)std::min<int64_t>(max_cols, d - c0);
        AccEpi as = ah;
        if (as.acc) as.acc += c0;
        int rc = spmm_slice(h, d_x + c0, ldx, d_y + c0, ldy, dc, bv, st, as, who);
        if (rc != SGL_OK) return rc;
    }
    return SGL_OK;
}

// ---- row gathers that widen: out_h[i, :] = float(X_h[idx[i], :]) -------------------------------------------------------------
constexpr int kGatherMaxHops = 16;
struct GIn {
    const uint16_t *p[kGatherMaxHops];
    int64_t ld[kGatherMaxHops];
};
struct GOut {
    float *p[kGatherMaxHops];
    int64_t ld[kGatherMaxHops];
};

// Hop in blockIdx.y; a thread owns VEC columns of U rows: U index loads, U row loads, U stores, all independent (the shape of
// gather_hops_y_kernel, sgl_aggregate.hip).  d = data columns, dw >= d = columns written: [d, dw) is the destination's own padding
// and is written as zeros.  Nothing is read beyond column d of a source row.  The destination is written once and read by someone
// else: non-temporal stores.  An index outside [-n_rows, n_rows) cannot be reported from here without a trap: its output row is
// filled with NaN (host indices are validated before the launch).
template <int VEC, int U>
__global__ __launch_bounds__(256) void gather_bf16_kernel(const GIn hx, const GOut ho, const int64_t n_rows,
                                                          const int64_t *__restrict__ idx, const int64_t n_idx, const int d,
                                                          const int dw, const int lpr) {
    const int h = blockIdx.y;
    const uint16_t *__restrict__ x = hx.p[h];
    const int64_t ldx = hx.ld[h];
    float *__restrict__ out = ho.p[h];
    const int64_t ldo = ho.ld[h];
    const int rpb = 256 / lpr;
    const int l = threadIdx.x % lpr;
    const int64_t i0 = (int64_t)blockIdx.x * (rpb * U) + threadIdx.x / lpr;
    int64_t src[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int64_t i = i0 + (int64_t)u * rpb;
        int64_t s = i < n_idx ? idx[i] : 0;
        if (s < 0) s += n_rows;                       // python-style negative index
        if (s < 0 || s >= n_rows) s = -1;
        src[u] = s;
    }
    const float qnan = __uint_as_float(0x7fc00000u);
    for (int c = l * VEC; c < dw; c += lpr * VEC) {
        if constexpr (VEC == 4) {
            f4 v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                v[u] = (f4){0.f, 0.f, 0.f, 0.f};
                if (src[u] < 0) {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (c + e < d) v[u][e] = qnan;
                } else if (c + 4 <= d) {
                    const u2 r = *reinterpret_cast<const u2 *>(x + src[u] * ldx + c);
                    v[u] = (f4){widen_lo(r[0]), widen_hi(r[0]), widen_lo(r[1]), widen_hi(r[1])};
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (c + e < d) v[u][e] = __uint_as_float((uint32_t)x[src[u] * ldx + c + e] << 16);
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t i = i0 + (int64_t)u * rpb;
                if (i < n_idx) __builtin_nontemporal_store(v[u], reinterpret_cast<f4 *>(out + i * ldo + c));
            }
        } else {
            float v[U];
#pragma unroll
            for (int u = 0; u < U; ++u)
                v[u] = c >= d ? 0.f : (src[u] < 0 ? qnan : __uint_as_float((uint32_t)x[src[u] * ldx + c] << 16));
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t i = i0 + (int64_t)u * rpb;
                if (i < n_idx) __builtin_nontemporal_store(v[u], out + i * ldo + c);
            }
        }
    }
}

int gather_impl(const char *who, int n_hops, const uint16_t *const *h_x, const int64_t *h_ldx, int64_t n_rows, const int64_t *d_idx,
                int64_t n_idx, float *const *h_out, const int64_t *h_ldo, int64_t d, int64_t pad, void *stream) {
    SGL_REQUIRE(n_idx >= 0 && d >= 0 && pad >= 0 && n_rows >= 0 && d + pad < INT32_MAX, "%s: bad sizes", who);
    SGL_REQUIRE_WIDTH(who, "d + pad_cols", d + pad);
    SGL_REQUIRE(n_hops >= 1 && h_x && h_ldx && h_out && h_ldo, "%s: NULL hop arrays or n_hops < 1", who);
    if (n_hops > kGatherMaxHops)
        return sgl::fail(SGL_ERR_UNSUPPORTED, "%s: at most %d hop matrices per launch (gather hop by hop)", who, kGatherMaxHops);
    const int64_t dw = d + pad;
    GIn hx;
    GOut ho;
    bool vec4 = dw % 4 == 0;
    for (int h = 0; h < n_hops; ++h) {
        hx.p[h] = h_x[h];
        hx.ld[h] = h_ldx[h];
        ho.p[h] = h_out[h];
        ho.ld[h] = h_ldo[h];
        SGL_REQUIRE(n_idx == 0 || d == 0 || (hx.p[h] && ho.p[h]), "%s: hop %d: NULL matrix", who, h);
        SGL_REQUIRE(hx.ld[h] >= d && aligned_to(hx.p[h], 2), "%s: hop %d: source pitch < d or pointer not 2-byte aligned", who, h);
        SGL_REQUIRE(ho.ld[h] >= dw && aligned_to(ho.p[h], 4), "%s: output %d: pitch < d + pad_cols or pointer not 4-byte aligned", who, h);
        vec4 = vec4 && hx.ld[h] % 4 == 0 && aligned_to(hx.p[h], 8) && ho.ld[h] % 4 == 0 && aligned_to(ho.p[h], 16);
    }
    for (int h = n_hops; h < kGatherMaxHops; ++h) {
        hx.p[h] = nullptr;
        ho.p[h] = nullptr;
        hx.ld[h] = ho.ld[h] = 0;
    }
    if (n_idx == 0 || dw == 0) return SGL_OK;
    SGL_REQUIRE(d_idx != nullptr, "%s: NULL indices", who);
    SGL_REQUIRE(n_rows > 0, "%s: indices into a matrix without rows", who);
    const int vec = vec4 ? 4 : 1;
    int lpr = 8;
    while (lpr < 64 && (int64_t)lpr * vec < dw) lpr <<= 1;
    constexpr int U = 4;
    const int64_t blocks = (n_idx + (256 / lpr) * U - 1) / ((256 / lpr) * U);
    if (!sgl::launch_fits(blocks * n_hops, 256)) return sgl::fail(SGL_ERR_UNSUPPORTED, "%s: too many indices for one launch", who);
    hipStream_t st = sgl::as_stream(stream);
    if (vec4)
        hipLaunchKernelGGL((gather_bf16_kernel<4, U>), dim3((unsigned)blocks, (unsigned)n_hops), dim3(256), 0, st, hx, ho, n_rows, d_idx,
                           n_idx, (int)d, (int)dw, lpr);
    else
        hipLaunchKernelGGL((gather_bf16_kernel<1, U>), dim3((unsigned)blocks, (unsigned)n_hops), dim3(256), 0, st, hx, ho, n_rows, d_idx,
                           n_idx, (int)d, (int)dw, lpr);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return sgl::fail((int)e, "%s: kernel launch failed: %s", who, hipGetErrorString(e));
    return SGL_OK;
}

}  // namespace

SGL_EXPORT int sgl_spmm_bf16(sgl_csr_t *h, const uint16_t *d_x, int64_t ldx, uint16_t *d_y, int64_t ldy, int64_t d, void *stream) {
    return spmm_impl(h, d_x, ldx, d_y, ldy, d, stream, AccEpi(), "sgl_spmm_bf16");
}

SGL_EXPORT int sgl_spmm_chain_bf16(sgl_csr_t *h, int n_hops, const uint16_t *d_x0, int64_t ldx0, uint16_t *const *h_y,
                                   const int64_t *h_ldy, int64_t d, void *stream) {
    if (!h) return sgl::fail(SGL_ERR_INVALID, "sgl_spmm_chain_bf16: NULL handle");
    SGL_REQUIRE(n_hops >= 0 && (n_hops == 0 || (h_y && h_ldy)), "sgl_spmm_chain_bf16: bad hop arrays");
    SGL_REQUIRE(n_hops == 0 || h->n_rows == h->n_cols, "sgl_spmm_chain_bf16: repeated products need a square matrix");
    const uint16_t *cur = d_x0;
    int64_t ldc = ldx0;
    for (int k = 0; k < n_hops; ++k) {
        int rc = spmm_impl(h, cur, ldc, h_y[k], h_ldy[k], d, stream, AccEpi(), "sgl_spmm_chain_bf16");
        if (rc != SGL_OK) return rc;
        cur = h_y[k];
        ldc = h_ldy[k];
    }
    return SGL_OK;
}

SGL_EXPORT int sgl_spmm_acc_bf16(sgl_csr_t *h, const uint16_t *d_x, int64_t ldx, uint16_t *d_y, int64_t ldy, int64_t d, float *d_acc,
                                 int64_t ldacc, float w, int mode, float divisor, void *stream) {
    AccEpi ah;
    const int rc = acc_mode_of("sgl_spmm_acc_bf16", d_acc, mode, divisor, ah.acc_mode);
    if (rc != SGL_OK) return rc;
    ah.acc = d_acc;
    ah.ldacc = ldacc;
    ah.acc_w = w;
    ah.acc_div = divisor;
    return spmm_impl(h, d_x, ldx, d_y, ldy, d, stream, ah, "sgl_spmm_acc_bf16");
}

SGL_EXPORT int sgl_gather_rows_bf16_f32(const uint16_t *d_x, int64_t ldx, int64_t n_rows, const int64_t *d_idx, int64_t n_idx,
                                        float *d_out, int64_t ldo, int64_t d, int64_t pad_cols, void *stream) {
    const uint16_t *xs[1] = {d_x};
    float *os[1] = {d_out};
    return gather_impl("sgl_gather_rows_bf16_f32", 1, xs, &ldx, n_rows, d_idx, n_idx, os, &ldo, d, pad_cols, stream);
}

SGL_EXPORT int sgl_gather_hops_bf16_f32(int n_hops, const uint16_t *const *h_x, const int64_t *h_ldx, int64_t n_rows,
                                        const int64_t *d_idx, int64_t n_idx, float *const *h_out, const int64_t *h_ldo, int64_t d,
                                        int64_t pad_cols, void *stream) {
    return gather_impl("sgl_gather_hops_bf16_f32", n_hops, h_x, h_ldx, n_rows, d_idx, n_idx, h_out, h_ldo, d, pad_cols, stream);
}
