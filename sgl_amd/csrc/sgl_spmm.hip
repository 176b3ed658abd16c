// CSR x dense fp32 SpMM for gfx950 (MI355X) -- the k-step A_hat . X kernel of GraphOp.propagate
// (reference: sgl/operators/base_op.py:29-35 -> csrc/matmul.c:23-40; successor of the dead cuSPARSE twin
// csrc/cudamatmul.c:104-119).
//
// Design:
//   * the path is sparse x dense, ~0.5 flop/byte: HBM/cache bound, no MFMA;
//   * one 64-lane wavefront owns one work item = a run of <= 63 whole rows holding ~item_nnz non-zeros
//     (host-built plan, sgl_core.cpp); very long rows are cut into pieces whose partial sums are combined by a
//     deterministic fix-up pass (no float atomics);
//   * inside a wavefront, lanes are laid out as R "non-zero slots" x GROUP "feature lanes" (R*GROUP = 64):
//     every step gathers R rows of X, each read as one contiguous, 16-byte-per-lane segment (coalesced), and
//     FMAs them into per-lane fp32 accumulators; the R slot accumulators are folded with a butterfly of
//     cross-lane shuffles when the row ends (wavefront-level reduction).  R = 1 walks the row in storage order
//     with one fmaf per non-zero = the reference's exact chain (bit-exact mode);
//   * the item's (col, val) stream is read as coalesced 64-element slices that stay in registers and are
//     broadcast to the slots through the LDS crossbar (ds_bpermute / v_readlane): the next slice is prefetched
//     while the current one is consumed, so the CSR stream never stalls the gathers;
//   * U independent gathers are kept in flight per lane (memory-level parallelism), x up to 8 waves per SIMD;
//   * block -> item mapping is XCD-aware: each of the 8 XCDs walks its own contiguous range of rows, so rows that
//     share neighbours (and the CSR stream) stay in one XCD's L2.
#include "sgl_spmm_common.h"

namespace {

template <int VEC>
struct VecT;
template <>
struct VecT<1> {
    using type = float;
};
template <>
struct VecT<2> {
    using type = float __attribute__((ext_vector_type(2)));
};
template <>
struct VecT<4> {
    using type = float __attribute__((ext_vector_type(4)));
};

template <int VEC>
__device__ __forceinline__ typename VecT<VEC>::type vzero() {
    typename VecT<VEC>::type z;
    if constexpr (VEC == 1) {
        z = 0.f;
    } else {
#pragma unroll
        for (int e = 0; e < VEC; ++e) z[e] = 0.f;
    }
    return z;
}

template <int VEC>
__device__ __forceinline__ void vfma(typename VecT<VEC>::type &acc, float v, const typename VecT<VEC>::type &x) {
    if constexpr (VEC == 1) {
        acc = __builtin_fmaf(v, x, acc);
    } else {
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[e] = __builtin_fmaf(v, x[e], acc[e]);
    }
}

template <int VEC>
__device__ __forceinline__ void vadd_xor(typename VecT<VEC>::type &acc, int off) {
    if constexpr (VEC == 1) {
        acc += __shfl_xor(acc, off, 64);
    } else {
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[e] += __shfl_xor(acc[e], off, 64);
    }
}

template <bool NT, typename T>
__device__ __forceinline__ T ld_stream(const T *p) {
    if constexpr (NT)
        return __builtin_nontemporal_load(p);
    else
        return *p;
}

template <bool NT, typename T>
__device__ __forceinline__ void st_stream(T *p, const T &v) {
    if constexpr (NT)
        __builtin_nontemporal_store(v, p);
    else
        *p = v;
}

struct SpmmArgs {
    const int32_t *items;       // (row_begin,row_end) pairs
    const sgl::Piece *pieces;   // long-row pieces
    const int64_t *rowptr;
    const int32_t *col;
    const float *val;
    const float *x;
    float *y;
    float *partial;
    int64_t ldx, ldy, ldp;
    int32_t n_items, n_pieces, d, accumulate;
    BlockMap map;
    // optional fused epilogue  Y = clamp(alpha * (A X) + res, lo, hi)   (label propagation / C&S step,
    // reference: sgl/tricks/utils.py:55-56); epi == 0 -> plain store
    const float *res;
    int64_t ldres;
    float epi_alpha, epi_lo, epi_hi;
    int32_t epi;
    float *acc;                 // optional running aggregate (see Epilogue)
    int64_t ldacc;
    float acc_w, acc_div;
    int32_t acc_mode;
    // optional replicas of Y: every output row is ALSO stored at the same (row, column) offset of these matrices
    // (same leading dimension as y).  Used to push a rank's new rows straight into the peers' feature replicas
    // over xGMI from the producing kernel (sgl_spmm_multi_f32); n_more == 0 otherwise.
    float *y_more[7];
    int32_t n_more;
    const uint8_t *row_mask;   // optional [n_rows]: bit q set = replica q needs this row (NULL = every replica gets it)
    const int32_t *rowmap;     // optional [n_rows]: storage row -> output row (sgl_csr_set_rowmap); NULL = identity
};

struct MultiOut {
    float *p[7];   // already offset to the item's first row
    int n;
    const uint8_t *mask;   // already offset to the item's first row (or nullptr)
};

struct Epilogue {
    const float *res = nullptr;   // row pointer already applied by the caller (may be nullptr)
    float alpha = 1.f, lo = 0.f, hi = 0.f;
    int on = 0;
    // running aggregate over hops (acc_apply, sgl_spmm_common.h)
    float *acc = nullptr;         // row pointer already applied (nullptr = off)
    int64_t ldacc = 0;
    float acc_w = 1.f, acc_div = 1.f;
    int acc_mode = 0;
};

__device__ __forceinline__ float acc_apply(float a, float y, const Epilogue &e) { return acc_apply(a, y, e.acc_mode, e.acc_w, e.acc_div); }

__device__ __forceinline__ float epi_apply(float v, float r, const Epilogue &e, bool has_res) {
    float t = __fmul_rn(e.alpha, v);          // alpha * spmm(...)   (rounded product, then rounded add: torch order)
    if (has_res) t = __fadd_rn(t, r);
    return t < e.lo ? e.lo : (t > e.hi ? e.hi : t);   // clamp that keeps NaN, like torch.clamp_
}

// One wavefront walks `nrows` consecutive rows whose non-zeros are colb/valb[0 .. tot) ; lane i of `my_rel`
// holds the offset of row i's first non-zero (lane nrows holds tot).
// Under a row map (RowMap, sgl_spmm_common.h) `out`, the residual and the running aggregate are un-offset base pointers.
template <int VEC, int GROUP, int NCH, int U, bool NT, bool MULTI>
__device__ __forceinline__ void run_rows(const int32_t *__restrict__ colb, const float *__restrict__ valb,
                                         const int my_rel, const int nrows, const int tot,
                                         const float *__restrict__ x, const int64_t ldx, float *__restrict__ out,
                                         const int64_t ldo, const int d, const bool accumulate, const int lane,
                                         const Epilogue epi, const int64_t ldres, const MultiOut mo,
                                         const RowMap rm = RowMap()) {
    using V = typename VecT<VEC>::type;
    constexpr int R = 64 / GROUP;
    const int s = (R == 1) ? 0 : (lane / GROUP);
    const int l = lane % GROUP;
    int colofs[NCH];
    bool on[NCH];
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
        colofs[ch] = (ch * GROUP + l) * VEC;
        on[ch] = colofs[ch] < d;
    }
    // current / next 64-element slice of the (col,val) stream, one element per lane
    int cbr = 0;
    int my_c = 0, nx_c = 0;
    float my_v = 0.f, nx_v = 0.f;
    if (lane < tot) {
        my_c = ld_stream<NT>(colb + lane);
        my_v = ld_stream<NT>(valb + lane);
    }
    if (64 + lane < tot) {
        nx_c = ld_stream<NT>(colb + 64 + lane);
        nx_v = ld_stream<NT>(valb + 64 + lane);
    }

    for (int ri = 0; ri < nrows; ++ri) {
        const int jb = __builtin_amdgcn_readlane(my_rel, ri);
        const int je = __builtin_amdgcn_readlane(my_rel, ri + 1);
        const int64_t ro = rm.on ? (int64_t)__builtin_amdgcn_readlane(rm.my_map, ri) : (int64_t)ri;   // output row
        float *orow = out + ro * ldo;
        V acc[NCH];
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) acc[ch] = vzero<VEC>();
        if (accumulate && s == 0) {
#pragma unroll
            for (int ch = 0; ch < NCH; ++ch)
                if (on[ch]) acc[ch] = *reinterpret_cast<const V *>(orow + colofs[ch]);
        }
        int j = jb;
        while (j < je) {
            const int lim = min(je, cbr + 64);
            const int o = j - cbr;
            const int cnt = lim - j;
            // slot of a non-zero = its index WITHIN ITS ROW mod R, not its index within this chunk: the chunk boundaries are
            // the 64-element slices of the item's stream, i.e. they depend on which rows share the item.  With the row-relative
            // assignment every slot adds the same terms in the same order under any plan and any processing order of the rows
            // (row maps, other item sizes): packed layouts (d <= 64) are bit-reproducible across plans like the R = 1 walk.
            const int sh = (R == 1) ? 0 : ((s - (j - jb)) & (R - 1));
            int t = 0;
            for (; t + R * U <= cnt; t += R * U) {
                int c[U];
                float v[U];
                V xv[U][NCH];
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
                            xv[u][ch] = *reinterpret_cast<const V *>(x + (int64_t)c[u] * ldx + colofs[ch]);
                    } else {
#pragma unroll
                        for (int u = 0; u < U; ++u) xv[u][ch] = vzero<VEC>();
                    }
                }
#pragma unroll
                for (int u = 0; u < U; ++u)
#pragma unroll
                    for (int ch = 0; ch < NCH; ++ch) vfma<VEC>(acc[ch], v[u], xv[u][ch]);
            }
            for (; t < cnt; t += R) {
                const int idx = (o + t + sh) & 63;
                const bool valid = (t + sh) < cnt;
                const int c = bcast_i<R>(my_c, idx);
                const float v = bcast_f<R>(my_v, idx);
                if (valid) {
#pragma unroll
                    for (int ch = 0; ch < NCH; ++ch)
                        if (on[ch]) {
                            const V xv = *reinterpret_cast<const V *>(x + (int64_t)c * ldx + colofs[ch]);
                            vfma<VEC>(acc[ch], v, xv);
                        }
                }
            }
            j = lim;
            if (lim == cbr + 64) {  // slice exhausted: rotate, prefetch the one after next
                cbr += 64;
                my_c = nx_c;
                my_v = nx_v;
                if (cbr + 64 + lane < tot) {
                    nx_c = ld_stream<NT>(colb + cbr + 64 + lane);
                    nx_v = ld_stream<NT>(valb + cbr + 64 + lane);
                }
            }
        }
        if constexpr (R > 1) {
#pragma unroll
            for (int off = GROUP; off < 64; off <<= 1)
#pragma unroll
                for (int ch = 0; ch < NCH; ++ch) vadd_xor<VEC>(acc[ch], off);
        }
        if (s == 0) {
#pragma unroll
            for (int ch = 0; ch < NCH; ++ch)
                if (on[ch]) {
                    V v = acc[ch];
                    if (epi.on) {
                        const bool has_res = epi.res != nullptr;
                        V r = vzero<VEC>();
                        if (has_res) r = *reinterpret_cast<const V *>(epi.res + ro * ldres + colofs[ch]);
                        if constexpr (VEC == 1) {
                            v = epi_apply(v, r, epi, has_res);
                        } else {
#pragma unroll
                            for (int e = 0; e < VEC; ++e) v[e] = epi_apply(v[e], r[e], epi, has_res);
                        }
                    }
                    if (epi.acc) {
                        float *ap = epi.acc + ro * epi.ldacc + colofs[ch];
                        V a = *reinterpret_cast<const V *>(ap);
                        if constexpr (VEC == 1) {
                            a = acc_apply(a, v, epi);
                        } else {
#pragma unroll
                            for (int e = 0; e < VEC; ++e) a[e] = acc_apply(a[e], v[e], epi);
                        }
                        *reinterpret_cast<V *>(ap) = a;   // (non-temporal hints on this stream measured slower: +4.4 vs +4.1 ms / 10 hops)
                    }
                    st_stream<NT>(reinterpret_cast<V *>(orow + colofs[ch]), v);
                    if constexpr (MULTI) {
                        const int need = mo.mask ? (int)mo.mask[ri] : 0x7f;   // wave-uniform: one byte per row
#pragma unroll
                        for (int q = 0; q < 7; ++q)  // replicas (peer memory): posted stores, nothing waits on them
                            if (q < mo.n && ((need >> q) & 1))
                                *reinterpret_cast<V *>(mo.p[q] + ro * ldo + colofs[ch]) = v;
                    }
                }
        }
    }
}

template <int VEC, int GROUP, int NCH, int U, bool NT, bool MULTI>
__global__ __launch_bounds__(256) void spmm_kernel(const SpmmArgs a) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.x;
    if (b < a.map.piece_blocks) {
        const int p = b * a.map.waves + wave;
        if (p >= a.n_pieces) return;
        const sgl::Piece pc = a.pieces[p];
        const int my_rel = (lane == 0) ? 0 : pc.len;
        const Epilogue none;   // pieces hold partial sums: the epilogue runs in the fix-up kernel
        MultiOut solo;
        solo.n = 0;
        solo.mask = nullptr;
        run_rows<VEC, GROUP, NCH, U, NT, false>(a.col + pc.begin, a.val + pc.begin, my_rel, 1, pc.len, a.x, a.ldx,
                                         a.partial + (int64_t)p * a.ldp, a.ldp, a.d, false, lane, none, 0, solo);
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
        Epilogue epi;
        epi.res = a.res ? a.res + first * a.ldres : nullptr;
        epi.alpha = a.epi_alpha;
        epi.lo = a.epi_lo;
        epi.hi = a.epi_hi;
        epi.on = a.epi;
        epi.acc = a.acc ? a.acc + first * a.ldacc : nullptr;
        epi.ldacc = a.ldacc;
        epi.acc_w = a.acc_w;
        epi.acc_div = a.acc_div;
        epi.acc_mode = a.acc_mode;
        MultiOut mo;
        mo.n = MULTI ? a.n_more : 0;
        mo.mask = (MULTI && a.row_mask) ? a.row_mask + row_begin : nullptr;
#pragma unroll
        for (int q = 0; q < 7; ++q) mo.p[q] = (MULTI && q < a.n_more) ? a.y_more[q] + (int64_t)row_begin * a.ldy : nullptr;
        run_rows<VEC, GROUP, NCH, U, NT, MULTI>(a.col + w.base, a.val + w.base, w.my_rel, nrows, w.tot, a.x, a.ldx,
                                         a.y + first * a.ldy, a.ldy, a.d, a.accumulate != 0, lane, epi,
                                         a.ldres, mo, rm);
    }
}

// Y[row, :] = (accumulate ? Y[row, :] : 0) + sum of the row's piece partials, in storage order.
__global__ __launch_bounds__(256) void spmm_fixup_kernel(const int32_t *__restrict__ long_row,
                                                         const int32_t *__restrict__ long_first,
                                                         const float *__restrict__ partial, int64_t ldp,
                                                         float *__restrict__ y, int64_t ldy, int d, int accumulate,
                                                         const float *__restrict__ res, int64_t ldres, Epilogue epi,
                                                         MultiOut mo) {
    const int kblocks = (d + 255) / 256;
    const int lr = blockIdx.x / kblocks;
    const int k = (blockIdx.x % kblocks) * 256 + threadIdx.x;
    if (k >= d) return;
    const int row = long_row[lr];
    const int p0 = long_first[lr], p1 = long_first[lr + 1];
    float *yp = y + (int64_t)row * ldy + k;
    float acc = accumulate ? *yp : 0.f;
    for (int p = p0; p < p1; ++p) acc += partial[(int64_t)p * ldp + k];
    if (epi.on) acc = epi_apply(acc, res ? res[(int64_t)row * ldres + k] : 0.f, epi, res != nullptr);
    if (epi.acc) {   // here epi.acc is the matrix base (rows are absolute in the fix-up)
        float *ap = epi.acc + (int64_t)row * epi.ldacc + k;
        *ap = acc_apply(*ap, acc, epi);
    }
    *yp = acc;
    const int need = mo.mask ? (int)mo.mask[row] : 0x7f;
#pragma unroll
    for (int q = 0; q < 7; ++q)
        if (q < mo.n && ((need >> q) & 1)) mo.p[q][(int64_t)row * ldy + k] = acc;
}

template <int VEC, int GROUP, int NCH, int U, bool NT>
hipError_t launch_variant(const SpmmArgs &a, int grid, hipStream_t st) {
    if (a.n_more > 0)
        hipLaunchKernelGGL((spmm_kernel<VEC, GROUP, NCH, U, NT, true>), dim3(grid), dim3(64 * a.map.waves), 0, st, a);
    else
        hipLaunchKernelGGL((spmm_kernel<VEC, GROUP, NCH, U, NT, false>), dim3(grid), dim3(64 * a.map.waves), 0, st, a);
    return hipGetLastError();
}

template <int VEC, int GROUP, int NCH, int U>
hipError_t launch_nt(const SpmmArgs &a, int grid, hipStream_t st, bool nt) {
    return nt ? launch_variant<VEC, GROUP, NCH, U, true>(a, grid, st)
              : launch_variant<VEC, GROUP, NCH, U, false>(a, grid, st);
}

template <int VEC, int GROUP, int NCH>
hipError_t launch_u(const SpmmArgs &a, int grid, hipStream_t st, bool nt, int ulevel) {
    using sgl::unroll_of;
    if (ulevel == 2) return launch_nt<VEC, GROUP, NCH, unroll_of(GROUP, NCH, 2)>(a, grid, st, nt);
    if (ulevel == 3) return launch_nt<VEC, GROUP, NCH, unroll_of(GROUP, NCH, 3)>(a, grid, st, nt);
    return ulevel == 0 ? launch_nt<VEC, GROUP, NCH, unroll_of(GROUP, NCH, 0)>(a, grid, st, nt)
                       : launch_nt<VEC, GROUP, NCH, unroll_of(GROUP, NCH, 1)>(a, grid, st, nt);
}

template <int VEC>
hipError_t launch_group(const SpmmArgs &a, int grid, hipStream_t st, bool nt, int ulevel, int group, int nch) {
    if (nch == 1) {
        switch (group) {
            case 8:
                return launch_u<VEC, 8, 1>(a, grid, st, nt, ulevel);
            case 16:
                return launch_u<VEC, 16, 1>(a, grid, st, nt, ulevel);
            case 32:
                return launch_u<VEC, 32, 1>(a, grid, st, nt, ulevel);
            default:
                return launch_u<VEC, 64, 1>(a, grid, st, nt, ulevel);
        }
    }
    if (nch == 2) return launch_u<VEC, 64, 2>(a, grid, st, nt, ulevel);
    return launch_u<VEC, 64, 4>(a, grid, st, nt, ulevel);
}

}  // namespace

static int pick_vec(const float *d_x, int64_t ldx, const float *d_y, int64_t ldy, int64_t d) {
    // vector width from alignment: every lane reads/writes VEC consecutive floats of a row
    if (d % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0 && aligned_to(d_x, 16) && aligned_to(d_y, 16)) return 4;
    if (d % 2 == 0 && ldx % 2 == 0 && ldy % 2 == 0 && aligned_to(d_x, 8) && aligned_to(d_y, 8)) return 2;
    return 1;
}

struct EpiHost {
    int on = 0;
    float alpha = 1.f, lo = 0.f, hi = 0.f;
    const float *res = nullptr;
    int64_t ldres = 0;
    int n_more = 0;             // replicas of Y (sgl_spmm_multi_f32)
    float *y_more[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    const uint8_t *row_mask = nullptr;
    // running aggregate (sgl_spmm_acc_f32)
    float *acc = nullptr;
    int64_t ldacc = 0;
    float acc_w = 1.f, acc_div = 1.f;
    int acc_mode = 0;
};

static int spmm_slice(sgl_csr_t *h, const float *d_x, int64_t ldx, float *d_y, int64_t ldy, int d, int vec,
                      int accumulate, hipStream_t st, const EpiHost &eh, const char *who) {
    SpmmLaunch L;
    int rc = spmm_launch(L, h, d / vec, d, false, who);
    if (rc == SGL_OK) rc = grow_partial(h, L.ldp);
    if (rc != SGL_OK) return rc;
    if (L.grid == 0) return SGL_OK;

    SpmmArgs a;
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
    a.accumulate = accumulate;
    a.res = eh.res;
    a.ldres = eh.ldres;
    a.epi_alpha = eh.alpha;
    a.epi_lo = eh.lo;
    a.epi_hi = eh.hi;
    a.epi = eh.on;
    a.acc = eh.acc;
    a.ldacc = eh.ldacc;
    a.acc_w = eh.acc_w;
    a.acc_div = eh.acc_div;
    a.acc_mode = eh.acc_mode;
    a.n_more = eh.n_more;
    a.row_mask = eh.row_mask;
    for (int q = 0; q < 7; ++q) a.y_more[q] = eh.y_more[q];
    a.rowmap = h->d_rowmap;
    a.map = L.map;
    a.partial = h->d_partial;
    hipError_t e;
    if (vec == 4)
        e = launch_group<4>(a, L.grid, st, L.nt, L.ulevel, L.group, L.nch);
    else if (vec == 2)
        e = launch_group<2>(a, L.grid, st, L.nt, L.ulevel, L.group, L.nch);
    else
        e = launch_group<1>(a, L.grid, st, L.nt, L.ulevel, L.group, L.nch);
    if (e != hipSuccess) return sgl::fail((int)e, "%s: kernel launch failed: %s", who, hipGetErrorString(e));
    if (L.fixup_grid > 0) {
        Epilogue fe;   // (the fix-up takes the residual's base as an argument of its own)
        fe.alpha = eh.alpha;
        fe.lo = eh.lo;
        fe.hi = eh.hi;
        fe.on = eh.on;
        fe.acc = eh.acc;
        fe.ldacc = eh.ldacc;
        fe.acc_w = eh.acc_w;
        fe.acc_div = eh.acc_div;
        fe.acc_mode = eh.acc_mode;
        MultiOut fmo;
        fmo.n = eh.n_more;
        fmo.mask = eh.row_mask;
        for (int q = 0; q < 7; ++q) fmo.p[q] = eh.y_more[q];
        hipLaunchKernelGGL(spmm_fixup_kernel, dim3((unsigned)L.fixup_grid), dim3(256), 0, st, h->d_rowmap ? h->d_long_out : h->d_long_row,
                           h->d_long_first, h->d_partial, a.ldp,
                           d_y, ldy, d, accumulate, eh.res, eh.ldres, fe, fmo);
        e = hipGetLastError();
        if (e != hipSuccess) return sgl::fail((int)e, "%s: fix-up launch failed: %s", who, hipGetErrorString(e));
    }
    return SGL_OK;
}

static int spmm_impl(sgl_csr_t *h, const float *d_x, int64_t ldx, float *d_y, int64_t ldy, int64_t d, int accumulate,
                     void *stream, EpiHost eh, const char *who) {
    if (!h) return sgl::fail(SGL_ERR_INVALID, "%s: NULL handle", who);
    SGL_REQUIRE(d >= 0 && d < INT32_MAX, "%s: bad d", who);
    SGL_REQUIRE_WIDTH(who, "d", d);
    if (d == 0 || h->n_rows == 0) return SGL_OK;
    SGL_REQUIRE(d_x && d_y, "%s: NULL X or Y", who);
    if (h->d_rowmap && eh.n_more > 0)
        return sgl::fail(SGL_ERR_UNSUPPORTED, "%s: a row-mapped handle does not support replicas", who);
    SGL_REQUIRE(ldx >= d && ldy >= d, "%s: leading dimension smaller than d", who);
    SGL_REQUIRE(aligned_to(d_x, 4) && aligned_to(d_y, 4), "%s: X/Y not 4-byte aligned", who);
    hipStream_t st = sgl::as_stream(stream);
    // one launch covers up to 64 lanes x 4 chunks x VEC columns; wider matrices go in column slices
    int vec = pick_vec(d_x, ldx, d_y, ldy, d);
    for (int q = 0; q < eh.n_more; ++q) {
        SGL_REQUIRE(eh.y_more[q] && aligned_to(eh.y_more[q], 4), "%s: bad replica pointer", who);
        if (vec == 4 && !aligned_to(eh.y_more[q], 16)) vec = aligned_to(eh.y_more[q], 8) && d % 2 == 0 ? 2 : 1;
        if (vec == 2 && !aligned_to(eh.y_more[q], 8)) vec = 1;
    }
    const int64_t vcap = sgl::tuning("spmm_vec", 0);   // experiments: cap the lane width (2 or 1 floats)
    if ((vcap == 1 || vcap == 2) && vcap < vec) vec = (int)vcap;
    if (eh.on && eh.res) {
        SGL_REQUIRE(eh.ldres >= d && aligned_to(eh.res, 4), "%s: bad residual matrix", who);
        if (vec == 4 && !(eh.ldres % 4 == 0 && aligned_to(eh.res, 16))) vec = (eh.ldres % 2 == 0 && aligned_to(eh.res, 8) && d % 2 == 0) ? 2 : 1;
        if (vec == 2 && !(eh.ldres % 2 == 0 && aligned_to(eh.res, 8))) vec = 1;
    }
    if (eh.acc) {
        SGL_REQUIRE(eh.ldacc >= d && aligned_to(eh.acc, 4), "%s: bad accumulator matrix", who);
        if (vec == 4 && !(eh.ldacc % 4 == 0 && aligned_to(eh.acc, 16))) vec = (eh.ldacc % 2 == 0 && aligned_to(eh.acc, 8) && d % 2 == 0) ? 2 : 1;
        if (vec == 2 && !(eh.ldacc % 2 == 0 && aligned_to(eh.acc, 8))) vec = 1;
    }
    const int64_t max_cols = 64 * 4 * vec;
    for (int64_t c0 = 0; c0 < d; c0 += max_cols) {
        const int dc = (int)std::min<int64_t>(max_cols, d - c0);
        EpiHost es = eh;
        if (es.res) es.res += c0;
        if (es.acc) es.acc += c0;
        for (int q = 0; q < es.n_more; ++q) es.y_more[q] += c0;
        int rc = spmm_slice(h, d_x + c0, ldx, d_y + c0, ldy, dc, vec, accumulate, st, es, who);
        if (rc != SGL_OK) return rc;
    }
    return SGL_OK;
}

SGL_EXPORT int sgl_spmm_f32(sgl_csr_t *h, const float *d_x, int64_t ldx, float *d_y, int64_t ldy, int64_t d,
                            int accumulate, void *stream) {
    return spmm_impl(h, d_x, ldx, d_y, ldy, d, accumulate, stream, EpiHost(), "sgl_spmm_f32");
}

// Y_0 = Y_1 = ... = A X: the product is stored into n_out matrices (same leading dimension).  Matrix 0 is normally
// local; the others may live in PEER GPUs' memory (IPC / symmetric-memory mappings): the producing wavefront pushes
// its finished rows straight into every peer's replica of the feature block over xGMI -- the all-gather between
// hops without copy kernels, staging buffers or a separate communication phase.
SGL_EXPORT int sgl_spmm_multi_f32(sgl_csr_t *h, const float *d_x, int64_t ldx, int n_out, float *const *h_y, int64_t ldy,
                                  int64_t d, const uint8_t *d_row_mask, void *stream) {
    SGL_REQUIRE(n_out >= 1 && n_out <= 8 && h_y, "sgl_spmm_multi_f32: n_out must be in [1, 8]");
    EpiHost eh;
    eh.row_mask = d_row_mask;
    eh.n_more = n_out - 1;
    for (int q = 1; q < n_out; ++q) eh.y_more[q - 1] = h_y[q];
    return spmm_impl(h, d_x, ldx, h_y[0], ldy, d, 0, stream, eh, "sgl_spmm_multi_f32");
}

// X_1 = A X_0, X_2 = A X_1, ... : the whole hop loop of GraphOp.propagate (base_op.py:29-35) issued from one call, so a
// small graph (Pubmed: tens of microseconds of kernel time per hop) is not dominated by per-hop host overhead.
SGL_EXPORT int sgl_spmm_chain_f32(sgl_csr_t *h, int n_hops, const float *d_x0, int64_t ldx0, float *const *h_y,
                                  const int64_t *h_ldy, int64_t d, void *stream) {
    if (!h) return sgl::fail(SGL_ERR_INVALID, "sgl_spmm_chain_f32: NULL handle");
    SGL_REQUIRE(n_hops >= 0 && (n_hops == 0 || (h_y && h_ldy)), "sgl_spmm_chain_f32: bad hop arrays");
    SGL_REQUIRE(n_hops == 0 || h->n_rows == h->n_cols, "sgl_spmm_chain_f32: repeated products need a square matrix");
    const float *cur = d_x0;
    int64_t ldc = ldx0;
    for (int k = 0; k < n_hops; ++k) {
        int rc = spmm_impl(h, cur, ldc, h_y[k], h_ldy[k], d, 0, stream, EpiHost(), "sgl_spmm_chain_f32");
        if (rc != SGL_OK) return rc;
        cur = h_y[k];
        ldc = h_ldy[k];
    }
    return SGL_OK;
}

// ---- hipGraph of a whole propagate(): for small graphs (Pubmed / Cora sized) each hop is a few tens of microseconds
// of kernel time, so the k launches (+ fix-ups) are captured once and replayed with a single hipGraphLaunch.
struct sgl_graph {
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    std::shared_ptr<std::atomic<uint64_t>> epoch;   // the handle's change counter and its value at capture time
    uint64_t captured = 0;
};

SGL_EXPORT int sgl_chain_graph_create(sgl_graph_t **out, sgl_csr_t *h, int n_hops, const float *d_x0, int64_t ldx0,
                                      float *const *h_y, const int64_t *h_ldy, int64_t d) {
    if (!out) return sgl::fail(SGL_ERR_INVALID, "sgl_chain_graph_create: NULL out");
    *out = nullptr;
    SGL_REQUIRE(h && n_hops >= 1 && h_y && h_ldy, "sgl_chain_graph_create: bad arguments");
    SGL_REQUIRE_WIDTH("sgl_chain_graph_create", "d", d);   // under its own name: every other argument is checked by the eager chain below
    // everything that may allocate or synchronise happens BEFORE the capture: one eager run sizes the split-row
    // workspace (and validates the arguments)
    int rc = sgl_spmm_chain_f32(h, n_hops, d_x0, ldx0, h_y, h_ldy, d, nullptr);
    if (rc != SGL_OK) return rc;
    SGL_HIP_CHECK(hipDeviceSynchronize());
    hipStream_t cap = nullptr;
    SGL_HIP_CHECK(hipStreamCreateWithFlags(&cap, hipStreamNonBlocking));
    sgl_graph_t *g = new (std::nothrow) sgl_graph_t();
    if (!g) {
        (void)hipStreamDestroy(cap);
        return sgl::fail(SGL_ERR_ALLOC, "sgl_chain_graph_create: out of memory");
    }
    hipError_t e = hipStreamBeginCapture(cap, hipStreamCaptureModeThreadLocal);
    if (e == hipSuccess) {
        rc = sgl_spmm_chain_f32(h, n_hops, d_x0, ldx0, h_y, h_ldy, d, cap);
        e = hipStreamEndCapture(cap, &g->graph);
        if (rc != SGL_OK && e == hipSuccess) e = hipErrorUnknown;
    }
    if (e == hipSuccess) e = hipGraphInstantiate(&g->exec, g->graph, nullptr, nullptr, 0);
    (void)hipStreamDestroy(cap);
    if (e != hipSuccess) {
        if (g->graph) (void)hipGraphDestroy(g->graph);
        delete g;
        return sgl::fail((int)e, "sgl_chain_graph_create: capture/instantiate failed: %s", hipGetErrorString(e));
    }
    g->epoch = h->epoch;
    g->captured = h->epoch->load();
    *out = g;
    return SGL_OK;
}

SGL_EXPORT int sgl_chain_graph_launch(sgl_graph_t *g, void *stream) {
    if (!g || !g->exec) return sgl::fail(SGL_ERR_INVALID, "sgl_chain_graph_launch: NULL graph");
    if (g->epoch && g->epoch->load() != g->captured)
        return sgl::fail(SGL_ERR_INVALID, "sgl_chain_graph_launch: the adjacency handle changed after the capture (new values / row map, "
                                          "or it was destroyed): capture the chain again");
    SGL_HIP_CHECK(hipGraphLaunch(g->exec, sgl::as_stream(stream)));
    return SGL_OK;
}

SGL_EXPORT int sgl_chain_graph_destroy(sgl_graph_t *g) {
    if (!g) return SGL_OK;
    if (g->exec) (void)hipGraphExecDestroy(g->exec);
    if (g->graph) (void)hipGraphDestroy(g->graph);
    delete g;
    return SGL_OK;
}

// Y = A X  and, in the same pass,  ACC <- ACC + w * Y  [ / divisor ]  or  ACC <- max / min(ACC, Y): the running aggregate of
// the Sum / Mean / SimpleWeighted / Max / Min MessageOps (message_op/{sum,mean,simple_weighted,max,min}_message_op.py) kept
// up to date where each row is produced, so those aggregators need no pass of their own over the hop matrices and no hop
// needs to be kept.
SGL_EXPORT int sgl_spmm_acc_f32(sgl_csr_t *h, const float *d_x, int64_t ldx, float *d_y, int64_t ldy, int64_t d, float *d_acc,
                                int64_t ldacc, float w, int mode, float divisor, void *stream) {
    EpiHost eh;
    const int rc = acc_mode_of("sgl_spmm_acc_f32", d_acc, mode, divisor, eh.acc_mode);
    if (rc != SGL_OK) return rc;
    eh.acc = d_acc;
    eh.ldacc = ldacc;
    eh.acc_w = w;
    eh.acc_div = divisor;
    return spmm_impl(h, d_x, ldx, d_y, ldy, d, 0, stream, eh, "sgl_spmm_acc_f32");
}

SGL_EXPORT int sgl_spmm_axpb_clamp_f32(sgl_csr_t *h, const float *d_x, int64_t ldx, float *d_y, int64_t ldy, int64_t d,
                                       float alpha, const float *d_res, int64_t ldres, float lo, float hi,
                                       void *stream) {
    EpiHost eh;
    eh.on = 1;
    eh.alpha = alpha;
    eh.lo = lo;
    eh.hi = hi;
    eh.res = d_res;
    eh.ldres = ldres;
    SGL_REQUIRE(!(lo > hi), "sgl_spmm_axpb_clamp_f32: lo > hi");
    return spmm_impl(h, d_x, ldx, d_y, ldy, d, 0, stream, eh, "sgl_spmm_axpb_clamp_f32");
}
