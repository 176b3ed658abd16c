// What the fp32 SpMM (sgl_spmm.hip) and the bfloat16 SpMM (sgl_spmm_bf16.hip) share: the in-wavefront helpers of a work item, the
// running-aggregate arithmetic, and the host side of a launch -- lane layout (sgl::spmm_layout, sgl_core.cpp), grid, split-row
// workspace -- so that both kernels follow one rule on one handle and plan.  The row walks (run_rows) differ on purpose, in their
// element type and their remainder handling, and stay in their files.  Not part of the ABI.
#pragma once
#include "sgl_csr.h"

namespace {

// broadcast element `idx` (0..63) of a wave-distributed register to this lane
template <int R>
__device__ __forceinline__ int bcast_i(int v, int idx) {
    if constexpr (R == 1)
        return __builtin_amdgcn_readlane(v, idx);  // idx is wave-uniform -> SGPR result
    else
        return __builtin_amdgcn_ds_bpermute(idx << 2, v);
}
template <int R>
__device__ __forceinline__ float bcast_f(float v, int idx) {
    return __int_as_float(bcast_i<R>(__float_as_int(v), idx));
}

// running aggregate over hops, updated where the row is produced (Sum / Mean / SimpleWeighted MessageOps without a
// second pass over the hop matrices): acc_mode 1: ACC += Y, 2: ACC += w * Y (rounded product, then add: the order of
// hop_reduce_kernel), 3: ACC = max(ACC, Y) (+8: min), +4: ACC /= acc_div afterwards (Mean's one true division, on the
// last hop).  Y itself is stored unchanged: it is the next hop's input.
__device__ __forceinline__ float acc_apply(float a, float y, int mode, float w, float div) {
    if ((mode & 3) == 3)   // running extremum with torch's NaN rule (a NaN in any hop wins), +8: min instead of max
        return (mode & 8) ? ((y < a || y != y) ? y : a) : ((y > a || y != y) ? y : a);
    a = ((mode & 3) == 2) ? __fadd_rn(a, __fmul_rn(y, w)) : __fadd_rn(a, y);
    if (mode & 4) a = __fdiv_rn(a, div);
    return a;
}

// Row map (sgl_csr_set_rowmap): the CSR's rows are stored in PROCESSING order (a locality ordering found at plan time), row i
// of the storage is row my_map[i] of the product.  Only the output side is indirect -- Y, the residual and the running
// aggregate are addressed with the mapped index from un-offset base pointers; the gathers use the original column ids, and a
// row's terms are added in their original order, so the result is bit-identical to the unpermuted matrix's.
struct RowMap {
    int my_map = 0;      // lane i: output row of the item's row i
    bool on = false;
};

// Block -> work, part of both kernels' arguments: the first piece_blocks blocks take the long-row pieces, the others the items, one
// per wavefront (block * waves + wave).  The hardware deals blocks to the 8 XCDs round-robin; under the remap item block ib takes
// the place xcd_block(ib), so that XCD x walks the x-th contiguous range of the item list.
struct BlockMap {
    int32_t piece_blocks, item_blocks_per_xcd, xcd_remap, waves;
};
__device__ __forceinline__ int xcd_block(int ib, int item_blocks_per_xcd) { return (ib & 7) * item_blocks_per_xcd + (ib >> 3); }

// The row-pointer window of a work item of `nrows` rows from `row_begin`: lane i of `my_rel` holds the offset of row i's first
// non-zero relative to `base`, the item's first non-zero (lane nrows holds tot, the item's number of non-zeros).
struct ItemWindow {
    int64_t base;
    int my_rel, tot;
};

__device__ __forceinline__ ItemWindow item_window(const int64_t *rowptr, int row_begin, int nrows, int lane) {
    ItemWindow w;
    const int64_t rp = rowptr[(int64_t)row_begin + min(lane, nrows)];
    const int lo = __builtin_amdgcn_readfirstlane((int)(uint32_t)rp);
    const int hi = __builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)rp >> 32));
    w.base = (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
    w.my_rel = (int)(rp - w.base);
    w.tot = __builtin_amdgcn_readlane(w.my_rel, nrows);
    return w;
}

__device__ __forceinline__ RowMap item_rowmap(const int32_t *rowmap, int row_begin, int nrows, int lane) {
    RowMap rm;
    rm.on = rowmap != nullptr;            // then the output-side pointers stay un-offset: rows are addressed through the map
    rm.my_map = rm.on ? rowmap[(int64_t)row_begin + max(min(lane, nrows - 1), 0)] : 0;
    return rm;
}

// ---- host -----------------------------------------------------------------------------------------------------------------
struct SpmmLaunch : sgl::SpmmLayout {
    BlockMap map;
    int64_t ldp;              // floats per row of the split-row workspace
    int grid, fixup_grid;     // blocks of the kernel (0: nothing to do) and of the fix-up pass (0: no split rows)
};

// everything about a launch of one column slice (d columns in `lanes` lanes per row) that does not depend on the element type
int spmm_launch(SpmmLaunch &L, const sgl_csr_t *h, int lanes, int d, bool bf16, const char *who) {
    static_cast<sgl::SpmmLayout &>(L) = sgl::spmm_layout(lanes, (h->flags & SGL_CSR_STRICT_ORDER) != 0, h->nnz, h->n_rows, bf16);
    L.ldp = bf16 ? (d + 7) / 8 * 8 : (d + 3) / 4 * 4;   // whole lane accesses: a lane stores up to 4 (bf16: 8) partial sums at once
    L.map.waves = L.waves;
    L.map.piece_blocks = (int32_t)((h->n_pieces + L.waves - 1) / L.waves);
    const int64_t item_blocks = (h->n_items + L.waves - 1) / L.waves;
    L.map.xcd_remap = (!(h->flags & SGL_CSR_NO_XCD_REMAP) && sgl::tuning("spmm_xcd_remap", 1) != 0) ? 1 : 0;
    L.map.item_blocks_per_xcd = (int32_t)((item_blocks + 7) / 8);
    const int64_t grid64 = L.map.piece_blocks + (L.map.xcd_remap ? (int64_t)L.map.item_blocks_per_xcd * 8 : item_blocks);
    if (grid64 >= INT32_MAX) return sgl::fail(SGL_ERR_UNSUPPORTED, "%s: grid too large", who);
    const int64_t fg = (int64_t)((d + 255) / 256) * h->n_long;
    if (fg >= INT32_MAX) return sgl::fail(SGL_ERR_UNSUPPORTED, "%s: fix-up grid too large", who);
    L.grid = (int)grid64;
    L.fixup_grid = (int)fg;
    return SGL_OK;
}

// The handle's one split-row workspace (fp32 partial sums, shared by both kernels) holds at least n_pieces rows of ldp floats.
int grow_partial(sgl_csr_t *h, int64_t ldp) {
    const size_t need = (size_t)h->n_pieces * (size_t)ldp;
    if (need > h->partial_cap) {
        // grow-only, and the outgrown buffer is kept until the handle dies: a ChainGraph captured earlier has its
        // address baked in and may be replayed after a wider eager call on the same handle
        if (h->d_partial) h->retired.push_back(h->d_partial);
        h->d_partial = nullptr;
        h->partial_cap = 0;
        SGL_HIP_CHECK(hipMalloc((void **)&h->d_partial, need * sizeof(float)));
        h->partial_cap = need;
    }
    return SGL_OK;
}

// the arguments of sgl_spmm_acc_f32 / sgl_spmm_acc_bf16 checked, and the mode as acc_apply takes it
int acc_mode_of(const char *who, const float *d_acc, int mode, float divisor, int &acc_mode) {
    SGL_REQUIRE(d_acc != nullptr, "%s: NULL accumulator", who);
    SGL_REQUIRE(!(divisor == 0.f), "%s: zero divisor", who);
    SGL_REQUIRE(mode >= SGL_ACC_SUM && mode <= SGL_ACC_MIN, "%s: unknown mode %d", who, mode);
    SGL_REQUIRE(mode < SGL_ACC_MAX || divisor == 1.f, "%s: max / min take no divisor", who);
    acc_mode = mode >= SGL_ACC_MAX ? (3 | (mode == SGL_ACC_MIN ? 8 : 0)) : ((mode == SGL_ACC_WSUM ? 2 : 1) | (divisor != 1.f ? 4 : 0));
    return SGL_OK;
}

}  // namespace
