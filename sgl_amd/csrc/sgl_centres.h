// Device helpers shared by the kernels that hold rows of X in registers against centres staged in LDS: sgl_kmeans.hip (K9, the
// assignment step) and sgl_cluster_loss.hip (K12, the clustering loss and its gradient).  A lane's sum of squared differences in the
// DIRECT form (Sq), and the staging of a tile of NEGATED centres (stage_centres, restage_centres);
// the lane sums (group_sum), the row loads that never read beyond column d of a last row (edge_load) and the column
// helpers (vzero, store_cols, load_cols) are sgl_rows.h's.  Not part of the ABI.
#pragma once
#include "sgl_rows.h"

namespace {

using f2 = float __attribute__((ext_vector_type(2)));

template <int VEC>
struct Sq;                                           // a lane's partial sum of squared differences
template <>
struct Sq<4> {
    f2 a = {0.f, 0.f};
    __device__ __forceinline__ void add(const f4 x, const f4 c) {
        const f2 lo = x.lo - c.lo, hi = x.hi - c.hi;
        a = __builtin_elementwise_fma(lo, lo, a);
        a = __builtin_elementwise_fma(hi, hi, a);
    }
    // the same with the centre NEGATED: x + (-c) is x - c bit for bit, and of the two only the packed add is selected as one
    // instruction (the subtraction of two float2 compiles to two scalar subtractions and two moves that pair their results again)
    __device__ __forceinline__ void add_negated(const f4 x, const f4 nc) {
        const f2 lo = x.lo + nc.lo, hi = x.hi + nc.hi;
        a = __builtin_elementwise_fma(lo, lo, a);
        a = __builtin_elementwise_fma(hi, hi, a);
    }
    __device__ __forceinline__ void merge(const Sq &o) { a += o.a; }
    __device__ __forceinline__ float total() const { return a[0] + a[1]; }
};
template <>
struct Sq<1> {
    float a = 0.f;
    __device__ __forceinline__ void add(const float x, const float c) {
        const float t = x - c;
        a = fmaf(t, t, a);
    }
    __device__ __forceinline__ void add_negated(const float x, const float nc) {
        const float t = x + nc;
        a = fmaf(t, t, a);
    }
    __device__ __forceinline__ void merge(const Sq &o) { a += o.a; }
    __device__ __forceinline__ float total() const { return a; }
};

// The streaming kernels (rows beyond the register layouts) sum a lane's chunks in blocks of kStreamBlock: each block from zero, the
// blocks added in order (Sq::merge).  One running sum per lane over the 4 096 chunks of a row of 10^6 columns loses the low bits of
// every term added to a sum that is already large -- measured at d = 1 048 580 on the k-means test rows, whose columns 0 .. 7 (the
// FIRST chunk of lanes 0 and 1) carry four fifths of the energy: 1.3e-5 of the squared distance, biased low, 4.5e-6 of dX, against
// 5e-7 / 3.6e-7 for numpy's pairwise float32 sum; in blocks 2.4e-7 (restated on the CPU: tests/test_wide_cpu.py).  A row of at most
// kStreamBlock chunks per lane (16 384 columns in 16-byte lanes, 4 096 in 4-byte lanes) is one block, and 0 + s = s: its bits are
// what they were.
constexpr int kStreamBlock = 64;

constexpr int kTileFloats = 16384;                   // 64 KiB of centres per tile

// centres j0 .. j0 + kt - 1, NEGATED (Sq::add_negated), into the tile (pitch dp = d rounded up to VEC), pad zeroed: one wavefront
// per centre row
template <int VEC>
__device__ __forceinline__ void stage_centres(float *__restrict__ tile, const float *__restrict__ cen, const int64_t ldc, const int k,
                                              const int j0, const int kt, const int d, const int dp) {
    using V = typename Vt<VEC>::type;
    const int lane = threadIdx.x % 64;
    for (int jj = threadIdx.x / 64; jj < kt; jj += 4) {
        const float *crow = cen + (int64_t)(j0 + jj) * ldc;
        const bool last = j0 + jj == k - 1;
        for (int col = lane * VEC; col < dp; col += 64 * VEC)
            *reinterpret_cast<V *>(tile + jj * dp + col) = -edge_load<VEC>(crow, col, d, last);
    }
}
// the same between the barriers that the tile's readers need; a tile that holds every centre (tile_k >= k) is staged once per
// workgroup (`staged`), not once per batch
template <int VEC>
__device__ __forceinline__ void restage_centres(bool &staged, float *__restrict__ tile, const float *__restrict__ cen, const int64_t ldc,
                                                const int k, const int j0, const int kt, const int tile_k, const int d, const int dp) {
    if (!(staged && tile_k >= k)) {
        __syncthreads();                             // the tile's last readers are done
        stage_centres<VEC>(tile, cen, ldc, k, j0, kt, d, dp);
        __syncthreads();
        staged = true;
    }
}

}  // namespace
