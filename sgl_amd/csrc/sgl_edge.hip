// K8: scores of an edge list, out[e] = <A[u_e, :], B[v_e, :]> -- the two lines that end the reference's link-prediction pipelines,
//   sim = torch.mm(Z, Z.t()); sim[e0, e1]     (sgl/tasks/link_prediction.py:282-283, sgl/tasks/utils.py:266 and 281-285)
// without the N x N matrix: per edge one 16-byte index load, two row gathers and a dot product.  Memory-bound and gather-shaped
// like the SpMM and the row gathers: E x (2 d x 4 + 16 + 4) bytes, no reuse the kernel could arrange (what reuse there is -- a node
// with many edges -- is the caches').
//
// Layout.  LPR lanes (8 / 16 / 32 / 64: sgl::pick_lpr) own one edge, 256 / LPR edge groups per workgroup, U edges per group:
// a group first loads its U index pairs, then for every chunk of LPR vectors issues the 2 U row loads before any arithmetic (the
// U-unroll of gather_rows_kernel: 2 U independent 16-byte loads per lane in flight), accumulates per lane with fmaf, elements 0..3
// of a vector in order, chunk after chunk, and finally sums the group's lanes with group_sum<LPR> (DPP / permlane: no LDS).
// The summation order therefore depends on (d, LPR, VEC) alone: not on E, not on where the edge stands in the list, and -- fmaf(a, b, c)
// == fmaf(b, a, c) -- not on which of the two rows is u.
//
// VEC = 4 needs 16-byte aligned bases and pitches that are multiples of 4 floats; the vector that straddles column d then lies inside
// the row's own pitch, and its elements >= d are zeroed BEFORE the product (the pad may hold NaN).  The last row of a matrix is the one
// row whose pitch the storage need not hold: its straddling vector is read element by element, nothing beyond column d.  VEC = 1 (one
// float per lane) takes everything else: column views at odd offsets, pitches that are no multiple of 4.
//
// Indices: negative ones count from the end; one outside [-n, n) makes THAT edge's output NaN (the rule of sgl_gather_rows_bf16_f32:
// device index tensors are not validated on the host, and a score kernel that aborts the process for one bad pair would take the
// caller's whole sweep with it).  The kernel never traps and reads row 0 in place of a bad row (n > 0 is checked on the host).
#include "sgl_rows.h"

namespace {

using i64x2 = long __attribute__((ext_vector_type(2)));
static_assert(sizeof(i64x2) == 16, "an edge is two int64");

template <int LPR, int VEC, int U>
__global__ __launch_bounds__(256) void edge_dot_kernel(const float *__restrict__ a, const int64_t lda, const int64_t n_a,
                                                       const float *__restrict__ b, const int64_t ldb, const int64_t n_b,
                                                       const int64_t *__restrict__ edges, const int edges16, const int64_t n_edges,
                                                       const int d, float *__restrict__ out) {
    using V = typename Vt<VEC>::type;
    constexpr int GPB = 256 / LPR;                   // edge groups per workgroup
    const int l = threadIdx.x % LPR;
    const int64_t e0 = (int64_t)blockIdx.x * (GPB * U) + threadIdx.x / LPR;
    const float *pa[U], *pb[U];
    bool la[U], lb[U], bad[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int64_t e = e0 + (int64_t)u * GPB;
        int64_t s = 0, t = 0;
        if (e < n_edges) {
            if (edges16) {
                const i64x2 p = *reinterpret_cast<const i64x2 *>(edges + 2 * e);
                s = p[0];
                t = p[1];
            } else {                                 // an edge list that starts on an odd multiple of 8 bytes
                s = edges[2 * e];
                t = edges[2 * e + 1];
            }
        }
        if (s < 0) s += n_a;                         // python-style negative index
        if (t < 0) t += n_b;
        bad[u] = s < 0 || s >= n_a || t < 0 || t >= n_b;
        if (bad[u]) s = t = 0;                       // a readable row; the result is replaced below
        pa[u] = a + s * lda;
        pb[u] = b + t * ldb;
        la[u] = s == n_a - 1;
        lb[u] = t == n_b - 1;
    }
    float acc[U];
#pragma unroll
    for (int u = 0; u < U; ++u) acc[u] = 0.f;
    for (int c = l * VEC; c < d; c += LPR * VEC) {
        V x[U], y[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            x[u] = edge_load<VEC>(pa[u], c, d, la[u]);
            y[u] = edge_load<VEC>(pb[u], c, d, lb[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if constexpr (VEC == 4) {
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[u] = fmaf(x[u][e], y[u][e], acc[u]);
            } else {
                acc[u] = fmaf(x[u], y[u], acc[u]);
            }
        }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const float s = group_sum<LPR>(acc[u]);
        const int64_t e = e0 + (int64_t)u * GPB;
        if (l == 0 && e < n_edges) out[e] = bad[u] ? __uint_as_float(0x7fc00000u) : s;
    }
}

// a matrix without rows: every index is out of range, every output NaN
__global__ __launch_bounds__(256) void edge_fill_kernel(float *__restrict__ out, const int64_t n, const float v) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) out[i] = v;
}

constexpr int kEdgesPerGroup = 4;                    // U: 8 row vectors per lane in flight, 62 VGPRs (8 wavefronts per SIMD), no scratch

}  // namespace

SGL_EXPORT int sgl_edge_dot_f32(const float *d_a, int64_t lda, int64_t n_a, const float *d_b, int64_t ldb, int64_t n_b,
                                const int64_t *d_edges, int64_t n_edges, int64_t d, float *d_out, void *stream) {
    SGL_REQUIRE(n_edges >= 0 && d >= 0 && d < INT32_MAX && n_a >= 0 && n_b >= 0, "sgl_edge_dot_f32: bad sizes");
    SGL_REQUIRE_WIDTH("sgl_edge_dot_f32", "d", d);
    // (a matrix without rows or without columns has no storage: its pointer is never used)
    SGL_REQUIRE((d_a || n_a == 0 || d == 0) && (d_b || n_b == 0 || d == 0) && d_edges && d_out, "sgl_edge_dot_f32: NULL arguments");
    SGL_REQUIRE(lda >= d && ldb >= d, "sgl_edge_dot_f32: row pitch smaller than d");
    SGL_REQUIRE(aligned_to(d_a, 4) && aligned_to(d_b, 4) && aligned_to(d_out, 4) && aligned_to(d_edges, 8),
                "sgl_edge_dot_f32: pointers must be aligned to their element size");
    if (n_edges == 0) return SGL_OK;
    hipStream_t st = sgl::as_stream(stream);
    if (d == 0) {                                    // empty sums: zeros, whatever the indices are; no kernel
        SGL_HIP_CHECK(hipMemsetAsync(d_out, 0, (size_t)n_edges * sizeof(float), st));
        return SGL_OK;
    }
    if (n_a == 0 || n_b == 0) {
        const int64_t blocks = n_edges < 256 * 1024 ? (n_edges + 255) / 256 : 1024;
        hipLaunchKernelGGL(edge_fill_kernel, dim3((unsigned)blocks), dim3(256), 0, st, d_out, n_edges, __builtin_nanf(""));
        SGL_LAUNCH_CHECK("sgl_edge_dot_f32");
        return SGL_OK;
    }
    const bool vec4 = lda % 4 == 0 && ldb % 4 == 0 && aligned_to(d_a, 16) && aligned_to(d_b, 16);
    const int lpr = sgl::pick_lpr(d, vec4 ? 4 : 1);
    const int64_t per_block = (int64_t)(256 / lpr) * kEdgesPerGroup;
    const int64_t blocks = (n_edges + per_block - 1) / per_block;
    if (!sgl::launch_fits(blocks, 256)) return sgl::fail(SGL_ERR_UNSUPPORTED, "sgl_edge_dot_f32: too many edges for one launch (split the list)");
    const int e16 = aligned_to(d_edges, 16) ? 1 : 0;
    with_lpr_vec(lpr, vec4, [&](auto L, auto V) {
        hipLaunchKernelGGL((edge_dot_kernel<L, V, kEdgesPerGroup>), dim3((unsigned)blocks), dim3(256), 0, st, d_a, lda, n_a, d_b, ldb, n_b, d_edges,
                           e16, n_edges, (int)d, d_out);
    });
    SGL_LAUNCH_CHECK("sgl_edge_dot_f32");
    return SGL_OK;
}
