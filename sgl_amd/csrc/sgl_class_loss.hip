// K14: the loss of the node-classification task, its gradient and the predicted class in ONE pass over the logits -- what
//   loss = loss_fn(out, y); pred = out.max(1)[1]; loss.backward()
// (train / mini_batch_train / accuracy, sgl/tasks/utils.py:12-98, with nn.CrossEntropyLoss) computes with a log-softmax forward, the NLL
// gather, an arg-max, the NLL backward and the log-softmax backward: about eight passes over [B, C] and two [B, C] temporaries.
// With m_i = max_j z_ij, s_i = sum_j exp(z_ij - m_i), lse_i = m_i + log s_i, and row i LIVE iff 0 <= y_i < c:
//   l_i    = lse_i - z_{i, y_i}                                   (0 for a row that is not live)
//   dZ_ij  = w (exp(z_ij - m_i) / s_i - [j = y_i])                (0 for a row that is not live)
//   pred_i = the lowest index of the row's maximum; a NaN counts as the maximum and the first NaN wins (torch's CPU max)
// pred does not depend on the label; when it is the only output no exp is evaluated and the labels are not read.
//
// Layout: LPR lanes (sgl::slice_instance, sgl_core.cpp) own a row and keep their slice of it in registers, CH vectors of VEC floats,
// lane l of the group holds columns (c * LPR + l) * VEC ..; 64 / LPR consecutive rows per wavefront, so a wavefront reads one
// contiguous piece of the matrix, and U such pieces per step (rows_per_group), all loaded before the first is reduced.  The maximum
// is taken first (group_max), the exponentials replace the logits in the registers, their sum is group_sum; lane 0 of the group finishes the row's loss (one logf, z_{i, y_i} re-read from the line the group just loaded).
// Rows wider than the register layouts (c > 1024): one row per wavefront, a running maximum with a rescaled sum per lane in a first
// read, the gradient from a second read that the caches serve.
//
// Order of the sums: per lane chunk after chunk, element after element, then group_sum<LPR>: it depends on (c, LPR, VEC) alone, not on
// n or the row's position.  No atomics, no scratch, no LDS: two runs are bit-equal, and so is every subset of the outputs.  expf, logf and the division
// are the accurate ones (build.py: no fast-math, correctly rounded division).  An entry of -inf is a class of probability 0; a NaN
// or +inf in a row (or a row of -inf alone) gives NaN in that row's loss and gradient alone.  Nothing traps.  VEC = 4 needs 16-byte
// aligned bases and pitches that are multiples of 4 floats on Z and dZ; nothing beyond column c of a last row is read, nothing beyond
// column c of any row written.
#include <climits>
#include <cmath>

#include "sgl_rows.h"

namespace {

constexpr int kNoIndex = INT32_MAX;                  // "no candidate" of the index minimum

template <int CTRL>
__device__ __forceinline__ int dpp_xchg_i(int v) {
    return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, false);
}
__device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }

// all-lanes minimum of an index over groups of LPR lanes: the exchanges of group_sum / group_max (sgl_rows.h)
template <int LPR>
__device__ __forceinline__ int group_min_index(int v) {
    v = imin(v, dpp_xchg_i<0xB1>(v));
    v = imin(v, dpp_xchg_i<0x4E>(v));
    v = imin(v, dpp_xchg_i<0x141>(v));
    if constexpr (LPR >= 16) v = imin(v, dpp_xchg_i<0x140>(v));
    if constexpr (LPR >= 32) {
        const auto r = __builtin_amdgcn_permlane16_swap((unsigned)v, (unsigned)v, false, false);
        v = imin((int)r[0], (int)r[1]);
    }
    if constexpr (LPR >= 64) {
        const auto r = __builtin_amdgcn_permlane32_swap((unsigned)v, (unsigned)v, false, false);
        v = imin((int)r[0], (int)r[1]);
    }
    return v;
}

template <int VEC>
__device__ __forceinline__ float elem(const typename Vt<VEC>::type &v, const int e) {
    if constexpr (VEC == 4) return v[e];
    else return v;
}
template <int VEC>
__device__ __forceinline__ void set_elem(typename Vt<VEC>::type &v, const int e, const float x) {
    if constexpr (VEC == 4) v[e] = x;
    else v = x;
}

// A lane's candidates for the row's arg-max, its columns taken in ascending order: the largest entry that is not NaN with the first
// column that holds it, and the first column that holds a NaN
struct Best {
    float top = -INFINITY;
    int at = kNoIndex, nan_at = kNoIndex;
    __device__ __forceinline__ void take(const float x, const int col) {
        if (x != x) {
            if (nan_at == kNoIndex) nan_at = col;
        } else if (at == kNoIndex || x > top) {
            top = x;
            at = col;
        }
    }
};

// the row's arg-max from the lanes' candidates and the row's maximum m (of the entries that are not NaN): the first NaN if there is
// one, else the first column that holds m
template <int LPR>
__device__ __forceinline__ int group_argmax(const Best &b, const float m) {
    const int first_nan = group_min_index<LPR>(b.nan_at);
    const int first_top = group_min_index<LPR>((b.at != kNoIndex && b.top == m) ? b.at : kNoIndex);
    return first_nan != kNoIndex ? first_nan : first_top;
}

// w (e / s - [col = y]); 0 for a row that is not live
__device__ __forceinline__ float grad_of(const float e, const float s, const bool hit, const bool live, const float w) {
    return live ? w * (e / s - (hit ? 1.f : 0.f)) : 0.f;
}

// U rows per lane group and step: their loads are issued before the first reduction waits for one (a wavefront that holds ONE row
// of 47 floats has 188 bytes in flight; at one float per lane the kernel then moves 1.0 TB/s, profiles/class_loss_rows_per_group.log)
template <int LPR, int VEC, int CH, int U>
__global__ __launch_bounds__(256) void class_loss_kernel(const float *__restrict__ z, const int64_t ldz, const int64_t n, const int c,
                                                         const int64_t *__restrict__ labels, const float w, float *__restrict__ dz,
                                                         const int64_t lddz, float *__restrict__ row_loss, int64_t *__restrict__ pred,
                                                         const int64_t n_batches) {
    using V = typename Vt<VEC>::type;
    constexpr int GPB = 256 / LPR;                   // lane groups per workgroup
    const int l = threadIdx.x % LPR;
    const int g = threadIdx.x / LPR;
    const bool want_exp = dz != nullptr || row_loss != nullptr;
    for (int64_t b = blockIdx.x; b < n_batches; b += gridDim.x) {   // (every lane stays in the loop: the group exchanges need whole wavefronts)
        V v[U][CH];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t row = (b * U + u) * GPB + g;   // (batch_row of sgl_rows.h, written out: the helper moved class_loss_kernel<64, 4, 4, 1>)
            const float *p = z + (row < n ? row : 0) * ldz;
#pragma unroll
            for (int k = 0; k < CH; ++k) {
                const int col = (k * LPR + l) * VEC;
                v[u][k] = vzero<VEC>();
                if (row < n && col < c) v[u][k] = edge_load<VEC>(p, col, c, row == n - 1);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t row = (b * U + u) * GPB + g;   // (batch_row of sgl_rows.h, written out: the helper moved class_loss_kernel<64, 4, 4, 1>)
            const bool in = row < n;
            Best best;
#pragma unroll
            for (int k = 0; k < CH; ++k) {
                const int col = (k * LPR + l) * VEC;
#pragma unroll
                for (int e = 0; e < VEC; ++e)
                    if (col + e < c) best.take(elem<VEC>(v[u][k], e), col + e);
            }
            const float m = group_max<LPR>(best.top);
            if (pred) {
                const int at = group_argmax<LPR>(best, m);
                if (in && l == 0) pred[row] = at;
            }
            if (!want_exp) continue;                 // (uniform: the same for every lane of the launch)
            const int64_t label = in ? labels[row] : -1;
            const bool live = label >= 0 && label < c;
            const int y = live ? (int)label : -1;
            float part = 0.f;
#pragma unroll
            for (int k = 0; k < CH; ++k) {
                const int col = (k * LPR + l) * VEC;
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    const float ex = col + e < c ? expf(elem<VEC>(v[u][k], e) - m) : 0.f;
                    set_elem<VEC>(v[u][k], e, ex);
                    part += ex;
                }
            }
            const float s = group_sum<LPR>(part);
            if (in) {
                if (row_loss && l == 0) row_loss[row] = live ? (m + logf(s)) - z[row * ldz + y] : 0.f;
                if (dz) {
                    float *orow = dz + row * lddz;
#pragma unroll
                    for (int k = 0; k < CH; ++k) {
                        const int col = (k * LPR + l) * VEC;
                        if (col < c) {
                            V o;
#pragma unroll
                            for (int e = 0; e < VEC; ++e) set_elem<VEC>(o, e, grad_of(elem<VEC>(v[u][k], e), s, col + e == y, live, w));
                            store_cols<VEC>(orow, col, c, o);
                        }
                    }
                }
            }
        }
    }
}

// rows beyond the register layouts: one row per wavefront.  First read: per lane a running maximum and the sum of exp(z - maximum),
// rescaled whenever the maximum moves, and the arg-max candidates; the lanes' sums are brought to the row's maximum and added
// (group_sum<64>).  Second read (the caches serve it): the gradient.  What the register kernels get from the arithmetic itself is
// said outright here: a NaN or +inf in the row, or a row of -inf alone, makes the sum NaN.
template <int VEC>
__global__ __launch_bounds__(256) void class_loss_stream_kernel(const float *__restrict__ z, const int64_t ldz, const int64_t n, const int c,
                                                                const int64_t *__restrict__ labels, const float w, float *__restrict__ dz,
                                                                const int64_t lddz, float *__restrict__ row_loss,
                                                                int64_t *__restrict__ pred) {
    using V = typename Vt<VEC>::type;
    const int l = threadIdx.x % 64;
    const bool want_exp = dz != nullptr || row_loss != nullptr;
    for (int64_t row = (int64_t)blockIdx.x * 4 + threadIdx.x / 64; row < n; row += (int64_t)gridDim.x * 4) {
        const float *p = z + row * ldz;
        const bool last = row == n - 1;
        Best best;
        float part = 0.f;                            // sum of exp(z - best.top) over this lane's columns so far
        bool bad = false;                            // a NaN or +inf among them
        for (int col = l * VEC; col < c; col += 64 * VEC) {
            const V v = edge_load<VEC>(p, col, c, last);
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                if (col + e >= c) continue;
                const float x = elem<VEC>(v, e);
                if (want_exp && x == x) {
                    if (best.at == kNoIndex || x > best.top) part = x == -INFINITY ? 0.f : part * expf(best.top - x) + 1.f;
                    else if (x != -INFINITY) part += expf(x - best.top);
                }
                bad = bad || x != x || x == INFINITY;
                best.take(x, col + e);
            }
        }
        const float m = group_max<64>(best.top);
        if (pred) {
            const int at = group_argmax<64>(best, m);
            if (l == 0) pred[row] = at;
        }
        if (!want_exp) continue;
        const int64_t label = labels[row];
        const bool live = label >= 0 && label < c;
        const int y = live ? (int)label : -1;
        float s = group_sum<64>(best.top == -INFINITY ? 0.f : part * expf(best.top - m));
        if (group_max<64>(bad ? 1.f : 0.f) > 0.f || m == -INFINITY) s = NAN;
        if (row_loss && l == 0) row_loss[row] = live ? (m + logf(s)) - p[y] : 0.f;
        if (dz) {
            float *orow = dz + row * lddz;
            for (int col = l * VEC; col < c; col += 64 * VEC) {
                const V v = edge_load<VEC>(p, col, c, last);
                V o;
#pragma unroll
                for (int e = 0; e < VEC; ++e) set_elem<VEC>(o, e, grad_of(expf(elem<VEC>(v, e) - m), s, col + e == y, live, w));
                store_cols<VEC>(orow, col, c, o);
            }
        }
    }
}

constexpr int64_t kMaxBlocks = (int64_t)1 << 20;     // one step per workgroup up to here (sgl_rows.h stream_grid: strided launches stream slower); strided beyond

// rows per lane group and step: as many as keep the row slices within 16 registers, at most 8 (VEC * CH registers per row)
constexpr int rows_per_group(int vec, int ch) { return vec * ch >= 16 ? 1 : (16 / (vec * ch) > 8 ? 8 : 16 / (vec * ch)); }

template <int LPR, int VEC, int CH>
void launch_rows(hipStream_t st, const float *d_z, int64_t ldz, int64_t n, int c, const int64_t *d_labels, float w, float *d_dz, int64_t lddz,
                 float *d_row_loss, int64_t *d_pred) {
    constexpr int U = rows_per_group(VEC, CH);
    const sgl::BatchGrid grid = sgl::loss_batch_grid(n, 256 / LPR, U, kMaxBlocks);
    hipLaunchKernelGGL((class_loss_kernel<LPR, VEC, CH, U>), dim3((unsigned)grid.blocks), dim3(256), 0, st, d_z, ldz, n, c, d_labels, w, d_dz,
                       lddz, d_row_loss, d_pred, grid.n_batches);
}

}  // namespace

SGL_EXPORT int sgl_class_loss_grad_f32(const float *d_z, int64_t ldz, int64_t n, int64_t c, const int64_t *d_labels, float w, float *d_dz,
                                       int64_t lddz, float *d_row_loss, int64_t *d_pred, void *stream) {
    const char *who = "sgl_class_loss_grad_f32";
    SGL_REQUIRE(n >= 0 && c >= 1 && c <= ((int64_t)1 << 30), "%s: bad sizes (n >= 0, 1 <= c <= 2^30)", who);
    // (a matrix without rows has no storage, no labels, no losses and no predictions: such a pointer is never used)
    SGL_REQUIRE(d_dz || d_row_loss || d_pred || n == 0, "%s: at least one of d_dz, d_row_loss and d_pred is needed", who);
    SGL_REQUIRE(d_z || n == 0, "%s: NULL arguments", who);
    SGL_REQUIRE(d_labels || n == 0 || !(d_dz || d_row_loss), "%s: d_labels may be NULL only when d_pred is the only output", who);
    SGL_REQUIRE(ldz >= c && (lddz >= c || !d_dz), "%s: row pitch smaller than c", who);
    SGL_REQUIRE(aligned_to(d_z, 4) && aligned_to(d_dz, 4) && aligned_to(d_row_loss, 4) && aligned_to(d_labels, 8) && aligned_to(d_pred, 8),
                "%s: pointers must be aligned to their element size", who);
    if (n == 0) return SGL_OK;
    hipStream_t st = sgl::as_stream(stream);
    const bool vec4 = ldz % 4 == 0 && aligned_to(d_z, 16) && (!d_dz || (lddz % 4 == 0 && aligned_to(d_dz, 16)));
    const int vec = vec4 ? 4 : 1;
    const sgl::SliceInstance in = sgl::slice_instance(c, vec, sgl::ClassLossSlices::chunks(vec));
    const int ci = (int)c;
    const bool launched = with_slice_instance<sgl::ClassLossSlices>(
        in, vec4, [&](auto L, auto V, auto C) { launch_rows<L, V, C>(st, d_z, ldz, n, ci, d_labels, w, d_dz, lddz, d_row_loss, d_pred); });
    if (!launched) {
        if (in.ch != 0) return sgl::fail(SGL_ERR_UNSUPPORTED, "%s: no kernel instance is compiled for %d lanes x %d chunks", who, in.lpr, in.ch);
        const int64_t blocks = sgl::loss_grid((n + 3) / 4, kMaxBlocks);
        with_vec(vec4, [&](auto V) {
            hipLaunchKernelGGL((class_loss_stream_kernel<V>), dim3((unsigned)blocks), dim3(256), 0, st, d_z, ldz, n, ci, d_labels, w, d_dz, lddz,
                               d_row_loss, d_pred);
        });
    }
    SGL_LAUNCH_CHECK(who);
    return SGL_OK;
}
