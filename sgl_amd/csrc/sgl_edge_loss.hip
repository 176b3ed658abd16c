// K11: one training step of link prediction on an edge list -- loss, per-edge coefficient and dZ in ONE pass over a prepared list:
//   sim = torch.mm(Z, Z.t()); pred = sigmoid(sim[e0, e1]); loss = loss_fn(pred, labels); loss.backward()
// (sgl/tasks/utils.py:280-295, edge_predict_train; default loss_fn F.binary_cross_entropy_with_logits, sgl/tasks/link_prediction.py:15)
// without the N x N matrix and without a per-step sort: the edges are grouped by endpoint ONCE (the incidence CSR of
// tricks/link_prediction.py: EdgePlan), and while row i is in registers every incident edge (i, j) gathers z_j once, forms the score,
// turns it into the loss coefficient c and accumulates c z_j into dZ[i].  2 E row gathers for loss and gradient together.
//
// Layout.  LPR lanes (sgl::slice_instance) own one PIECE: at most max_piece consecutive incidences of one row.  A lane keeps its slice of z_i
// and of the piece's dZ sum in registers, CH vectors of VEC floats each (vector (c LPR + l) of the row for lane l, chunk c: K9's
// layout); CH = 0 is the instance for rows beyond the register layouts, which re-reads z_i per chunk and keeps the sum in the output
// row it owns.  The piece's entries are walked U at a time: per chunk the U row loads are issued before any arithmetic (K8's unroll).
//
// Score.  s = <z_i, z_j> in exactly edge_dot_kernel's order for the same (d, LPR, VEC): per lane fmaf over the elements of a vector,
// chunk after chunk, then group_sum<LPR>.  fmaf(a, b, c) == fmaf(b, a, c), so the score has the same bits seen from u's row and from
// v's row, and they are the bits of sgl_edge_dot_f32.
//
// Coefficient (w: one scalar, 1 / E for the mean).
//   SIGMOID_LOGITS  the reference as written -- torch.sigmoid and THEN binary_cross_entropy_with_logits:
//                   p = sigma(s), L = (1 - y) p + log1p(exp(-p)), c = w (sigma(p) - y) p (1 - p)
//   LOGITS          L = max(s, 0) - s y + log1p(exp(-|s|)), c = w (sigma(s) - y)
//   GIVEN           c = given[e]: no dot product, no loss (the backward of edge scores under any loss)
// sigma(s) and p (1 - p) = sigma(s) sigma(-s) are formed from e = exp(-|s|): finite, and without cancellation, for every finite s.
//
// Sums.  dZ of a piece: acc = fmaf(c, z_j, acc) in entry order.  A row that is one piece writes dZ[row], pieces of a cut row write rows
// of the partial buffer, which edge_fold_kernel adds in piece order.  piece_loss[p] = the float32 sum of L over the piece's PRIMARY
// entries (code >= 0: this row is u_e) in entry order.  No atomics anywhere: two runs are bit-equal.  Every row has at least one piece
// (a node without incidences an empty one), so dZ is overwritten whole -- exact zeros there, whatever the buffer held.
//
// Indices are the plan's: validated and wrapped when it was built.  The kernel has no bad-index path.
#include "sgl_rows.h"

namespace {

enum { MODE_SIGMOID_LOGITS = 0, MODE_LOGITS = 1, MODE_GIVEN = 2 };

constexpr int kEntriesPerStep = 4;                   // U, as in edge_dot_kernel (and <= 8, the smallest lane group: one entry per lane below)

using i64x4 = long __attribute__((ext_vector_type(4)));

template <int MODE>
__device__ __forceinline__ void loss_coef(const float s, const float y, const float w, float &loss, float &c) {
    const float e = expf(-fabsf(s));                 // in (0, 1]
    const float r = 1.f / (1.f + e);
    const float sig = s >= 0.f ? r : e * r;          // sigma(s)
    if constexpr (MODE == MODE_SIGMOID_LOGITS) {
        const float ep = expf(-sig);                 // sig in [0, 1]
        loss = (1.f - y) * sig + log1pf(ep);
        c = w * (1.f / (1.f + ep) - y) * (e * r * r);
    } else {
        loss = fmaxf(s, 0.f) - s * y + log1pf(e);
        c = w * (s >= 0.f ? (1.f - y) - e * r : sig - y);   // sigma(s) - y; for s >= 0 as (1 - y) - sigma(-s): no cancellation at y = 1
    }
}

template <int VEC>
__device__ __forceinline__ float dot_step(const typename Vt<VEC>::type x, const typename Vt<VEC>::type y, float acc) {
    if constexpr (VEC == 4) {
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = fmaf(x[e], y[e], acc);
        return acc;
    } else {
        return fmaf(x, y, acc);
    }
}

template <int VEC>
__device__ __forceinline__ typename Vt<VEC>::type axpy_step(const float c, const typename Vt<VEC>::type y, typename Vt<VEC>::type acc) {
    if constexpr (VEC == 4) {
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = fmaf(c, y[e], acc[e]);
        return acc;
    } else {
        return fmaf(c, y, acc);
    }
}

template <int LPR, int VEC, int MODE, int CH>
__global__ __launch_bounds__(256) void edge_loss_grad_kernel(const float *__restrict__ z, const int64_t ldz, const int64_t n, const int d,
                                                             const int64_t *__restrict__ pieces, const int64_t n_pieces,
                                                             const int32_t *__restrict__ inc_other, const int64_t *__restrict__ inc_edge,
                                                             const float *__restrict__ labels, const float *__restrict__ given,
                                                             const float w, float *dz, const int64_t lddz, float *partial,
                                                             const int64_t ldp, const int ovec, float *__restrict__ score,
                                                             float *__restrict__ coef, float *__restrict__ piece_loss) {
    using V = typename Vt<VEC>::type;
    constexpr int GPB = 256 / LPR;                   // pieces per workgroup
    constexpr int U = kEntriesPerStep;
    constexpr int NCH = CH > 0 ? CH : 1;
    const int l = threadIdx.x % LPR;
    const int64_t p = (int64_t)blockIdx.x * GPB + threadIdx.x / LPR;
    const bool live = p < n_pieces;                  // a whole lane group is live or not; nobody returns before the last group_sum
    int64_t row = 0, begin = 0, end = 0, dest = -1;
    if (live) {
        const i64x4 t = *reinterpret_cast<const i64x4 *>(pieces + 4 * p);
        row = t[0];
        begin = t[1];
        end = t[2];
        dest = t[3];
    }
    const float *zi = z + row * ldz;
    const bool last_i = row == n - 1;
    float *orow = dest < 0 ? dz + row * lddz : partial + dest * ldp;

    V xi[NCH], acc[NCH];
    if constexpr (CH > 0) {
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const int col = (c * LPR + l) * VEC;
            xi[c] = (MODE != MODE_GIVEN && live && col < d) ? edge_load<VEC>(zi, col, d, last_i) : vzero<VEC>();
            acc[c] = vzero<VEC>();
        }
    } else {
        if (live)
            for (int col = l * VEC; col < d; col += LPR * VEC) store_cols<VEC>(orow, col, d, vzero<VEC>(), ovec != 0);
    }

    float loss = 0.f;
    for (int64_t k = begin; k < end; k += U) {
        const float *pj[U];
        int64_t edge[U];
        bool lastj[U], ok[U], primary[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            ok[u] = k + u < end;
            const int64_t kk = ok[u] ? k + u : k;    // a slot beyond the piece repeats its first entry and is not used
            const int64_t j = inc_other[kk];
            const int64_t code = inc_edge[kk];
            primary[u] = code >= 0;
            edge[u] = primary[u] ? code : ~code;
            pj[u] = z + j * ldz;
            lastj[u] = j == n - 1;
        }
        float cf[U];
        V y[U];                                      // CH == 1: the other rows stay in registers for the sum
        if constexpr (MODE == MODE_GIVEN) {
#pragma unroll
            for (int u = 0; u < U; ++u) cf[u] = given[edge[u]];
            if constexpr (CH == 1) {
                const int col = l * VEC;
#pragma unroll
                for (int u = 0; u < U; ++u) y[u] = col < d ? edge_load<VEC>(pj[u], col, d, lastj[u]) : vzero<VEC>();
            }
        } else {
            float lab[U], s[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                lab[u] = labels[edge[u]];
                s[u] = 0.f;
            }
            if constexpr (CH > 0) {
#pragma unroll
                for (int c = 0; c < CH; ++c) {
                    const int col = (c * LPR + l) * VEC;
                    if (col < d) {
                        V t[U];
#pragma unroll
                        for (int u = 0; u < U; ++u) t[u] = edge_load<VEC>(pj[u], col, d, lastj[u]);
#pragma unroll
                        for (int u = 0; u < U; ++u) s[u] = dot_step<VEC>(xi[c], t[u], s[u]);
                        if constexpr (CH == 1) {
#pragma unroll
                            for (int u = 0; u < U; ++u) y[u] = t[u];
                        }
                    } else if constexpr (CH == 1) {
#pragma unroll
                        for (int u = 0; u < U; ++u) y[u] = vzero<VEC>();
                    }
                }
            } else {
                for (int col = l * VEC; col < d; col += LPR * VEC) {
                    const V x = edge_load<VEC>(zi, col, d, last_i);
                    V t[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) t[u] = edge_load<VEC>(pj[u], col, d, lastj[u]);
#pragma unroll
                    for (int u = 0; u < U; ++u) s[u] = dot_step<VEC>(x, t[u], s[u]);
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) s[u] = group_sum<LPR>(s[u]);
            // one entry per lane: lane u of the group turns entry u's score into (L, c) -- ONE sequence of exp / log1p / divisions per
            // wavefront instead of U -- and the group reads them back (sgl_rows.h, "one hop per lane"); the arithmetic is the same
            float s_mine = s[0], y_mine = lab[0], le_mine, cf_mine;
#pragma unroll
            for (int u = 1; u < U; ++u)
                if (l == u) {
                    s_mine = s[u];
                    y_mine = lab[u];
                }
            loss_coef<MODE>(s_mine, y_mine, w, le_mine, cf_mine);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                cf[u] = from_lane<LPR>(cf_mine, u);
                const float le = from_lane<LPR>(le_mine, u);
                if (ok[u] && primary[u]) {
                    loss += le;
                    if (l == 0) {
                        if (score) score[edge[u]] = s[u];
                        if (coef) coef[edge[u]] = cf[u];
                    }
                }
            }
        }
        // dZ of the piece, entry after entry
        if constexpr (CH == 1) {
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (ok[u]) acc[0] = axpy_step<VEC>(cf[u], y[u], acc[0]);
        } else if constexpr (CH > 1) {
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                const int col = (c * LPR + l) * VEC;
                if (col < d) {
                    V t[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) t[u] = edge_load<VEC>(pj[u], col, d, lastj[u]);
#pragma unroll
                    for (int u = 0; u < U; ++u)
                        if (ok[u]) acc[c] = axpy_step<VEC>(cf[u], t[u], acc[c]);
                }
            }
        } else {
            for (int col = l * VEC; col < d; col += LPR * VEC) {   // every lane re-reads what it alone wrote
                V t[U];
#pragma unroll
                for (int u = 0; u < U; ++u) t[u] = edge_load<VEC>(pj[u], col, d, lastj[u]);
                V a = load_cols<VEC>(orow, col, d, ovec != 0);
#pragma unroll
                for (int u = 0; u < U; ++u)
                    if (ok[u]) a = axpy_step<VEC>(cf[u], t[u], a);
                store_cols<VEC>(orow, col, d, a, ovec != 0);
            }
        }
    }
    if (live) {
        if constexpr (CH > 0) {
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                const int col = (c * LPR + l) * VEC;
                if (col < d) store_cols<VEC>(orow, col, d, acc[c], ovec != 0);
            }
        }
        if (MODE != MODE_GIVEN && l == 0 && piece_loss) piece_loss[p] = loss;
    }
}

// dZ[row] = the partial rows of a cut row, added in piece order: one wavefront per cut row, one column per lane
__global__ __launch_bounds__(256) void edge_fold_kernel(const int64_t *__restrict__ fold, const int64_t n_fold, const float *__restrict__ partial,
                                                        const int64_t ldp, const int d, float *__restrict__ dz, const int64_t lddz) {
    const int l = threadIdx.x % 64;
    for (int64_t f = (int64_t)blockIdx.x * 4 + threadIdx.x / 64; f < n_fold; f += (int64_t)gridDim.x * 4) {
        const int64_t row = fold[3 * f], first = fold[3 * f + 1], count = fold[3 * f + 2];
        for (int col = l; col < d; col += 64) {
            float a = partial[first * ldp + col];
            for (int64_t q = 1; q < count; ++q) a += partial[(first + q) * ldp + col];
            dz[row * lddz + col] = a;
        }
    }
}

constexpr int kMaxFoldBlocks = 2048;

}  // namespace

SGL_EXPORT int sgl_edge_loss_grad_f32(const float *d_z, int64_t ldz, int64_t n, int64_t d, const int64_t *d_pieces, int64_t n_pieces,
                                      const int32_t *d_inc_other, const int64_t *d_inc_edge, int64_t n_inc, const float *d_labels,
                                      const float *d_given, int64_t n_edges, int mode, float w, float *d_dz, int64_t lddz,
                                      float *d_partial, int64_t ldp, int64_t n_partial, const int64_t *d_fold, int64_t n_fold,
                                      float *d_score, float *d_coef, float *d_piece_loss, void *stream) {
    const char *who = "sgl_edge_loss_grad_f32";
    SGL_REQUIRE(n >= 0 && n < INT32_MAX && d >= 0 && d < INT32_MAX && n_pieces >= 0 && n_inc >= 0 && n_edges >= 0 && n_partial >= 0 && n_fold >= 0,
                "%s: bad sizes", who);
    SGL_REQUIRE_WIDTH(who, "d", d);
    SGL_REQUIRE(n_inc == 2 * n_edges, "%s: the incidence list must hold every edge twice", who);
    SGL_REQUIRE(mode == MODE_SIGMOID_LOGITS || mode == MODE_LOGITS || mode == MODE_GIVEN, "%s: unknown mode %d", who, mode);
    SGL_REQUIRE(d_z || n == 0 || d == 0, "%s: NULL z", who);
    SGL_REQUIRE((d_pieces || n_pieces == 0) && (d_fold || n_fold == 0) && (d_partial || n_partial == 0 || d == 0), "%s: NULL piece tables", who);
    SGL_REQUIRE((d_inc_other && d_inc_edge) || n_inc == 0, "%s: NULL incidence list", who);
    SGL_REQUIRE(d_dz || n == 0 || d == 0, "%s: NULL dz", who);
    SGL_REQUIRE(mode == MODE_GIVEN ? (d_given || n_edges == 0) : (d_labels || n_edges == 0), "%s: NULL %s", who,
                mode == MODE_GIVEN ? "coefficients" : "labels");
    SGL_REQUIRE(mode != MODE_GIVEN || (!d_score && !d_coef && !d_piece_loss), "%s: the GIVEN mode has no score, coefficient or loss output", who);
    SGL_REQUIRE(ldz >= d && lddz >= d && (ldp >= d || n_partial == 0), "%s: row pitch smaller than d", who);
    SGL_REQUIRE(n_fold <= n_partial, "%s: more cut rows than partial rows", who);
    SGL_REQUIRE(aligned_to(d_z, 4) && aligned_to(d_dz, 4) && aligned_to(d_partial, 4) && aligned_to(d_labels, 4) && aligned_to(d_given, 4) &&
                    aligned_to(d_score, 4) && aligned_to(d_coef, 4) && aligned_to(d_piece_loss, 4) && aligned_to(d_inc_other, 4) &&
                    aligned_to(d_inc_edge, 8) && aligned_to(d_fold, 8) && aligned_to(d_pieces, 32),
                "%s: pointers must be aligned to their element size (the piece table to its 32-byte records)", who);
    if (n_pieces == 0 && n_fold == 0) return SGL_OK;
    hipStream_t st = sgl::as_stream(stream);
    if (d == 0) {                                    // rows without columns: nothing to sum, every score is an empty sum; no kernel
        if (d_piece_loss && n_pieces) SGL_HIP_CHECK(hipMemsetAsync(d_piece_loss, 0, (size_t)n_pieces * sizeof(float), st));
        if (d_score && n_edges) SGL_HIP_CHECK(hipMemsetAsync(d_score, 0, (size_t)n_edges * sizeof(float), st));
        if (d_coef && n_edges) SGL_HIP_CHECK(hipMemsetAsync(d_coef, 0, (size_t)n_edges * sizeof(float), st));
        return SGL_OK;
    }
    const bool vec4 = ldz % 4 == 0 && aligned_to(d_z, 16);
    const int vec = vec4 ? 4 : 1;
    // chunks per lane of the compiled instance: 1 (any lane count), then 64 lanes with 2 / 4 / 8 vectors or 2 / 8 / 32 floats; 0 beyond
    const sgl::SliceInstance in = sgl::slice_instance(d, vec, sgl::EdgeLossSlices::chunks(vec));
    const int ovec = (lddz % 4 == 0 && aligned_to(d_dz, 16) && (n_partial == 0 || (ldp % 4 == 0 && aligned_to(d_partial, 16)))) ? 1 : 0;
    if (n_pieces > 0) {
        const int64_t per_block = 256 / in.lpr;
        const int64_t blocks = (n_pieces + per_block - 1) / per_block;
        if (!sgl::launch_fits(blocks, 256)) return sgl::fail(SGL_ERR_UNSUPPORTED, "%s: too many pieces for one launch (split the table)", who);
        const dim3 grid((unsigned)blocks);
        const int di = (int)d;
        // (ch = 0, the in-place form, is a compiled instance of this family)
        auto launch = [&](auto M) {
            return with_slice_instance<sgl::EdgeLossSlices, 0>(in, vec4, [&](auto L, auto V, auto C) {
                hipLaunchKernelGGL((edge_loss_grad_kernel<L, V, M, C>), grid, dim3(256), 0, st, d_z, ldz, n, di, d_pieces, n_pieces, d_inc_other,
                                   d_inc_edge, d_labels, d_given, w, d_dz, lddz, d_partial, ldp, ovec, d_score, d_coef, d_piece_loss);
            });
        };
        const bool launched = mode == MODE_SIGMOID_LOGITS ? launch(Int<MODE_SIGMOID_LOGITS>{})
                              : mode == MODE_LOGITS       ? launch(Int<MODE_LOGITS>{})
                                                          : launch(Int<MODE_GIVEN>{});
        if (!launched) return sgl::fail(SGL_ERR_UNSUPPORTED, "%s: no kernel instance for %d lanes x %d chunks", who, in.lpr, in.ch);
        SGL_LAUNCH_CHECK(who);
    }
    if (n_fold > 0) {
        const int64_t blocks = sgl::loss_grid((n_fold + 3) / 4, kMaxFoldBlocks);
        hipLaunchKernelGGL(edge_fold_kernel, dim3((unsigned)blocks), dim3(256), 0, st, d_fold, n_fold, d_partial, ldp, (int)d, d_dz, lddz);
        SGL_LAUNCH_CHECK(who);
    }
    return SGL_OK;
}
