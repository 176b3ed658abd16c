// Internal helpers shared by the translation units of libsgl_hip.so (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/sgl_hip.h"

#define SGL_EXPORT extern "C" __attribute__((visibility("default")))

namespace sgl {

// thread-local last-error text (sgl_last_error)
void set_error(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
const char *get_error();

inline int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
inline int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    set_error("%s", buf);
    return code;
}

#define SGL_HIP_CHECK(expr)                                                                          \
    do {                                                                                             \
        hipError_t _e = (expr);                                                                      \
        if (_e != hipSuccess)                                                                        \
            return ::sgl::fail((int)_e, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, \
                               __LINE__);                                                            \
    } while (0)

#define SGL_REQUIRE(cond, ...)                                     \
    do {                                                           \
        if (!(cond)) return ::sgl::fail(SGL_ERR_INVALID, __VA_ARGS__); \
    } while (0)

// A row width (d, c, k, d + pad_cols) beyond SGL_MAX_WIDTH (include/sgl_hip.h): the kernels hold a column in `int` and step it by up
// to a tile (lanes x floats per lane, c + 4, d + 3), which would wrap in the last columns below 2^31 -- refused by name, before any launch
#define SGL_REQUIRE_WIDTH(who, what, v)                                                                                          \
    do {                                                                                                                         \
        if ((int64_t)(v) > (int64_t)SGL_MAX_WIDTH)                                                                               \
            return ::sgl::fail(SGL_ERR_UNSUPPORTED, "%s: %s=%lld is wider than SGL_MAX_WIDTH=%lld", who, what, (long long)(v),   \
                               (long long)SGL_MAX_WIDTH);                                                                        \
    } while (0)

// ---- execution plan (host) ---------------------------------------------------------------------------------
struct Piece {
    int64_t begin;  // first non-zero (absolute)
    int32_t len;    // number of non-zeros
    int32_t row;    // output row
};

struct Plan {
    int64_t n_rows = 0;
    std::vector<int32_t> items;        // (row_begin, row_end) pairs
    std::vector<Piece> pieces;         // pieces of long rows, in row / storage order
    std::vector<int32_t> long_row;     // rows that were split
    std::vector<int32_t> long_first;   // [n_long+1] first piece of each long row
    int64_t max_item_rows = 0, max_item_nnz = 0;
};

constexpr int kMaxItemRows = 63;        // row-pointer window of one wavefront: 64 lanes hold rows+1 offsets
constexpr int kDefaultItemNnz = 512;
constexpr int kDefaultLongRowNnz = 2048;
constexpr int64_t kSmallLaunchNnz = 100000000;   // below this a launch gets 256-nnz work items (sgl_csr_create)

int build_plan(Plan &plan, const int64_t *rowptr, int64_t n_rows, int32_t item_nnz, int32_t long_row_nnz);

// tuning knobs (sgl_set_tuning)
int64_t tuning(const char *key, int64_t dflt);

// grid of a loss-kernel launch (K9, K11's fold, K12, K14) that strides over `wanted` blocks of work: the kernel's own cap, or the
// tuning key loss_blocks where it is > 0 -- the tests' way to the strided form at small sizes; read once per launch
inline int64_t loss_grid(int64_t wanted, int64_t cap) {
    const int64_t forced = tuning("loss_blocks", 0);
    if (forced > 0 && forced < cap) cap = forced;
    return wanted < cap ? wanted : cap;
}
// the same for a register kernel of K9, K12, K14 that strides over batches of n rows: `groups` lane groups per workgroup (256 / LPR)
// x `u` rows per group make one batch
struct BatchGrid {
    int64_t n_batches, blocks;
};
inline BatchGrid loss_batch_grid(int64_t n, int groups, int u, int64_t cap) {
    const int64_t per_batch = (int64_t)groups * u;
    const int64_t n_batches = (n + per_batch - 1) / per_batch;
    return {n_batches, loss_grid(n_batches, cap)};
}

// what sgl_csr_create takes for item_nnz <= 0 / long_row_nnz == 0: functions of the matrix's nnz only (sgl_core.cpp)
int32_t default_item_nnz(int64_t nnz);
int32_t default_long_row_nnz(int64_t nnz);

// ---- SpMM launch rule (host, sgl_core.cpp): one rule for the fp32 and the bfloat16 kernel --------------------
struct SpmmLayout {
    int group, nch, ulevel, waves;   // lanes per feature row (R = 64 / group non-zero slots) x column chunks per lane; level of unroll_of; wavefronts per workgroup
    bool nt;                         // non-temporal CSR stream / Y stores (fp32 only)
};
// `lanes` = columns of the slice / elements per lane; reads the tuning keys spmm_group, spmm_unroll, spmm_nt, spmm_waves
SpmmLayout spmm_layout(int lanes, bool strict, int64_t nnz, int64_t n_rows, bool bf16);

// gathers in flight per lane (the template argument U of spmm_kernel / spmm_bf16_kernel), scaled down with the number of column
// chunks to bound registers.  Level 3 (32 in flight, one-row-per-step layout only) is compiled for fp32 alone.
constexpr int unroll_of(int group, int nch, int ulevel) {
    const int uh = (nch == 1) ? 8 : (nch == 2 ? 4 : 2);
    return ulevel == 2 ? uh * 2 / (nch == 1 ? 1 : 2) : ulevel == 3 ? ((nch == 1 && group == 64) ? 32 : uh) : ulevel == 0 ? uh / 2 : uh;
}

// ---- row rule (host, sgl_core.cpp): lanes x chunks of the register-resident row kernels, one rule for float32 and bfloat16 hops ----
struct RowLayout {
    int lpr, ch;         // lanes per row x 16-byte chunks per lane
};
struct RowInstance {
    int lpr, ch, hmax;   // hmax: the even hop capacity of the compiled instance; 0 = the layout has none for this hop count
};
int pick_lpr(int64_t d, int vec);                                    // the smallest of 8 / 16 / 32 / 64 lanes that covers ceil(d / vec)

// ---- slice rule (host, sgl_core.cpp): the instance of a loss / k-means kernel (K9, K11, K12, K14) whose lanes keep a slice of a row ----
// The 64-lane instances of a family are compiled for these numbers of vectors per lane, one list per lane size; the rule
// (slice_instance) and the typed dispatch (with_slice_instance, sgl_rows.h) both read them here and nowhere else.
struct ChunkList {
    const int *values;
    int count;
};
template <int... Cs>
struct Chunks {
    static constexpr int values[] = {Cs...};
    static constexpr ChunkList list() { return {values, (int)sizeof...(Cs)}; }
};
template <typename V4, typename V1>
struct SliceFamily {
    using Vec4 = V4;     // lanes of 16 bytes
    using Vec1 = V1;     // lanes of one float
    static constexpr ChunkList chunks(int vec) { return vec == 4 ? V4::list() : V1::list(); }
};
using KmeansSlices = SliceFamily<Chunks<2, 3, 4, 6, 8>, Chunks<2, 4, 8, 16, 32>>;   // K9: rows of up to 2048 floats
using EdgeLossSlices = SliceFamily<Chunks<2, 4, 8>, Chunks<2, 8, 32>>;              // K11
using ClusterLossSlices = SliceFamily<Chunks<2, 4, 8>, Chunks<2, 8, 32>>;           // K12
using ClassLossSlices = SliceFamily<Chunks<2, 4>, Chunks<2, 4, 8, 16>>;             // K14: up to 1024 logits in at most 16 registers
struct SliceInstance {
    int lpr, ch;         // lanes per row x vectors per lane; ch = 0: beyond the register layouts (64 lanes)
};
SliceInstance slice_instance(int64_t width, int vec, ChunkList compiled);
RowLayout row_layout(int64_t d, int n_hops, bool allow_8x5 = false);  // reads the tuning keys row_lpr32x2, row_narrow_groups
RowInstance row_instance(int64_t d, int n_hops, bool allow_8x5 = false);
int out_cols(int64_t d, int64_t pad, int64_t room);                  // columns a row kernel writes; reads row_whole_lines
int check_pad(const char *who, int64_t width, int64_t pad, int64_t ldo);

inline hipStream_t as_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }

// A HIP launch carries at most 2^32 - 1 threads per grid dimension; beyond that the launch is silently truncated on this
// stack (found the hard way at papers100M size).  One-thread-per-element launchers check this, the rest stride.
inline bool launch_fits(int64_t blocks, int64_t threads_per_block) {
    return blocks >= 0 && blocks * threads_per_block < ((int64_t)1 << 32) && blocks < (int64_t)INT32_MAX;
}

}  // namespace sgl

inline bool aligned_to(const void *p, size_t a) { return (reinterpret_cast<uintptr_t>(p) % a) == 0; }

struct sgl_plan {
    sgl::Plan p;
};
