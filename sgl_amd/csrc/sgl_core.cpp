// Host-only part of libsgl_hip.so: error text, tuning knobs, the SpMM launch rule, the row rule of the register-resident
// aggregator kernels and the SpMM execution-plan builder.
// No device code here, so these entry points work (and are unit-tested) on a machine without a GPU.
#include <algorithm>
#include <atomic>
#include <map>
#include <mutex>
#include <thread>

#include "sgl_common.h"

namespace sgl {

static thread_local std::string g_err;

void set_error(const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
}
const char *get_error() { return g_err.c_str(); }

static std::mutex g_tune_mu;
static std::map<std::string, int64_t> &tune_map() {
    static std::map<std::string, int64_t> m = {
        {"spmm_unroll", 0},      // 0 = auto; 1 / 3 / 2 = low / mid / high number of gathers in flight per lane
        {"spmm_vec", 0},         // 0 = widest legal lane access; 2 / 1 = cap at 8 / 4 bytes per lane
        {"spmm_nt", 0},          // 1 = non-temporal loads for the CSR stream / stores of Y
        {"spmm_group", 0},       // 0 = auto; force lanes-per-feature-row (8/16/32/64)
        {"spmm_waves", 0},       // 0 = default (4 waves per workgroup)
        {"spmm_xcd_remap", 1},   // contiguous row ranges per XCD
        {"spmm_heavy_first", 1}, // plan time: work items that end in a heavy row are issued first inside every XCD range
        {"agg_blocks", 0},       // 0 = one 16-byte element per thread (grid capped at 2^22 blocks); > 0 caps the grid of the streaming aggregators (grid-stride)
        {"loss_blocks", 0},      // 0 = each kernel's own cap; > 0 caps the grid of the k-means / cluster-loss / class-loss kernels and the edge-loss fold (grid-stride)
        {"nafs_fused", 1},       // 0 = force the two-pass NAFS path
        {"row_lpr32x2", 1},      // row-wise kernels, 128 < d <= 256: 32 lanes x 2 chunks per row (2 rows per wavefront)
        {"row_whole_lines", 1},    // gate / NAFS / concat outputs: the pad columns of a row pitch (< one line beyond d) are written as zeros
        {"row_narrow_groups", 1},  // row-wise kernels: 16 lanes x 3 / 8 lanes x 5 chunks when that at least halves the idle lane slots
                                   // (0 = off, 1 = both, 2 = 16 x 3 only, 3 = 8 x 5 only)
        {"gather_lpr", 0},       // row gather / scatter: 0 = the lane group that idles the fewest slots; 8 / 16 / 32 / 64 force one
        {"gather_hops_grid", 1},         // sgl_gather_hops_padded_f32: 1 = hop in blockIdx.y (default), 0 = hop loop inside the thread
        {"gather_rows_per_thread", 0},   // 0 = sized so that the grid is about one round of the chip (1 ... 16); else 1 / 2 / 4 / 8 / 16
        {"concat_flat_read", 1}, // whole-rows concat: read whole pitches contiguously across the block's rows (0 = row by row, hop by hop)
        {"concat_lds", 1},       // any-width concat of rows >= 256 floats: assemble the output row in LDS (1 = auto: whole rows per block
                                 // where 1024-float tiles would be < 85 % full, 2 = always tiles, 3 = always whole rows, 0 = funnel-select kernel)
    };
    return m;
}

int64_t tuning(const char *key, int64_t dflt) {
    std::lock_guard<std::mutex> lk(g_tune_mu);
    auto &m = tune_map();
    auto it = m.find(key);
    if (it == m.end()) return dflt;
    return it->second;
}

// One wavefront per item: small matrices get smaller items so that the chip (256 CUs x 4 SIMDs x 8 waves) still
// sees enough wavefronts to hide memory latency; large ones use the 512-nnz default.  In between -- a launch of fewer
// than ~200 000 such items, e.g. a rank's block of a sharded job: a few "rounds" of the 8 192 resident wavefronts --
// 256-nnz items end the launch more evenly (profiles/r03_probe_small_launch.log: -3 % at an eighth of the
// products-sized graph, neutral on the whole of it).  Results do not depend on the item size.
int32_t default_item_nnz(int64_t nnz) {
    const int64_t want_items = 256 * 4 * 8;
    const int64_t cap = nnz >= kSmallLaunchNnz ? kDefaultItemNnz : kDefaultItemNnz / 2;
    return (int32_t)std::min<int64_t>(cap, std::max<int64_t>(16, nnz / want_items));
}

// Where a row is cut into pieces.  A row is ONE sequential chain of gathers in one wavefront; on a small matrix the whole
// launch is only a few such chains long, so its longest row IS the launch (Pubmed-sized S0: a 171-nnz hub row of 2 KB gathers
// took 62 us per hop whatever the item size; cut at 32 non-zeros the hop takes 44 us, 0.52 -> 0.73 of the roofline,
// profiles/r04_small_graph_sweep.log).  The threshold depends on the matrix (its nnz) only -- never on the plan -- so any two
// plans of one matrix still cut the same rows at the same places and agree bit for bit; strict order never cuts.
int32_t default_long_row_nnz(int64_t nnz) {
    return nnz < (1 << 18) ? 32 : nnz < (1 << 20) ? 128 : nnz < (1 << 22) ? 512 : kDefaultLongRowNnz;
}

SpmmLayout spmm_layout(int lanes, bool strict, int64_t nnz, int64_t n_rows, bool bf16) {
    SpmmLayout L;
    // Lane layout (measured on MI355X, profiles/r01_sweep*.log): rows wider than 16 lanes (64 floats) are gathered one
    // non-zero per step by the whole wavefront (R = 1): as fast as two half-wave slots and it keeps the reference's
    // sequential fmaf order; narrower rows (bf16: d <= 128 with 16-byte lanes, the d = 100 hop is 13 lanes) pack
    // R = 64/GROUP non-zeros per step or the lanes would idle.  Rows wider than 64 lanes go in column chunks; strict
    // order always walks one non-zero per step.
    L.group = 64;
    L.nch = 1;
    if (lanes > 64) {
        const int need = (lanes + 63) / 64;
        L.nch = need <= 2 ? need : 4;
    } else if (!strict && lanes <= 16) {
        L.group = 8;
        while (L.group < lanes) L.group <<= 1;
    }
    const int64_t forced = tuning("spmm_group", 0);   // strict order keeps its one chain per row whatever the key says
    if (!strict && (forced == 8 || forced == 16 || forced == 32 || forced == 64) && L.nch == 1 && forced >= lanes) L.group = (int)forced;
    // gathers in flight per lane: 16 for the one-row-per-step layout, 8 for the packed ones (0 = this default).  A row's
    // remainder (nnz mod U) is gathered one dependent load at a time, so short rows want smaller batches: measured
    // (profiles/r02_flat_*.log) 51 nnz/row: U=16 8.73 ms vs U=8 8.79; 30 nnz/row (papers100M-shaped shard): U=8 37.2 ms
    // vs U=16 38.1; 6 nnz/row: U=4 11.27 vs U=8 11.36 vs U=16 13.9.  (A walk that batches across row ends was measured
    // too: within 1 % of this one with the right U, 2-4 % slower for d = 147 and in strict order -- not kept.)
    // bf16: the packed layouts take 16 per slot too from 40 non-zeros per row on (products shape, d = 100 at a 128-element
    // pitch: 4.47 ms per hop against 4.58 with 8 and 4.56 with 4, profiles/bf16_hop_dtype_unroll.json), 8 below.
    const bool whole_wave = L.group == 64 && L.nch == 1;
    L.ulevel = whole_wave ? 2 : 1;
    if (L.nch == 1 && n_rows > 0) {
        const double avg = (double)nnz / (double)n_rows;
        if (whole_wave) {
            if (avg < 12.0) L.ulevel = 0;
            else if (avg < 40.0) L.ulevel = 1;
        } else {
            L.ulevel = bf16 ? (avg >= 40.0 ? 2 : 1) : 1;
        }
    }
    const int64_t un = tuning("spmm_unroll", 0);
    if (un == 1) L.ulevel = 0;
    if (un == 2) L.ulevel = 2;
    if (un == 3) L.ulevel = 1;
    if (un == 4) L.ulevel = bf16 ? L.ulevel : 3;   // 32 gathers in flight (one-row-per-step layout only): fp32 alone compiles it
    L.nt = bf16 ? false : tuning("spmm_nt", 0) != 0;   // the bf16 kernel has no non-temporal variant
    L.waves = (int)tuning("spmm_waves", 0);
    if (L.waves != 1 && L.waves != 2 && L.waves != 4) L.waves = 4;
    return L;
}

// ---- row rule: lanes x chunks of a register-resident row kernel (sgl_rows.h dispatches on what these return) -----------------
int pick_lpr(int64_t d, int vec) {
    const int64_t lanes = (d + vec - 1) / vec;
    int lpr = 8;
    while (lpr < lanes && lpr < 64) lpr <<= 1;
    return lpr;
}

// The instance of a loss / k-means kernel (K9, K11, K12, K14) that serves rows of `width` floats read `vec` floats at a time: the
// narrowest lane group that covers the row with one vector per lane; beyond 64 lanes the next number of vectors per lane the family
// compiles (`compiled`, ascending: a list of sgl_common.h); beyond the last: ch = 0 -- the streaming kernel, K11's in-place form.
SliceInstance slice_instance(int64_t width, int vec, ChunkList compiled) {
    SliceInstance r;
    r.lpr = pick_lpr(width, vec);
    const int64_t chunks = (width + (int64_t)r.lpr * vec - 1) / ((int64_t)r.lpr * vec);
    r.ch = chunks <= 1 ? 1 : 0;
    for (int i = 0; i < compiled.count && r.ch == 0; ++i)
        if (chunks <= compiled.values[i]) r.ch = compiled.values[i];
    return r;
}

// A row of d floats is ceil(d / 4) 16-byte slots; LPR lanes take CH slots each (slot (c * LPR + l) of the row for lane l, chunk c),
// 64 / LPR rows per wavefront.  Power-of-two groups leave slots idle when the row is not a power of two wide, and idle slots still
// cost their share of every load and VALU instruction: d = 147 (BASELINE config 3: 100 features + 47 label columns = 37 slots) on
// 32 lanes x 2 chunks idles 27 of 64.  Narrow groups with more chunks per lane fit such rows far better -- 8 lanes x 5 chunks
// (40 slots, 8 rows per wavefront, every load instruction of a lane group is one whole 128-byte line) or 16 x 3 (48 slots) -- at
// the price of CH x HMAX hop vectors in registers, so they are instantiated for few hops only (<= 6 / <= 12) and chosen when they
// at least halve the idle slots.  Measured at d = 147 (profiles/r04_aggregators_layouts.log): 16 x 3 is as fast as 32 x 2 at 6 hops
// and 12-15 % faster at 11 (row-dot 0.597 -> 0.661 of peak, gate 0.539 -> 0.613, NAFS 0.536 -> 0.612); 8 x 5 (151 VGPRs, 3 waves
// per SIMD) pays only in the jk-score kernel (0.585 -> 0.657 at 6 hops) and is instantiated for that kernel alone (allow_8x5).  At
// 6 hops the gate / NAFS kernels are NOT issue-bound -- halving their VALU instructions and quartering their wavefronts changed
// nothing (profiles/r04_agg_pmc.md) -- what they lost against the plain sum was the partly written last line of the output row
// (store_row of sgl_rows.h, out_cols below).
static const int kNarrow[2][3] = {{16, 3, 12}, {8, 5, 6}};       // lanes, chunks, most hops instantiated

RowLayout row_layout(int64_t d, int n_hops, bool allow_8x5) {
    RowLayout r;
    r.lpr = pick_lpr(d, 4);
    r.ch = (d > r.lpr * 4) ? 2 : 1;
    if (r.lpr == 64 && r.ch == 1 && d > 128 && tuning("row_lpr32x2", 1) != 0) {   // 2 rows per wavefront
        r.lpr = 32;
        r.ch = 2;
    }
    if (tuning("row_narrow_groups", 1) != 0 && d <= r.lpr * 4 * r.ch) {
        const int slots = (int)((d + 3) / 4);
        const int64_t mode = tuning("row_narrow_groups", 1);       // 1: both candidates, 2: 16 x 3 only, 3: 8 x 5 only (measurements)
        for (const auto &c : kNarrow) {
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

// the compiled instance that serves n_hops in the layout: every even hop capacity up to 16 for the wide layouts, up to 12 / 6 for
// the narrow groups (CH x HMAX hop vectors live in registers)
RowInstance row_instance(int64_t d, int n_hops, bool allow_8x5) {
    const RowLayout r = row_layout(d, n_hops, allow_8x5);
    int most = 16;
    for (const auto &c : kNarrow)
        if (r.lpr == c[0] && r.ch == c[1]) most = c[2];
    const int hmax = (n_hops < 1 || n_hops > most) ? 0 : std::max(2, (n_hops + 1) / 2 * 2);
    return RowInstance{r.lpr, r.ch, hmax};
}

// Columns a row-producing kernel writes: the d data columns plus the `pad` columns after them that the CALLER declared to be the
// row's own padding (the *_padded_f32 entry points; sgl_amd.device passes the tail of the pitch of the outputs it allocates) --
// written as zeros, so that every line of the row is written whole.  The kernels never guess: with pad = 0 nothing beyond column
// d is touched.  `room` = the columns the lane layout reaches.
int out_cols(int64_t d, int64_t pad, int64_t room) {
    int64_t dw = tuning("row_whole_lines", 1) != 0 ? d + pad : d;
    if (dw > room) dw = room > d ? room / 4 * 4 : d;
    if (dw > d && dw % 4 != 0) dw = d;              // (validated by the entry points: d + pad is a whole number of vectors)
    return (int)dw;
}

int check_pad(const char *who, int64_t width, int64_t pad, int64_t ldo) {
    if (pad < 0 || width + pad > ldo) return fail(SGL_ERR_INVALID, "%s: pad_cols=%lld does not fit the output pitch", who, (long long)pad);
    if (pad > 0 && ((width + pad) % 4 != 0 || ldo % 4 != 0))
        return fail(SGL_ERR_INVALID, "%s: padded rows must be whole 16-byte vectors (width + pad_cols and ldo multiples of 4)", who);
    return SGL_OK;
}

// Issue order of the work items.  An item closes when it reaches item_nnz non-zeros, so one that ends in a heavy row holds up
// to item_nnz + long_row_nnz of them: several times the usual wavefront lifetime.  Where such an item is issued late, the launch
// ends with a few wavefronts on an otherwise empty chip -- one per cent of the single-GPU launch, but a rank's launch of the
// 8-rank job is only ~3.5 rounds of resident wavefronts (profiles/r03_probe_small_launch.log: -3.5 %).  Inside every XCD's range
// of the item list (the ranges spmm_kernel walks with 4 wavefronts per block) the items holding >= 2 x item_nnz non-zeros
// therefore go first, longest first; the others keep their row order.  Items are whole rows: results do not change.
static void heavy_items_first(Plan &plan, const int64_t *rowptr, int32_t item_nnz) {
    const int64_t n = (int64_t)plan.items.size() / 2;
    if (n < 64) return;
    const int64_t range = (((n + 3) / 4 + 7) / 8) * 4;
    const int64_t heavy = 2 * (int64_t)std::max(item_nnz, 1);
    struct It {
        int32_t b, e;
        int64_t nnz;
    };
    std::vector<It> seg;
    for (int64_t lo = 0; lo < n; lo += range) {
        const int64_t hi = std::min(n, lo + range);
        seg.clear();
        for (int64_t i = lo; i < hi; ++i) {
            const int32_t b = plan.items[2 * i], e = plan.items[2 * i + 1];
            seg.push_back(It{b, e, rowptr[e] - rowptr[b]});
        }
        auto mid = std::stable_partition(seg.begin(), seg.end(), [&](const It &t) { return t.nnz >= heavy; });
        std::stable_sort(seg.begin(), mid, [](const It &x, const It &y) { return x.nnz > y.nnz; });
        for (int64_t i = lo; i < hi; ++i) {
            plan.items[2 * i] = seg[(size_t)(i - lo)].b;
            plan.items[2 * i + 1] = seg[(size_t)(i - lo)].e;
        }
    }
}

// Greedy partition of the rows [r0, r1) into work items (see include/sgl_hip.h, "execution plan"); a fresh item starts at r0.
static int build_segment(Plan &plan, const int64_t *rowptr, int64_t r0, int64_t r1, int32_t item_nnz, int32_t long_row_nnz) {
    const bool split = long_row_nnz > 0;
    int64_t cur_begin = r0, cur_nnz = 0;
    auto close_item = [&](int64_t end) {
        if (end > cur_begin) {
            plan.items.push_back((int32_t)cur_begin);
            plan.items.push_back((int32_t)end);
            plan.max_item_rows = std::max<int64_t>(plan.max_item_rows, end - cur_begin);
            plan.max_item_nnz = std::max<int64_t>(plan.max_item_nnz, cur_nnz);
        }
        cur_begin = end;
        cur_nnz = 0;
    };
    for (int64_t r = r0; r < r1; ++r) {
        const int64_t b = rowptr[r], e = rowptr[r + 1];
        if (e < b) return fail(SGL_ERR_INVALID, "build_plan: row pointers decrease at row %lld", (long long)r);
        const int64_t deg = e - b;
        if (!split && deg >= (int64_t)INT32_MAX)
            return fail(SGL_ERR_UNSUPPORTED, "build_plan: a row with >= 2^31 non-zeros needs long_row_nnz > 0");
        if (split && deg > long_row_nnz) {
            close_item(r);  // rows before the long one
            plan.long_row.push_back((int32_t)r);
            for (int64_t p = b; p < e; p += long_row_nnz) {
                Piece pc;
                pc.begin = p;
                pc.len = (int32_t)std::min<int64_t>(long_row_nnz, e - p);
                pc.row = (int32_t)r;
                plan.pieces.push_back(pc);
            }
            plan.long_first.push_back((int32_t)plan.pieces.size());
            cur_begin = r + 1;
            cur_nnz = 0;
            continue;
        }
        // a row that would push the item past 2^31-1 relative offsets cannot happen when split is on
        // (deg <= long_row_nnz); without splitting close the item first so offsets stay 32-bit.
        if (cur_nnz > 0 && cur_nnz + deg >= (int64_t)INT32_MAX) close_item(r);
        cur_nnz += deg;
        if (cur_nnz >= item_nnz || (r + 1 - cur_begin) >= kMaxItemRows) close_item(r + 1);
    }
    close_item(r1);
    return SGL_OK;
}

// Rows are cut into segments of kPlanSegmentRows; every segment is partitioned on its own (a fresh item starts at its first row:
// at most one short item per 2^20 rows) by a team of host threads and the pieces are laid end to end.  The plan depends on the
// segment size only, never on the number of threads; matrices of up to two segments -- everything but the 10^7 ... 10^8-row
// blocks of the papers100M-sized jobs, where the serial loop was hundreds of milliseconds of setup -- are one segment: the plan
// they always had.  Items are whole rows and long rows are cut per row: results do not depend on any of this.
constexpr int64_t kPlanSegmentRows = (int64_t)1 << 20;

int build_plan(Plan &plan, const int64_t *rowptr, int64_t n_rows, int32_t item_nnz, int32_t long_row_nnz) {
    if (n_rows < 0 || (n_rows > 0 && rowptr == nullptr)) return fail(SGL_ERR_INVALID, "build_plan: bad arguments");
    if (n_rows >= (int64_t)INT32_MAX) return fail(SGL_ERR_UNSUPPORTED, "build_plan: n_rows >= 2^31 (shard the matrix)");
    if (item_nnz <= 0) item_nnz = kDefaultItemNnz;
    plan = Plan();
    plan.n_rows = n_rows;
    plan.long_first.push_back(0);
    if (n_rows <= 2 * kPlanSegmentRows) {
        const int rc = build_segment(plan, rowptr, 0, n_rows, item_nnz, long_row_nnz);
        if (rc != SGL_OK) return rc;
    } else {
        const int64_t n_seg = (n_rows + kPlanSegmentRows - 1) / kPlanSegmentRows;
        std::vector<Plan> segs((size_t)n_seg);
        std::vector<int> rcs((size_t)n_seg, SGL_OK);
        std::vector<std::string> errs((size_t)n_seg);
        const int n_thr = (int)std::max<int64_t>(1, std::min<int64_t>({(int64_t)std::thread::hardware_concurrency(), (int64_t)16, n_seg}));
        std::atomic<int64_t> next{0};
        auto work = [&]() {
            for (int64_t sidx = next.fetch_add(1); sidx < n_seg; sidx = next.fetch_add(1)) {
                const int64_t r0 = sidx * kPlanSegmentRows, r1 = std::min(n_rows, r0 + kPlanSegmentRows);
                rcs[(size_t)sidx] = build_segment(segs[(size_t)sidx], rowptr, r0, r1, item_nnz, long_row_nnz);
                if (rcs[(size_t)sidx] != SGL_OK) errs[(size_t)sidx] = get_error();      // the error text is per thread
            }
        };
        std::vector<std::thread> team;
        for (int t = 1; t < n_thr; ++t) team.emplace_back(work);
        work();
        for (auto &t : team) t.join();
        size_t n_items = 0, n_pieces = 0, n_long = 0;
        for (int64_t sidx = 0; sidx < n_seg; ++sidx) {
            if (rcs[(size_t)sidx] != SGL_OK) return fail(rcs[(size_t)sidx], "%s", errs[(size_t)sidx].c_str());
            n_items += segs[(size_t)sidx].items.size();
            n_pieces += segs[(size_t)sidx].pieces.size();
            n_long += segs[(size_t)sidx].long_row.size();
        }
        plan.items.reserve(n_items);
        plan.pieces.reserve(n_pieces);
        plan.long_row.reserve(n_long);
        plan.long_first.reserve(n_long + 1);
        for (auto &sg : segs) {
            const int32_t piece0 = (int32_t)plan.pieces.size();
            plan.items.insert(plan.items.end(), sg.items.begin(), sg.items.end());
            plan.pieces.insert(plan.pieces.end(), sg.pieces.begin(), sg.pieces.end());
            plan.long_row.insert(plan.long_row.end(), sg.long_row.begin(), sg.long_row.end());
            for (int32_t lf : sg.long_first) plan.long_first.push_back(piece0 + lf);   // (a segment's list has no leading 0)
            plan.max_item_rows = std::max(plan.max_item_rows, sg.max_item_rows);
            plan.max_item_nnz = std::max(plan.max_item_nnz, sg.max_item_nnz);
            sg = Plan();
        }
    }
    if (tuning("spmm_heavy_first", 1) != 0) heavy_items_first(plan, rowptr, item_nnz);
    return SGL_OK;
}

}  // namespace sgl

SGL_EXPORT int sgl_version(void) { return 110; }

SGL_EXPORT const char *sgl_last_error(void) { return sgl::get_error(); }

SGL_EXPORT int sgl_device_count(int *count) {
    if (!count) return sgl::fail(SGL_ERR_INVALID, "sgl_device_count: NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        n = 0;
    }
    *count = n;
    return SGL_OK;
}

SGL_EXPORT int sgl_set_tuning(const char *key, int64_t value) {
    if (!key) return sgl::fail(SGL_ERR_INVALID, "sgl_set_tuning: NULL key");
    std::lock_guard<std::mutex> lk(sgl::g_tune_mu);
    auto &m = sgl::tune_map();
    auto it = m.find(key);
    if (it == m.end()) return sgl::fail(SGL_ERR_INVALID, "sgl_set_tuning: unknown key '%s'", key);
    it->second = value;
    return SGL_OK;
}

SGL_EXPORT int sgl_get_tuning(const char *key, int64_t *value) {
    if (!key || !value) return sgl::fail(SGL_ERR_INVALID, "sgl_get_tuning: NULL");
    std::lock_guard<std::mutex> lk(sgl::g_tune_mu);
    auto &m = sgl::tune_map();
    auto it = m.find(key);
    if (it == m.end()) return sgl::fail(SGL_ERR_INVALID, "sgl_get_tuning: unknown key '%s'", key);
    *value = it->second;
    return SGL_OK;
}

SGL_EXPORT int sgl_plan_build(sgl_plan_t **out, const int64_t *h_rowptr, int64_t n_rows, int32_t item_nnz,
                              int32_t long_row_nnz) {
    if (!out) return sgl::fail(SGL_ERR_INVALID, "sgl_plan_build: NULL out");
    *out = nullptr;
    sgl_plan_t *p = new (std::nothrow) sgl_plan_t();
    if (!p) return sgl::fail(SGL_ERR_ALLOC, "sgl_plan_build: out of memory");
    int rc = sgl::build_plan(p->p, h_rowptr, n_rows, item_nnz, long_row_nnz);
    if (rc != SGL_OK) {
        delete p;
        return rc;
    }
    *out = p;
    return SGL_OK;
}

SGL_EXPORT int sgl_plan_counts(const sgl_plan_t *plan, int64_t counts[8]) {
    if (!plan || !counts) return sgl::fail(SGL_ERR_INVALID, "sgl_plan_counts: NULL");
    memset(counts, 0, 8 * sizeof(int64_t));
    counts[0] = (int64_t)plan->p.items.size() / 2;
    counts[1] = (int64_t)plan->p.pieces.size();
    counts[2] = (int64_t)plan->p.long_row.size();
    counts[3] = plan->p.max_item_rows;
    counts[4] = plan->p.max_item_nnz;
    counts[5] = plan->p.n_rows;
    return SGL_OK;
}

SGL_EXPORT int sgl_plan_export(const sgl_plan_t *plan, int32_t *h_items, int64_t *h_piece_begin, int32_t *h_piece_len,
                               int32_t *h_piece_row, int32_t *h_long_row, int32_t *h_long_first) {
    if (!plan) return sgl::fail(SGL_ERR_INVALID, "sgl_plan_export: NULL plan");
    const sgl::Plan &p = plan->p;
    if (h_items && !p.items.empty()) memcpy(h_items, p.items.data(), p.items.size() * sizeof(int32_t));
    for (size_t i = 0; i < p.pieces.size(); ++i) {
        if (h_piece_begin) h_piece_begin[i] = p.pieces[i].begin;
        if (h_piece_len) h_piece_len[i] = p.pieces[i].len;
        if (h_piece_row) h_piece_row[i] = p.pieces[i].row;
    }
    if (h_long_row && !p.long_row.empty()) memcpy(h_long_row, p.long_row.data(), p.long_row.size() * sizeof(int32_t));
    if (h_long_first) memcpy(h_long_first, p.long_first.data(), p.long_first.size() * sizeof(int32_t));
    return SGL_OK;
}

SGL_EXPORT void sgl_plan_destroy(sgl_plan_t *plan) { delete plan; }
