// The life cycle of the device CSR handle sgl_csr_t (sgl_csr.h): creation with its host-built execution plan (sgl_core.cpp), row map,
// new values, info, destruction.  The SpMM kernels that run on the handle are in sgl_spmm.hip (fp32 hops) and sgl_spmm_bf16.hip
// (bfloat16 hops).
#include "sgl_csr.h"

// permutation check of a row map on the device: every entry in range, no output row named twice
__global__ __launch_bounds__(256) void rowmap_check_kernel(const int32_t *__restrict__ map, const int64_t n, unsigned *__restrict__ seen,
                                                           int *__restrict__ bad) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t m = map[i];
    if (m < 0 || m >= n) {
        atomicOr(bad, 1);
        return;
    }
    const unsigned bit = 1u << (m & 31);
    if (atomicOr(&seen[m >> 5], bit) & bit) atomicOr(bad, 2);
}

// The row pointers come to the host for the plan (sgl::build_plan).  Small ones in one copy; the 10^7 ... 10^8 rows of a
// papers100M-sized block (up to 888 MB) through two page-locked 32 MB staging buffers, the copy of chunk c + 1 in flight while
// chunk c is unpacked -- a pageable destination of that size is staged by the runtime at a fraction of the link rate -- and the
// host waits on the chunks' EVENTS, not on the stream: work the caller queued behind this call on other streams is not held up.
static int fetch_rowptr(std::vector<int64_t> &h, const int64_t *d, hipStream_t st) {
    const size_t n = h.size();
    constexpr size_t kChunk = (size_t)4 << 20;                        // elements: 32 MB
    if (n <= 2 * kChunk) {
        SGL_HIP_CHECK(hipMemcpyAsync(h.data(), d, n * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        SGL_HIP_CHECK(hipStreamSynchronize(st));
        return SGL_OK;
    }
    int64_t *stage[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    int rc = SGL_OK;
    auto cleanup = [&]() {
        for (int i = 0; i < 2; ++i) {
            if (stage[i]) (void)hipHostFree(stage[i]);
            if (ev[i]) (void)hipEventDestroy(ev[i]);
        }
    };
    for (int i = 0; i < 2 && rc == SGL_OK; ++i) {
        if (hipHostMalloc((void **)&stage[i], kChunk * sizeof(int64_t), hipHostMallocDefault) != hipSuccess ||
            hipEventCreateWithFlags(&ev[i], hipEventDisableTiming) != hipSuccess)
            rc = sgl::fail(SGL_ERR_ALLOC, "sgl_csr_create: no page-locked staging buffer for the row pointers");
    }
    const size_t n_chunks = (n + kChunk - 1) / kChunk;
    auto issue = [&](size_t c) -> hipError_t {
        const size_t off = c * kChunk, len = std::min(kChunk, n - off);
        hipError_t e = hipMemcpyAsync(stage[c & 1], d + off, len * sizeof(int64_t), hipMemcpyDeviceToHost, st);
        return e != hipSuccess ? e : hipEventRecord(ev[c & 1], st);
    };
    if (rc == SGL_OK && issue(0) != hipSuccess) rc = sgl::fail(SGL_ERR_INVALID, "sgl_csr_create: copying the row pointers failed");
    for (size_t c = 0; c < n_chunks && rc == SGL_OK; ++c) {
        if (hipEventSynchronize(ev[c & 1]) != hipSuccess) {
            rc = sgl::fail(SGL_ERR_INVALID, "sgl_csr_create: copying the row pointers failed");
            break;
        }
        const size_t off = c * kChunk, len = std::min(kChunk, n - off);
        // chunk c sits in stage[c & 1]; chunk c + 1 goes to the other buffer, whose contents (chunk c - 1) were unpacked in the last round
        if (c + 1 < n_chunks && issue(c + 1) != hipSuccess) {
            rc = sgl::fail(SGL_ERR_INVALID, "sgl_csr_create: copying the row pointers failed");
            break;
        }
        memcpy(h.data() + off, stage[c & 1], len * sizeof(int64_t));
    }
    if (rc != SGL_OK) (void)hipStreamSynchronize(st);                   // nothing may still write into the buffers we free
    cleanup();
    return rc;
}

SGL_EXPORT int sgl_csr_create(sgl_csr_t **out, int64_t n_rows, int64_t n_cols, int64_t nnz, const int64_t *d_rowptr,
                              const int32_t *d_col, const float *d_val, uint32_t flags, int32_t item_nnz,
                              int32_t long_row_nnz, void *stream) {
    if (!out) return sgl::fail(SGL_ERR_INVALID, "sgl_csr_create: NULL out");
    *out = nullptr;
    SGL_REQUIRE(n_rows >= 0 && n_cols >= 0 && nnz >= 0, "sgl_csr_create: negative size");
    SGL_REQUIRE(n_rows < INT32_MAX && n_cols < INT32_MAX, "sgl_csr_create: n_rows/n_cols must be < 2^31 (int32 ids)");
    SGL_REQUIRE(d_rowptr != nullptr, "sgl_csr_create: NULL row pointers");
    SGL_REQUIRE(nnz == 0 || (d_col && d_val), "sgl_csr_create: NULL col/val with nnz > 0");
    hipStream_t st = sgl::as_stream(stream);
    std::vector<int64_t> h_rowptr((size_t)n_rows + 1);
    {
        const int rc_fetch = fetch_rowptr(h_rowptr, d_rowptr, st);
        if (rc_fetch != SGL_OK) return rc_fetch;
    }
    SGL_REQUIRE(h_rowptr[0] == 0 && h_rowptr[n_rows] == nnz, "sgl_csr_create: rowptr[0]=%lld rowptr[n]=%lld but nnz=%lld",
                (long long)h_rowptr[0], (long long)h_rowptr[n_rows], (long long)nnz);
    if (item_nnz <= 0) item_nnz = sgl::default_item_nnz(nnz);
    if (long_row_nnz == 0) long_row_nnz = sgl::default_long_row_nnz(nnz);
    if (flags & SGL_CSR_STRICT_ORDER) long_row_nnz = -1;
    sgl::Plan plan;
    int rc = sgl::build_plan(plan, h_rowptr.data(), n_rows, item_nnz, long_row_nnz);
    if (rc != SGL_OK) return rc;

    sgl_csr_t *h = new (std::nothrow) sgl_csr_t();
    if (!h) return sgl::fail(SGL_ERR_ALLOC, "sgl_csr_create: out of memory");
    h->n_rows = n_rows;
    h->n_cols = n_cols;
    h->nnz = nnz;
    h->d_rowptr = d_rowptr;
    h->d_col = d_col;
    h->d_val = d_val;
    h->flags = flags;
    h->n_items = (int64_t)plan.items.size() / 2;
    h->n_pieces = (int64_t)plan.pieces.size();
    h->n_long = (int64_t)plan.long_row.size();
    (void)hipGetDevice(&h->device);
    auto upload = [&](void **dst, const void *src, size_t bytes) -> int {
        if (bytes == 0) return SGL_OK;
        SGL_HIP_CHECK(hipMalloc(dst, bytes));
        SGL_HIP_CHECK(hipMemcpyAsync(*dst, src, bytes, hipMemcpyHostToDevice, st));
        return SGL_OK;
    };
    rc = upload((void **)&h->d_items, plan.items.data(), plan.items.size() * sizeof(int32_t));
    if (rc == SGL_OK) rc = upload((void **)&h->d_pieces, plan.pieces.data(), plan.pieces.size() * sizeof(sgl::Piece));
    if (rc == SGL_OK) rc = upload((void **)&h->d_long_row, plan.long_row.data(), plan.long_row.size() * sizeof(int32_t));
    if (rc == SGL_OK && h->n_long > 0)
        rc = upload((void **)&h->d_long_first, plan.long_first.data(), plan.long_first.size() * sizeof(int32_t));
    if (rc == SGL_OK) {
        hipError_t e = hipStreamSynchronize(st);  // host vectors die at return
        if (e != hipSuccess) rc = sgl::fail((int)e, "sgl_csr_create: sync failed: %s", hipGetErrorString(e));
    }
    if (rc != SGL_OK) {
        sgl_csr_destroy(h);
        return rc;
    }
    *out = h;
    return SGL_OK;
}

SGL_EXPORT int sgl_csr_destroy(sgl_csr_t *h) {
    if (!h) return SGL_OK;
    h->epoch->store(~0ull);                // a chain graph captured on this handle refuses to replay from now on
    (void)hipFree(h->d_items);
    (void)hipFree(h->d_pieces);
    (void)hipFree(h->d_long_row);
    (void)hipFree(h->d_long_first);
    (void)hipFree(h->d_partial);
    (void)hipFree(h->d_long_out);
    for (float *p : h->retired) (void)hipFree(p);
    delete h;
    return SGL_OK;
}

// The handle's rows are stored in processing order: storage row i is row d_rowmap[i] of the product (a permutation of
// 0..n_rows-1, e.g. sgl_reorder_community's order applied with sgl_csr_permute_rows).  Every product of this handle then writes
// (and, for the epilogues, reads the residual / running aggregate of) output row d_rowmap[i]; X is gathered by the ORIGINAL
// column ids and every row keeps the order of its terms, so results are bit-identical to the unpermuted matrix's.  NULL
// removes the map.  The array must stay alive as long as the handle uses it.
SGL_EXPORT int sgl_csr_set_rowmap(sgl_csr_t *h, const int32_t *d_rowmap, void *stream) {
    if (!h) return sgl::fail(SGL_ERR_INVALID, "sgl_csr_set_rowmap: NULL handle");
    h->d_rowmap = nullptr;
    h->epoch->fetch_add(1);
    if (!d_rowmap || h->n_rows == 0) return SGL_OK;
    hipStream_t st = sgl::as_stream(stream);
    {   // a map that is not a permutation would make every SpMM write rows out of bounds or leave rows unwritten: checked once
        const size_t words = (size_t)(h->n_rows + 31) / 32;
        unsigned *d_seen = nullptr;
        SGL_HIP_CHECK(hipMalloc(&d_seen, (words + 1) * sizeof(unsigned)));
        int *d_bad = reinterpret_cast<int *>(d_seen + words);
        hipError_t e = hipMemsetAsync(d_seen, 0, (words + 1) * sizeof(unsigned), st);
        int bad = 0;
        if (e == hipSuccess) {
            hipLaunchKernelGGL(rowmap_check_kernel, dim3((unsigned)((h->n_rows + 255) / 256)), dim3(256), 0, st, d_rowmap, h->n_rows, d_seen, d_bad);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        (void)hipFree(d_seen);
        if (e != hipSuccess) return sgl::fail((int)e, "sgl_csr_set_rowmap: validation failed: %s", hipGetErrorString(e));
        SGL_REQUIRE(!(bad & 1), "sgl_csr_set_rowmap: map entry outside [0, n_rows)");
        SGL_REQUIRE(!(bad & 2), "sgl_csr_set_rowmap: the map names an output row twice (it must be a permutation)");
    }
    if (h->n_long > 0) {   // the split rows' fix-up writes whole output rows: give it their mapped ids
        std::vector<int32_t> map((size_t)h->n_rows), rows((size_t)h->n_long);
        SGL_HIP_CHECK(hipMemcpyAsync(map.data(), d_rowmap, map.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        SGL_HIP_CHECK(hipMemcpyAsync(rows.data(), h->d_long_row, rows.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        SGL_HIP_CHECK(hipStreamSynchronize(st));
        for (auto &r : rows) {
            SGL_REQUIRE(r >= 0 && r < h->n_rows && map[r] >= 0 && map[r] < h->n_rows, "sgl_csr_set_rowmap: map entry outside [0, n_rows)");
            r = map[r];
        }
        if (!h->d_long_out) SGL_HIP_CHECK(hipMalloc(&h->d_long_out, rows.size() * sizeof(int32_t)));
        SGL_HIP_CHECK(hipMemcpyAsync(h->d_long_out, rows.data(), rows.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
        SGL_HIP_CHECK(hipStreamSynchronize(st));
    }
    h->d_rowmap = d_rowmap;
    return SGL_OK;
}

// Same structure, new values: the plan depends on the row pointers only, so re-weighting the matrix (another r of the
// NAFS ensemble, another alpha of a PPR sweep: sgl/tasks/node_clustering.py:205-217) needs no new plan.
SGL_EXPORT int sgl_csr_set_values(sgl_csr_t *h, const float *d_val) {
    if (!h) return sgl::fail(SGL_ERR_INVALID, "sgl_csr_set_values: NULL handle");
    SGL_REQUIRE(h->nnz == 0 || d_val, "sgl_csr_set_values: NULL values");
    if (d_val != h->d_val) h->epoch->fetch_add(1);
    h->d_val = d_val;
    return SGL_OK;
}

SGL_EXPORT int sgl_csr_info(const sgl_csr_t *h, int64_t info[8]) {
    if (!h || !info) return sgl::fail(SGL_ERR_INVALID, "sgl_csr_info: NULL");
    info[0] = h->n_rows;
    info[1] = h->n_cols;
    info[2] = h->nnz;
    info[3] = h->n_items;
    info[4] = h->n_pieces;
    info[5] = h->n_long;
    info[6] = h->flags;
    info[7] = (int64_t)(h->partial_cap * sizeof(float));
    return SGL_OK;
}
