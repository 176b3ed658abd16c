// The device CSR handle behind sgl_csr_t (include/sgl_hip.h): made, changed and destroyed in sgl_csr.hip, used by the translation
// units that launch SpMM kernels on it (sgl_spmm.hip: fp32 hops, sgl_spmm_bf16.hip: bfloat16 hops; what the two share is in
// sgl_spmm_common.h).  Not part of the ABI.
#pragma once
#include "sgl_common.h"

#include <atomic>
#include <memory>

struct sgl_csr {
    int64_t n_rows = 0, n_cols = 0, nnz = 0;
    const int64_t *d_rowptr = nullptr;
    const int32_t *d_col = nullptr;
    const float *d_val = nullptr;
    uint32_t flags = 0;
    int64_t n_items = 0, n_pieces = 0, n_long = 0;
    int32_t *d_items = nullptr;
    sgl::Piece *d_pieces = nullptr;
    int32_t *d_long_row = nullptr;
    int32_t *d_long_first = nullptr;
    float *d_partial = nullptr;
    size_t partial_cap = 0;  // floats
    std::vector<float *> retired;   // outgrown workspaces: a captured hipGraph may still replay into them (freed at destroy)
    int device = 0;
    const int32_t *d_rowmap = nullptr;   // caller's [n_rows] storage row -> output row (sgl_csr_set_rowmap), not owned
    int32_t *d_long_out = nullptr;       // output rows of the split rows under the row map
    // bumped by sgl_csr_set_values / sgl_csr_set_rowmap, set to ~0 by sgl_csr_destroy: a captured chain graph has the value and
    // row-map pointers of its capture baked in and refuses to replay once they changed (shared: outlives the handle)
    std::shared_ptr<std::atomic<uint64_t>> epoch = std::make_shared<std::atomic<uint64_t>>(0);
};
