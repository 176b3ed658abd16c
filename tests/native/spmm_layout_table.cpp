// The SpMM launch rule and the handle's default thresholds as the library computes them, without a GPU: sgl::spmm_layout,
// sgl::default_item_nnz and sgl::default_long_row_nnz of sgl_amd/csrc/sgl_core.cpp, built by tests/test_spmm_order_cpu.py with g++
// and compared there against the restatements of tests/spmm_order_common.py and sgl_amd/device.py.
// One query per line on stdin, one answer per line on stdout:
//   dtype lanes strict nnz n_rows spmm_group spmm_unroll spmm_waves spmm_nt   ->   group nch U nt waves     (dtype: f32 | bf16)
//   nnz                                                                       ->   item_nnz long_row_nnz
#include <cstdio>
#include <cstring>

#include "../../sgl_amd/csrc/sgl_common.h"

int main() {
    char line[256], dtype[16];
    while (fgets(line, sizeof(line), stdin)) {
        long long lanes, strict, nnz, n_rows, key[4];
        const int got = sscanf(line, "%15s %lld %lld %lld %lld %lld %lld %lld %lld", dtype, &lanes, &strict, &nnz, &n_rows, &key[0],
                               &key[1], &key[2], &key[3]);
        if (got == 1 && sscanf(line, "%lld", &nnz) == 1) {
            printf("%d %d\n", (int)sgl::default_item_nnz(nnz), (int)sgl::default_long_row_nnz(nnz));
            continue;
        }
        const bool bf16 = strcmp(dtype, "bf16") == 0;
        if (got != 9 || (!bf16 && strcmp(dtype, "f32") != 0)) {
            fprintf(stderr, "spmm_layout_table: bad query: %s", line);
            return 2;
        }
        const char *names[4] = {"spmm_group", "spmm_unroll", "spmm_waves", "spmm_nt"};
        for (int k = 0; k < 4; ++k)
            if (sgl_set_tuning(names[k], key[k]) != SGL_OK) return 3;
        const sgl::SpmmLayout L = sgl::spmm_layout((int)lanes, strict != 0, nnz, n_rows, bf16);
        printf("%d %d %d %d %d\n", L.group, L.nch, sgl::unroll_of(L.group, L.nch, L.ulevel), L.nt ? 1 : 0, L.waves);
    }
    return 0;
}
