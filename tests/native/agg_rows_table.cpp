// The row rule of the register-resident aggregator kernels as the library computes it, without a GPU: sgl::row_instance and
// sgl::out_cols of sgl_amd/csrc/sgl_core.cpp, built by tests/test_agg_rows_cpu.py with g++ and compared there against the
// restatements of tests/agg_rows_common.py.
// One query per line on stdin, one answer per line on stdout:
//   d n_hops allow_8x5 pad row_lpr32x2 row_narrow_groups row_whole_lines   ->   lpr ch hmax out_cols
// (hmax = 0: the layout has no compiled instance for n_hops; out_cols for `pad` declared columns and the layout's room)
#include <cstdio>

#include "../../sgl_amd/csrc/sgl_common.h"

int main() {
    char line[256];
    while (fgets(line, sizeof(line), stdin)) {
        long long d, n_hops, allow, pad, key[3];
        if (sscanf(line, "%lld %lld %lld %lld %lld %lld %lld", &d, &n_hops, &allow, &pad, &key[0], &key[1], &key[2]) != 7) {
            fprintf(stderr, "agg_rows_table: bad query: %s", line);
            return 2;
        }
        const char *names[3] = {"row_lpr32x2", "row_narrow_groups", "row_whole_lines"};
        for (int k = 0; k < 3; ++k)
            if (sgl_set_tuning(names[k], key[k]) != SGL_OK) return 3;
        const sgl::RowInstance in = sgl::row_instance(d, (int)n_hops, allow != 0);
        const sgl::RowLayout lay = sgl::row_layout(d, (int)n_hops, allow != 0);
        if (lay.lpr != in.lpr || lay.ch != in.ch) return 4;
        printf("%d %d %d %d\n", in.lpr, in.ch, in.hmax, sgl::out_cols(d, pad, (long long)in.lpr * in.ch * 4));
    }
    return 0;
}
