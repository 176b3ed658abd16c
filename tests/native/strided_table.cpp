// The host arithmetic behind the strided launches as the library computes it, without a GPU: sgl::pick_lpr, sgl::slice_instance
// (sgl_amd/csrc/sgl_core.cpp) over each family's lists and sgl::loss_grid (sgl_common.h) under the tuning key loss_blocks, built by tests/test_strided_cpu.py
// with g++ and compared there against the restatements of tests/strided_common.py.
// One query per line on stdin, one answer per line on stdout:
//   lpr d vec                     ->   lanes per row
//   km / el / cl / cls w vec      ->   lpr ch                 (the rule of K9 / K11 / K12 / K14; ch = 0: beyond the register layouts)
//   grid wanted cap loss_blocks   ->   blocks                 (sets the key first and reads it back)
#include <cstdio>
#include <cstring>

#include "../../sgl_amd/csrc/sgl_common.h"

int main() {
    char line[256], what[16];
    while (fgets(line, sizeof(line), stdin)) {
        long long a, b, c = 0;
        const int got = sscanf(line, "%15s %lld %lld %lld", what, &a, &b, &c);
        if (got >= 3 && !strcmp(what, "lpr")) {
            printf("%d\n", sgl::pick_lpr(a, (int)b));
        } else if (got >= 3 && (!strcmp(what, "km") || !strcmp(what, "el") || !strcmp(what, "cl") || !strcmp(what, "cls"))) {
            const int vec = (int)b;
            const sgl::ChunkList compiled = !strcmp(what, "km")   ? sgl::KmeansSlices::chunks(vec)
                                            : !strcmp(what, "el") ? sgl::EdgeLossSlices::chunks(vec)
                                            : !strcmp(what, "cl") ? sgl::ClusterLossSlices::chunks(vec)
                                                                  : sgl::ClassLossSlices::chunks(vec);
            const sgl::SliceInstance in = sgl::slice_instance(a, vec, compiled);
            printf("%d %d\n", in.lpr, in.ch);
        } else if (got == 4 && !strcmp(what, "grid")) {
            int64_t back = -1;
            if (sgl_set_tuning("loss_blocks", c) != SGL_OK || sgl_get_tuning("loss_blocks", &back) != SGL_OK || back != c) return 3;
            printf("%lld\n", (long long)sgl::loss_grid(a, b));
        } else {
            fprintf(stderr, "strided_table: bad query: %s", line);
            return 2;
        }
    }
    return 0;
}
