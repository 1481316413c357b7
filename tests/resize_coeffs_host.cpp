// Host program of tests/test_resize_coeffs_host.py: mrfa_amd/csrc_data/resize_coeffs.h -- the text the data library compiles -- built by g++ alone.
// Arguments: groups of five, `in_size in0 in1 out_size filter` (in0, in1 as %.9g: they read back as the same float32).  Per group one line:
// ksize, then the 2 out_size bounds, then the out_size * ksize coefficients.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "resize_coeffs.h"

int main(int argc, char** argv) {
    if ((argc - 1) % 5 != 0) {
        fprintf(stderr, "usage: %s (in_size in0 in1 out_size filter)...\n", argv[0]);
        return 2;
    }
    for (int a = 1; a + 4 < argc; a += 5) {
        const int in_size = atoi(argv[a]), out_size = atoi(argv[a + 3]), filter = atoi(argv[a + 4]);
        const float in0 = strtof(argv[a + 1], nullptr), in1 = strtof(argv[a + 2], nullptr);
        if (in_size < 1 || out_size < 1 || !mrfa_resize::filter_known(filter) || !mrfa_resize::box_ok(in_size, in0, in1)) {
            printf("refused\n");
            continue;
        }
        const double kd = mrfa_resize::axis_of(in0, in1, out_size, filter).ksize;
        if (kd > 4096.0) {
            printf("refused\n");
            continue;
        }
        const int ksize = (int)kd;
        std::vector<int> bounds(2 * (size_t)out_size), kk((size_t)out_size * ksize);
        std::vector<double> w((size_t)ksize);
        mrfa_resize::coeffs(in_size, in0, in1, out_size, filter, ksize, bounds.data(), kk.data(), w.data());
        printf("%d", ksize);
        for (int v : bounds) printf(" %d", v);
        for (int v : kk) printf(" %d", v);
        printf("\n");
    }
    return 0;
}
