// mrfa_amd/csrc/equiv_math.h compiled by g++ alone (tests/test_equiv_math_host.py).  Reads from stdin, every float as a C hexadecimal literal:
//   P, then P lines "qx qy c";  n, then n lines "x y";  m, then m lines "d"
// and prints n lines "s gx gy hxx hxy hyy" followed by m lines "U U' U''", again as hexadecimal floats (exact both ways).
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "equiv_math.h"

static float read_float() {
    char buf[64];
    if (scanf("%63s", buf) != 1) exit(2);
    return strtof(buf, nullptr);
}

static int read_int() {
    int v;
    if (scanf("%d", &v) != 1 || v < 0 || v > (1 << 20)) exit(2);
    return v;
}

int main() {
    const int P = read_int();
    std::vector<float> q(2 * (size_t)P + 1), c((size_t)P + 1);
    for (int k = 0; k < P; ++k) {
        q[2 * k] = read_float();
        q[2 * k + 1] = read_float();
        c[k] = read_float();
    }
    const int n = read_int();
    for (int i = 0; i < n; ++i) {
        const float x = read_float(), y = read_float();
        const EquivSums a = equiv_sums(x, y, q.data(), c.data(), P);
        printf("%a %a %a %a %a %a\n", (double)a.s, (double)a.gx, (double)a.gy, (double)a.hxx, (double)a.hxy, (double)a.hyy);
    }
    const int m = read_int();
    for (int i = 0; i < m; ++i) {
        const float d = read_float(), de = d + EQUIV_EPS, lg = logf(de);
        printf("%a %a %a\n", (double)equiv_u(d, lg), (double)equiv_du(d, lg, de), (double)equiv_ddu(d, lg, de));
    }
    return 0;
}
