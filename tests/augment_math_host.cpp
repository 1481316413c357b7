// Host program of tests/test_augment_math_host.py: mrfa_amd/csrc_data/augment_math.h -- the text the device kernels compile -- built by g++ alone, every
// primitive evaluated on all 2^24 inputs.  Prints one line per (primitive, parameter): name, parameter, sum of the packed outputs, and the sum weighted by
// input index + 1, both modulo 2^64.  The test forms the same sums from tests/ref_augment.py.
#include <initializer_list>
#include <stdint.h>
#include <stdio.h>

#include "augment_math.h"

static const float FACTORS[] = {0.0f, 0.9f, 1.0f, 1.1f, 2.0f, 0.9428090f, 1.0471976f};
static const unsigned SHIFTS[] = {1, 25, 231, 128};
static const unsigned MEANS[] = {10, 117};

static inline uint64_t pack(AugRgb c) { return (uint64_t)c.r << 16 | (uint64_t)c.g << 8 | c.b; }

template <class F>
static void run(const char* name, double param, F fn) {
    uint64_t sum = 0, wsum = 0;
    for (uint32_t v = 0; v < (1u << 24); ++v) {
        AugRgb c;
        c.r = v >> 16, c.g = (v >> 8) & 255u, c.b = v & 255u;
        const uint64_t o = fn(c);
        sum += o;
        wsum += o * ((uint64_t)v + 1);
    }
    printf("%s %.9g %llu %llu\n", name, param, (unsigned long long)sum, (unsigned long long)wsum);
}

int main() {
    run("luma", 0, [](AugRgb c) { return (uint64_t)aug_luma(c.r, c.g, c.b); });
    for (float f : FACTORS) {
        run("brightness", f, [f](AugRgb c) { return pack(aug_blend3(0u, c, f)); });
        run("saturation", f, [f](AugRgb c) { return pack(aug_blend3(aug_luma(c.r, c.g, c.b), c, f)); });
        for (unsigned m : MEANS) {
            char name[32];
            snprintf(name, sizeof name, "contrast@%u", m);
            run(name, f, [f, m](AugRgb c) { return pack(aug_blend3(m, c, f)); });
        }
    }
    run("rgb_to_hsv", 0, [](AugRgb c) { return pack(aug_rgb_to_hsv(c)); });
    run("hsv_to_rgb", 0, [](AugRgb c) { return pack(aug_hsv_to_rgb(c)); });
    for (unsigned s : SHIFTS) run("hue", s, [s](AugRgb c) { return pack(aug_hue(c, s)); });
    // the chain as the kernels call it: every op, a fixed mean; and the prefix the luma-sum pass takes
    const unsigned char order[4] = {AUG_SATURATION, AUG_HUE, AUG_CONTRAST, AUG_BRIGHTNESS};
    const float factor[3] = {1.07f, 0.93f, 1.05f};
    run("chain", 0, [&](AugRgb c) { return pack(aug_chain(c, order, factor, 231u, 117u, false)); });
    run("chain_prefix", 0, [&](AugRgb c) { return pack(aug_chain(c, order, factor, 231u, 117u, true)); });
    for (unsigned long long n : {1ull, 2ull, 3ull, 35ull, 65536ull})
        for (unsigned long long S : {0ull, 1ull, 10ull, 21ull, 52ull, 53ull, 8355840ull, 16711680ull})
            if (S <= 255 * n) printf("mean %llu/%llu %u 0\n", S, n, aug_contrast_mean(S, n));
    return 0;
}
