// The per-pixel arithmetic of the colour jitter (include/mrfa_data_hip.h states the rules): written ONCE, compiled by hipcc for the kernels of augment.hip
// and by g++ alone for the host program of tests/test_augment_math_host.py, which evaluates every primitive on all 2^24 inputs against tests/ref_augment.py.
// Every rule is a sequence of individually rounded operations: compile with -ffp-contract=off and without fast-math on both sides (the pragma below says
// the same to clang, whatever the command line).  Plain C++: no HIP type, no intrinsic.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define MRFA_HD __host__ __device__
#else
#define MRFA_HD
#endif
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

// op codes (MRFA_AUG_* of include/mrfa_data_hip.h)
enum { AUG_NONE = 0, AUG_BRIGHTNESS = 1, AUG_CONTRAST = 2, AUG_SATURATION = 3, AUG_HUE = 4, AUG_OPS = 4 };

struct AugRgb { unsigned r, g, b; };      // three bytes, each in [0, 255]

MRFA_HD inline unsigned aug_clamp_int(int v) { return v < 0 ? 0u : v > 255 ? 255u : (unsigned)v; }

MRFA_HD inline unsigned aug_luma(unsigned r, unsigned g, unsigned b) { return (19595u * r + 38470u * g + 7471u * b + 0x8000u) >> 16; }

// t = f32(d) + f (f32(x) - f32(d)), truncated and clamped.  f is finite and >= 0, so t is finite: |t| <= 255 (1 + f).
MRFA_HD inline unsigned aug_blend(unsigned d, unsigned x, float f) {
    const float fd = (float)d;
    const float diff = (float)x - fd;      // exact
    const float prod = f * diff;
    const float t = fd + prod;
    return t >= 255.f ? 255u : t > 0.f ? (unsigned)(int)t : 0u;
}

MRFA_HD inline AugRgb aug_blend3(unsigned d, AugRgb c, float f) {
    AugRgb o;
    o.r = aug_blend(d, c.r, f);
    o.g = aug_blend(d, c.g, f);
    o.b = aug_blend(d, c.b, f);
    return o;
}

// (r, g, b) -> (H, S, V) in the fields (r, g, b)
MRFA_HD inline AugRgb aug_rgb_to_hsv(AugRgb c) {
    const unsigned mx = c.r > c.g ? (c.r > c.b ? c.r : c.b) : (c.g > c.b ? c.g : c.b);
    const unsigned mn = c.r < c.g ? (c.r < c.b ? c.r : c.b) : (c.g < c.b ? c.g : c.b);
    AugRgb o;
    o.b = mx;
    if (mx == mn) {
        o.r = o.g = 0;
        return o;
    }
    const float cr = (float)(mx - mn);
    const float sat = cr / (float)mx;
    const float rc = (float)(mx - c.r) / cr, gc = (float)(mx - c.g) / cr, bc = (float)(mx - c.b) / cr;
    float h;
    if (c.r == mx) {
        h = bc - gc;
    } else if (c.g == mx) {
        const double s = 2.0 + (double)rc;
        h = (float)(s - (double)bc);
    } else {
        const double s = 4.0 + (double)gc;
        h = (float)(s - (double)rc);
    }
    const double x = (double)h / 6.0 + 1.0;            // in [5/6, 11/6]: fmod(x, 1.0) is x - floor(x), exactly
    const float hm = (float)(x - floor(x));
    o.r = aug_clamp_int((int)((double)hm * 255.0));
    o.g = aug_clamp_int((int)((double)sat * 255.0));
    return o;
}

// C round() for v >= 0 (halves away from zero), as an integer: floor(v) and the fraction, which is exact
MRFA_HD inline unsigned aug_round_byte(double v) {
    const double fl = floor(v);
    const int i = (int)fl + (v - fl >= 0.5 ? 1 : 0);
    return aug_clamp_int(i);
}

// (H, S, V) in the fields (r, g, b) -> (r, g, b)
MRFA_HD inline AugRgb aug_hsv_to_rgb(AugRgb c) {
    const unsigned H = c.r, S = c.g, V = c.b;
    AugRgb o;
    if (S == 0) {
        o.r = o.g = o.b = V;
        return o;
    }
    const double hf = (double)(float)H * 6.0 / 255.0;
    const double fi = floor(hf);
    const double f = (double)(float)(hf - fi);
    const double fs = (double)(float)((double)(float)S / 255.0);
    const double v = (double)V;
    const unsigned p = aug_round_byte(v * (1.0 - fs));
    const unsigned q = aug_round_byte(v * (1.0 - fs * f));
    const unsigned t = aug_round_byte(v * (1.0 - fs * (1.0 - f)));
    switch ((int)fi % 6) {
        case 0: o.r = V; o.g = t; o.b = p; break;
        case 1: o.r = q; o.g = V; o.b = p; break;
        case 2: o.r = p; o.g = V; o.b = t; break;
        case 3: o.r = p; o.g = q; o.b = V; break;
        case 4: o.r = t; o.g = p; o.b = V; break;
        default: o.r = V; o.g = p; o.b = q; break;
    }
    return o;
}

MRFA_HD inline AugRgb aug_hue(AugRgb c, unsigned shift) {
    AugRgb hsv = aug_rgb_to_hsv(c);
    hsv.r = (hsv.r + shift) & 255u;
    return aug_hsv_to_rgb(hsv);
}

// One pair's op chain on one pixel.  factor[op - 1] for the three blends; `mean` is the frame's contrast mean.  until_contrast: stop BEFORE the contrast
// op (the luma-sum pass: the pixel as contrast will find it).  AUG_NONE entries are skipped.
MRFA_HD inline AugRgb aug_chain(AugRgb c, const unsigned char* op, const float* factor, unsigned hue_shift, unsigned mean, bool until_contrast) {
    for (int k = 0; k < AUG_OPS; ++k) {
        const int o = op[k];
        if (o == AUG_BRIGHTNESS) {
            c = aug_blend3(0u, c, factor[0]);
        } else if (o == AUG_CONTRAST) {
            if (until_contrast) return c;
            c = aug_blend3(mean, c, factor[1]);
        } else if (o == AUG_SATURATION) {
            c = aug_blend3(aug_luma(c.r, c.g, c.b), c, factor[2]);
        } else if (o == AUG_HUE) {
            c = aug_hue(c, hue_shift);
        }
    }
    return c;
}

// m = int(mean(L) + 0.5) from the integer sum S over n pixels
MRFA_HD inline unsigned aug_contrast_mean(unsigned long long S, unsigned long long n) { return (unsigned)((2ull * S + n) / (2ull * n)); }
