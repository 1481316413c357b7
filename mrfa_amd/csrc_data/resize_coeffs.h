// The coefficient rules of the resize entries (include/mrfa_resize_hip.h, whose comment is the specification): Pillow's precompute_coeffs and
// normalize_coeffs_8bpc for one axis, in ONE text.  Plain C++17, no HIP: the data library compiles it on the host side (with -ffp-contract=off, like every
// file of csrc_data/) and tests/resize_coeffs_host.cpp compiles it with g++ alone.  libm's sin / cos, as Pillow's build uses them.
#ifndef MRFA_RESIZE_COEFFS_H
#define MRFA_RESIZE_COEFFS_H

#include <math.h>

namespace mrfa_resize {

constexpr int FILTER_BOX = 0, FILTER_BILINEAR = 1, FILTER_HAMMING = 2, FILTER_BICUBIC = 3, FILTER_LANCZOS = 4;
constexpr int PRECISION_BITS = 22;                       // coefficients are fixed point with 22 fractional bits
constexpr double PI = 3.14159265358979323846;            // M_PI

inline bool filter_known(int filter) { return filter >= FILTER_BOX && filter <= FILTER_LANCZOS; }

inline double filter_support(int filter) {
    switch (filter) {
        case FILTER_BOX: return 0.5;
        case FILTER_BILINEAR: return 1.0;
        case FILTER_HAMMING: return 1.0;
        case FILTER_BICUBIC: return 2.0;
        default: return 3.0;
    }
}

inline double sinc(double x) {
    if (x == 0.0) return 1.0;
    x = x * PI;
    return sin(x) / x;
}

inline double filter_value(int filter, double x) {
    switch (filter) {
        case FILTER_BOX:
            return x > -0.5 && x <= 0.5 ? 1.0 : 0.0;
        case FILTER_BILINEAR:
            if (x < 0.0) x = -x;
            return x < 1.0 ? 1.0 - x : 0.0;
        case FILTER_HAMMING:
            if (x < 0.0) x = -x;
            if (x == 0.0) return 1.0;
            if (x >= 1.0) return 0.0;
            x = x * PI;
            return sin(x) / x * (0.54 + 0.46 * cos(x));
        case FILTER_BICUBIC: {
            const double a = -0.5;
            if (x < 0.0) x = -x;
            if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
            if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
            return 0.0;
        }
        default:
            return -3.0 <= x && x < 3.0 ? sinc(x) * sinc(x / 3) : 0.0;
    }
}

// the box of one axis, as the entries take it: both ends are float32 already; it lies in [0, in_size] and in1 - in0, formed in float32, is > 0
inline bool box_ok(int in_size, float in0, float in1) {
    return isfinite(in0) && isfinite(in1) && in0 >= 0.f && in1 <= (float)in_size && in1 - in0 > 0.f;
}

struct Axis {
    double in0, scale, support, ss;
    double ksize;                                        // 2 ceil(support) + 1 as a double: the caller holds it against its cap BEFORE it becomes an int
};

inline Axis axis_of(float in0, float in1, int out_size, int filter) {
    Axis a;
    const float d = in1 - in0;                           // formed in float32
    a.in0 = (double)in0;
    a.scale = (double)d / out_size;
    const double fscale = a.scale < 1.0 ? 1.0 : a.scale;
    a.support = filter_support(filter) * fscale;
    a.ksize = 2.0 * ceil(a.support) + 1.0;
    a.ss = 1.0 / fscale;
    return a;
}

// bounds: out_size rows (xmin, cnt); kk: out_size rows of ksize coefficients, entries past cnt are 0.  ksize == (int)axis_of(...).ksize.
// w is scratch of ksize doubles.
inline void coeffs(int in_size, float in0, float in1, int out_size, int filter, int ksize, int* bounds, int* kk, double* w) {
    const Axis a = axis_of(in0, in1, out_size, filter);
    for (int xx = 0; xx < out_size; ++xx) {
        const double center = a.in0 + (xx + 0.5) * a.scale;
        int xmin = (int)(center - a.support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + a.support + 0.5);
        if (xmax > in_size) xmax = in_size;
        int cnt = xmax - xmin;
        if (cnt < 0) cnt = 0;
        if (cnt > ksize) cnt = ksize;                    // (never taken: cnt <= 2 support + 1 <= ksize; it keeps a row inside its ksize slots whatever rounding does)
        double ww = 0.0;
        for (int x = 0; x < cnt; ++x) {
            w[x] = filter_value(filter, (x + xmin - center + 0.5) * a.ss);
            ww += w[x];
        }
        int* k = kk + (long long)xx * ksize;
        for (int x = 0; x < cnt; ++x) {
            const double v = ww != 0.0 ? w[x] / ww : w[x];
            k[x] = (int)(v * 4194304.0 + (v < 0 ? -0.5 : 0.5));
        }
        for (int x = cnt; x < ksize; ++x) k[x] = 0;
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = cnt;
    }
}

}  // namespace mrfa_resize
#endif
