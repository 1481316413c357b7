// The thin-plate-spline arithmetic of the equivariance entries (include/mrfa_equiv_hip.h states the formulas): the ONE text of U, U', U'' and of the six sums
// over the control points, compiled by hipcc for the kernels of equivariance.hip and by g++ alone for the host program of tests/test_equiv_math_host.py.
// Plain C++: no HIP type, no intrinsic.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define MRFA_EQ_HD __host__ __device__
#else
#define MRFA_EQ_HD
#endif

#define EQUIV_EPS 1e-6f

// s, its gradient (gx, gy) and its Hessian (hxx, hxy, hyy) at one point
struct EquivSums { float s, gx, gy, hxx, hxy, hyy; };

// U(d) = d^2 log(d + eps) and its first two derivatives, d >= 0; lg = logf(d + eps), de = d + eps, shared by the three
MRFA_EQ_HD inline float equiv_u(float d, float lg) { return d * d * lg; }
MRFA_EQ_HD inline float equiv_du(float d, float lg, float de) { return 2.f * d * lg + d * d / de; }
MRFA_EQ_HD inline float equiv_ddu(float d, float lg, float de) {
    const float q = d / de;
    return 2.f * lg + 4.f * q - q * q;
}

MRFA_EQ_HD inline float equiv_sign(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }

// the six sums at (x, y) over P control points q (x, y interleaved) with weights c, in index order.  A caller that reads only .s (the frame warp) leaves the
// other five to the compiler's dead-code elimination: every sum is its own chain.
MRFA_EQ_HD inline EquivSums equiv_sums(float x, float y, const float* q, const float* c, int P) {
    EquivSums a = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < P; ++k) {
        const float dx = x - q[2 * k], dy = y - q[2 * k + 1];
        const float d = fabsf(dx) + fabsf(dy);
        const float de = d + EQUIV_EPS;
        const float lg = logf(de);
        const float sx = equiv_sign(dx), sy = equiv_sign(dy);
        const float ck = c[k];
        const float c1 = ck * equiv_du(d, lg, de), c2 = ck * equiv_ddu(d, lg, de);
        a.s += ck * equiv_u(d, lg);
        a.gx += c1 * sx;
        a.gy += c1 * sy;
        a.hxx += c2 * (sx * sx);
        a.hxy += c2 * (sx * sy);
        a.hyy += c2 * (sy * sy);
    }
    return a;
}
