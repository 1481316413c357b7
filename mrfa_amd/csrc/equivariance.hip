// The equivariance constraint of the reference's objective (modules/model.py:231-247) as three launches: the frame warp with the sampling position computed in
// registers, and the value + Jacobian terms forward and backward with the thin-plate spline's derivatives in closed form.  include/mrfa_equiv_hip.h is the
// specification, equiv_math.h the one text of the spline sums.
#include "common.h"
#include "equiv_math.h"
#include "mrfa_equiv_hip.h"

namespace {

constexpr int EQ_THREADS = 256;

// torch's reflect_coordinates(v, -1, 2 size - 1) followed by clip_coordinates (the rule of sample.hip's warp_frame_reflect_kernel)
__device__ __forceinline__ float eq_reflect_coord(float v, float size) {
    const float span = size;
    v = fabsf(v + 0.5f);
    const float flips = floorf(v / span);
    const float extra = v - flips * span;
    v = (((int)flips) & 1) ? (span - extra - 0.5f) : (extra - 0.5f);
    return fminf(fmaxf(v, 0.f), size - 1.f);
}

// One thread per output pixel, all channels; blockIdx.y is the sample, so theta[b], the points and params[b] are the same for the whole workgroup: LDS.
// The P logf per pixel are the arithmetic; the taps are those of warp_frame_reflect_kernel.
__global__ void __launch_bounds__(EQ_THREADS) equiv_warp_frame_kernel(const float* __restrict__ in, int C, int H, int W, const float* __restrict__ theta,
                                                                      const float* __restrict__ points, const float* __restrict__ params, int P,
                                                                      float* __restrict__ out) {
    __shared__ float s_theta[6];
    __shared__ float s_q[2 * MRFA_EQUIV_MAX_POINTS];
    __shared__ float s_c[MRFA_EQUIV_MAX_POINTS];
    const int b = blockIdx.y, tid = threadIdx.x;
    if (tid < 6) s_theta[tid] = theta[b * 6 + tid];
    for (int k = tid; k < 2 * P; k += EQ_THREADS) s_q[k] = points[k];
    for (int k = tid; k < P; k += EQ_THREADS) s_c[k] = params[(long long)b * P + k];
    __syncthreads();
    const long long hw = (long long)H * W;
    const long long pix = (long long)blockIdx.x * EQ_THREADS + tid;
    if (pix >= hw) return;
    const int i = (int)(pix / W), j = (int)(pix - (long long)i * W);
    const float gx = 2.f * ((float)j / (float)(W - 1)) - 1.f, gy = 2.f * ((float)i / (float)(H - 1)) - 1.f;      // make_coordinate_grid
    const float s = equiv_sums(gx, gy, s_q, s_c, P).s;
    const float tx = s_theta[0] * gx + s_theta[1] * gy + s_theta[2] + s;
    const float ty = s_theta[3] * gx + s_theta[4] * gy + s_theta[5] + s;
    const float x = eq_reflect_coord(((tx + 1.f) * W - 1.f) * 0.5f, (float)W), y = eq_reflect_coord(((ty + 1.f) * H - 1.f) * 0.5f, (float)H);
    const float x0f = floorf(x), y0f = floorf(y);
    const int x0 = (int)x0f, y0 = (int)y0f, x1 = x0 + 1, y1 = y0 + 1;
    const float wx1 = x - x0f, wy1 = y - y0f, wx0 = 1.f - wx1, wy0 = 1.f - wy1;
    const bool x1ok = x1 < W, y1ok = y1 < H;                         // (after the clip x0, y0 are in range; the far neighbours may be one past the edge: weight 0)
    const float* pin = in + (long long)b * C * hw;
    float* pout = out + (long long)b * C * hw + pix;
    const long long o00 = (long long)y0 * W + x0;
    for (int c = 0; c < C; ++c) {
        const float* pc = pin + (long long)c * hw;
        float v = pc[o00] * wx0 * wy0;
        if (x1ok) v += pc[o00 + 1] * wx1 * wy0;
        if (y1ok) v += pc[o00 + W] * wx0 * wy1;
        if (x1ok && y1ok) v += pc[o00 + W + 1] * wx1 * wy1;
        pout[(long long)c * hw] = v;
    }
}

struct M2 { float a, b, c, d; };                                     // [[a, b], [c, d]]
__device__ __forceinline__ M2 mul(M2 x, M2 y) { return {x.a * y.a + x.b * y.c, x.a * y.b + x.b * y.d, x.c * y.a + x.d * y.c, x.c * y.b + x.d * y.d}; }
__device__ __forceinline__ M2 tr(M2 x) { return {x.a, x.c, x.b, x.d}; }
__device__ __forceinline__ M2 inv2x2(M2 m) {
    const float det = m.a * m.d - m.b * m.c;
    return {m.d / det, -m.b / det, -m.c / det, m.a / det};
}
__device__ __forceinline__ M2 load2x2(const float* p) {
    return {p[0], p[1], p[2], p[3]};
}
__device__ __forceinline__ void store2x2(float* p, M2 m) {
    p[0] = m.a; p[1] = m.b; p[2] = m.c; p[3] = m.d;
}

// what forward and backward share at point i: the spline sums at kp_t[i], T(kp_t[i]) and JT(kp_t[i])
struct EqPoint { EquivSums u; float tx, ty; M2 jt; };

__device__ __forceinline__ EqPoint eq_point(int i, int K, const float* __restrict__ kp_t, const float* __restrict__ theta, const float* q, const float* c_all,
                                            int P) {
    const int b = i / K;
    const float x = kp_t[2 * i], y = kp_t[2 * i + 1];
    const float* th = theta + b * 6;
    EqPoint e;
    e.u = equiv_sums(x, y, q, c_all + (long long)b * P, P);
    e.tx = th[0] * x + th[1] * y + th[2] + e.u.s;
    e.ty = th[3] * x + th[4] * y + th[5] + e.u.s;
    e.jt = {th[0] + e.u.gx, th[1] + e.u.gy, th[3] + e.u.gx, th[4] + e.u.gy};
    return e;
}

// the control points, and params where it fits, into LDS; returns where the kernel reads params from
__device__ __forceinline__ const float* eq_stage(const float* __restrict__ points, const float* __restrict__ params, int B, int P, float* s_q, float* s_c) {
    for (int k = threadIdx.x; k < 2 * P; k += EQ_THREADS) s_q[k] = points[k];
    const bool fits = B * P <= MRFA_EQUIV_LDS_PARAMS;                 // (B P < 2^31: checked on the host side)
    if (fits)
        for (int k = threadIdx.x; k < B * P; k += EQ_THREADS) s_c[k] = params[k];
    __syncthreads();
    return fits ? s_c : params;
}

// One workgroup.  value: every thread sums its points in index order, the wave sums by butterfly, thread 0 adds the four wave sums in order: a fixed order.
__global__ void __launch_bounds__(EQ_THREADS) equiv_loss_fwd_kernel(int B, int K, const float* __restrict__ kp_d, const float* __restrict__ jac_d,
                                                                    const float* __restrict__ kp_t, const float* __restrict__ jac_t,
                                                                    const float* __restrict__ theta, const float* __restrict__ points,
                                                                    const float* __restrict__ params, int P, float w_e, float w_j,
                                                                    float* __restrict__ value, float* __restrict__ term) {
    __shared__ float s_q[2 * MRFA_EQUIV_MAX_POINTS];
    __shared__ float s_c[MRFA_EQUIV_LDS_PARAMS];
    __shared__ float s_part[EQ_THREADS / 64];
    const float* c_all = eq_stage(points, params, B, P, s_q, s_c);
    const int n = B * K;
    float acc = 0.f;
    for (int i = threadIdx.x; i < n; i += EQ_THREADS) {
        const EqPoint e = eq_point(i, K, kp_t, theta, s_q, c_all, P);
        acc += fabsf(kp_d[2 * i] - e.tx) + fabsf(kp_d[2 * i + 1] - e.ty);
        if (term) {
            const M2 v = mul(inv2x2(load2x2(jac_d + 4 * (long long)i)), mul(e.jt, load2x2(jac_t + 4 * (long long)i)));
            store2x2(term + 4 * (long long)i, {w_j * fabsf(1.f - v.a), w_j * fabsf(0.f - v.b), w_j * fabsf(0.f - v.c), w_j * fabsf(1.f - v.d)});
        }
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = s_part[0];
        for (int w = 1; w < EQ_THREADS / 64; ++w) t += s_part[w];
        value[0] = w_e / (float)(2 * n) * t;
    }
}

__global__ void __launch_bounds__(EQ_THREADS) equiv_loss_bwd_kernel(int B, int K, const float* __restrict__ kp_d, const float* __restrict__ jac_d,
                                                                    const float* __restrict__ kp_t, const float* __restrict__ jac_t,
                                                                    const float* __restrict__ theta, const float* __restrict__ points,
                                                                    const float* __restrict__ params, int P, float w_e, float w_j,
                                                                    const float* __restrict__ g_value, const float* __restrict__ g_term,
                                                                    float* __restrict__ d_kp_d, float* __restrict__ d_jac_d, float* __restrict__ d_kp_t,
                                                                    float* __restrict__ d_jac_t) {
    __shared__ float s_q[2 * MRFA_EQUIV_MAX_POINTS];
    __shared__ float s_c[MRFA_EQUIV_LDS_PARAMS];
    const float* c_all = eq_stage(points, params, B, P, s_q, s_c);
    const int n = B * K;
    const float gscale = g_value[0] * (w_e / (float)(2 * n));
    for (int i = threadIdx.x; i < n; i += EQ_THREADS) {
        const EqPoint e = eq_point(i, K, kp_t, theta, s_q, c_all, P);
        const float dkx = gscale * equiv_sign(kp_d[2 * i] - e.tx), dky = gscale * equiv_sign(kp_d[2 * i + 1] - e.ty);
        d_kp_d[2 * i] = dkx;
        d_kp_d[2 * i + 1] = dky;
        const float gtx = -dkx, gty = -dky;
        float dx = e.jt.a * gtx + e.jt.c * gty, dy = e.jt.b * gtx + e.jt.d * gty;                       // JT^T gT
        if (g_term) {
            const M2 jt_in = load2x2(jac_t + 4 * (long long)i), ji = inv2x2(load2x2(jac_d + 4 * (long long)i)), g = load2x2(g_term + 4 * (long long)i);
            const M2 m = mul(e.jt, jt_in), v = mul(ji, m);
            const M2 gv = {-w_j * g.a * equiv_sign(1.f - v.a), -w_j * g.b * equiv_sign(0.f - v.b), -w_j * g.c * equiv_sign(0.f - v.c),
                           -w_j * g.d * equiv_sign(1.f - v.d)};
            const M2 jit = tr(ji);
            const M2 gm = mul(jit, gv), gji = mul(gv, tr(m));
            const M2 dd = mul(jit, mul(gji, jit));
            store2x2(d_jac_d + 4 * (long long)i, {-dd.a, -dd.b, -dd.c, -dd.d});
            store2x2(d_jac_t + 4 * (long long)i, mul(tr(e.jt), gm));
            const M2 gjt = mul(gm, tr(jt_in));
            const float ggx = gjt.a + gjt.c, ggy = gjt.b + gjt.d;
            dx += ggx * e.u.hxx + ggy * e.u.hxy;
            dy += ggx * e.u.hxy + ggy * e.u.hyy;
        }
        d_kp_t[2 * i] = dx;
        d_kp_t[2 * i + 1] = dy;
    }
}

// the checks the two loss entries share; jac_set: how many of the Jacobian pointers are non-NULL out of jac_all
int check_loss_args(const char* name, int B, int K, int P, const void* kp_d, const void* kp_t, const void* theta, const void* points, const void* params,
                    float w_j, int jac_set, int jac_all) {
    MRFA_CHECK_ARG(B >= 1 && K >= 1, "%s: B and K must be >= 1 (B %d, K %d)", name, B, K);
    MRFA_CHECK_ARG((long long)B * K <= 0x3fffffffLL, "%s: B K = %lld points is beyond 2^30 - 1", name, (long long)B * K);
    MRFA_CHECK_ARG(P >= 0 && P <= MRFA_EQUIV_MAX_POINTS, "%s: P must be in [0, %d], not %d", name, MRFA_EQUIV_MAX_POINTS, P);
    MRFA_CHECK_ARG((long long)B * (P > 0 ? P : 1) <= 0x7fffffffLL, "%s: B P is beyond 2^31 - 1", name);
    MRFA_CHECK_ARG(kp_d && kp_t && theta, "%s: null pointer (kp_d, kp_t or theta)", name);
    MRFA_CHECK_ARG(P == 0 || (points && params), "%s: null points or params with P = %d", name, P);
    MRFA_CHECK_ARG(jac_set == 0 || jac_set == jac_all, "%s: the Jacobian pointers are NULL together or not at all (%d of %d are set)", name, jac_set, jac_all);
    MRFA_CHECK_ARG((jac_set != 0) == (w_j != 0.f), "%s: the Jacobian pointers are set exactly when w_j != 0 (w_j %g, %s)", name, (double)w_j,
                   jac_set ? "set" : "NULL");
    return 0;
}

}  // namespace

extern "C" int mrfa_equiv_version(void) { return MRFA_EQUIV_ABI_VERSION; }

extern "C" int mrfa_equiv_warp_frame(void* stream, const float* in, int N, int C, int H, int W, const float* theta, const float* points, const float* params,
                                     int P, float* out) {
    MRFA_CHECK_ARG(N >= 1 && C >= 1, "equiv_warp_frame: N and C must be >= 1 (N %d, C %d)", N, C);
    MRFA_CHECK_ARG(H >= 2 && W >= 2, "equiv_warp_frame: H and W must be >= 2, the grid divides by size - 1 (H %d, W %d)", H, W);
    MRFA_CHECK_ARG(N <= 65535, "equiv_warp_frame: N %d is beyond 65535", N);
    MRFA_CHECK_ARG((long long)H * W <= 0x7fffffffLL, "equiv_warp_frame: H W is beyond 2^31 - 1");
    MRFA_CHECK_ARG(P >= 0 && P <= MRFA_EQUIV_MAX_POINTS, "equiv_warp_frame: P must be in [0, %d], not %d", MRFA_EQUIV_MAX_POINTS, P);
    MRFA_CHECK_ARG(in && theta && out, "equiv_warp_frame: null pointer (in, theta or out)");
    MRFA_CHECK_ARG(P == 0 || (points && params), "equiv_warp_frame: null points or params with P = %d", P);
    const dim3 grid((unsigned)cdiv((long long)H * W, EQ_THREADS), (unsigned)N);
    hipLaunchKernelGGL(equiv_warp_frame_kernel, grid, dim3(EQ_THREADS), 0, (hipStream_t)stream, in, C, H, W, theta, points, params, P, out);
    MRFA_CHECK_LAUNCH("equiv_warp_frame");
    return 0;
}

extern "C" int mrfa_equiv_loss_fwd(void* stream, int B, int K, const float* kp_d, const float* jac_d, const float* kp_t, const float* jac_t, const float* theta,
                                   const float* points, const float* params, int P, float w_e, float w_j, float* value, float* term) {
    const int jac_set = (jac_d != nullptr) + (jac_t != nullptr) + (term != nullptr);
    if (int rc = check_loss_args("equiv_loss_fwd", B, K, P, kp_d, kp_t, theta, points, params, w_j, jac_set, 3))
        return rc;
    MRFA_CHECK_ARG(value, "equiv_loss_fwd: null value");
    hipLaunchKernelGGL(equiv_loss_fwd_kernel, dim3(1), dim3(EQ_THREADS), 0, (hipStream_t)stream, B, K, kp_d, jac_d, kp_t, jac_t, theta, points, params, P, w_e,
                       w_j, value, term);
    MRFA_CHECK_LAUNCH("equiv_loss_fwd");
    return 0;
}

extern "C" int mrfa_equiv_loss_bwd(void* stream, int B, int K, const float* kp_d, const float* jac_d, const float* kp_t, const float* jac_t, const float* theta,
                                   const float* points, const float* params, int P, float w_e, float w_j, const float* g_value, const float* g_term,
                                   float* d_kp_d, float* d_jac_d, float* d_kp_t, float* d_jac_t) {
    const int jac_set = (jac_d != nullptr) + (jac_t != nullptr) + (g_term != nullptr) + (d_jac_d != nullptr) + (d_jac_t != nullptr);
    if (int rc = check_loss_args("equiv_loss_bwd", B, K, P, kp_d, kp_t, theta, points, params, w_j, jac_set, 5))
        return rc;
    MRFA_CHECK_ARG(g_value && d_kp_d && d_kp_t, "equiv_loss_bwd: null pointer (g_value, d_kp_d or d_kp_t)");
    hipLaunchKernelGGL(equiv_loss_bwd_kernel, dim3(1), dim3(EQ_THREADS), 0, (hipStream_t)stream, B, K, kp_d, jac_d, kp_t, jac_t, theta, points, params, P, w_e,
                       w_j, g_value, g_term, d_kp_d, d_jac_d, d_kp_t, d_jac_t);
    MRFA_CHECK_LAUNCH("equiv_loss_bwd");
    return 0;
}
