// kp_pose_dist: the pose distance of driving frames to their source from the model's keypoints, with a running argmin over a clip kept on the device
// (demo.py:75-98, find_best_frame, with the 68 face landmarks replaced by the K keypoints).  Entry: include/mrfa_hip.h.  Inference only.
//
// One workgroup of ONE wave per source; lane l takes frames l, l + 64, ... of that source, one whole frame per lane: K <= 64 points are a few hundred
// operations, the point of the kernel is that a clip's search is one launch per group of frames and one host read at its end.  Per frame, in this order
// (tests/test_best_frame_gpu.py counts the roundings):
//   c = (sum_k p_k) / K;  q_k = p_k - c;  A = hull area of q;  n_k = q_k / sqrt(A);  dist = sum_k (n_k.x - m_k.x)^2 + (n_k.y - m_k.y)^2, m = the source's n.
// Hull: Andrew's monotone chain on the centred points -- an index sort by (x, y), a lower and an upper chain that pop while the turn is not strictly
// counter-clockwise (cross <= 0: collinear and duplicate points never stay on a chain), the shoelace sum over the chains' edges.  Every operation of the
// turn test and of the shoelace terms is rounded on its own (no contraction into fused operations), so an edge walked in both directions (all points on one
// line) cancels exactly.  Every loop is bounded by K whatever the data holds (NaN included): chain and sort indices stay inside [0, K).
// LDS, [k][lane] so that lanes at the same k hit different banks: the centred points (32 KiB) and the two byte index arrays (4 KiB each).
// No atomics, no cross-lane sums: bit-identical run to run.
#include <limits.h>

#include "common.h"
#include "mrfa_hip.h"

namespace {

constexpr int NT = 64;                     // one wave
constexpr int MAXK = 64;

struct PoseState {
    float best_dist;
    int best_index, frames_seen, pad;
};

struct PoseLds {
    float2 q[MAXK * NT];
    unsigned char ord[MAXK * NT], stk[MAXK * NT];
};

__device__ __forceinline__ bool finite2(float2 v) { return isfinite(v.x) && isfinite(v.y); }

// centres the K points at p into L.q (this lane's column) and returns the area of their convex hull; c: the centre, fin: every coordinate was finite
__device__ float centre_hull(const float2* __restrict__ p, int K, int lane, PoseLds& L, float2& c, bool& fin) {
#pragma clang fp contract(off)
    float sx = 0.f, sy = 0.f;
    fin = true;
    for (int k = 0; k < K; ++k) {
        const float2 v = p[k];
        sx += v.x;
        sy += v.y;
        fin = fin && finite2(v);
    }
    c = make_float2(sx / (float)K, sy / (float)K);
    // insertion sort of the indices by (x, y); a NaN compares false and travels to the front
    for (int i = 0; i < K; ++i) {
        const float2 r = p[i];
        const float2 v = make_float2(r.x - c.x, r.y - c.y);
        L.q[i * NT + lane] = v;
        int j = i;
        while (j > 0) {
            const int o = L.ord[(j - 1) * NT + lane];
            const float2 w = L.q[o * NT + lane];
            if (w.x < v.x || (w.x == v.x && w.y <= v.y)) break;
            L.ord[j * NT + lane] = (unsigned char)o;
            --j;
        }
        L.ord[j * NT + lane] = (unsigned char)i;
    }
    float acc = 0.f;
    for (int pass = 0; pass < 2; ++pass) {                                  // lower chain left to right, upper chain right to left: counter-clockwise
        int h = 0;
        for (int t = 0; t < K; ++t) {
            const int i = L.ord[(pass ? K - 1 - t : t) * NT + lane];
            const float2 v = L.q[i * NT + lane];
            while (h >= 2) {
                const float2 o = L.q[L.stk[(h - 2) * NT + lane] * NT + lane], a = L.q[L.stk[(h - 1) * NT + lane] * NT + lane];
                const float turn = (a.x - o.x) * (v.y - o.y) - (a.y - o.y) * (v.x - o.x);
                if (!(turn <= 0.f)) break;
                --h;
            }
            L.stk[h * NT + lane] = (unsigned char)i;                        // h <= t < K
            ++h;
        }
        for (int t = 0; t + 1 < h; ++t) {
            const float2 a = L.q[L.stk[t * NT + lane] * NT + lane], b = L.q[L.stk[(t + 1) * NT + lane] * NT + lane];
            acc += a.x * b.y - b.x * a.y;
        }
    }
    return 0.5f * acc;
}

__global__ __launch_bounds__(NT) void kp_pose_dist_kernel(const float2* __restrict__ kd, const float2* __restrict__ ks, int rep, int K,
                                                          float* __restrict__ dist_out, float* __restrict__ area_out, PoseState* __restrict__ state) {
    __shared__ PoseLds L;
    const int s = blockIdx.x, lane = threadIdx.x;
    const float2* ps = ks + (size_t)s * K;
    float2 cs;
    bool fin_s;
    const float As = centre_hull(ps, K, lane, L, cs, fin_s);               // every lane computes its source's centre and area: the same numbers in each
    const bool ok_s = fin_s && isfinite(As) && As > 0.f;
    const float rs = sqrtf(As);
    float best = INFINITY;
    int best_j = INT_MAX;
    for (int j = lane; j < rep; j += NT) {
        const size_t n = (size_t)s * rep + j;
        float2 cd;
        bool fin_d;
        const float Ad = centre_hull(kd + n * K, K, lane, L, cd, fin_d);   // leaves the frame's centred points in L.q
        float dist = INFINITY;
        if (ok_s && fin_d && isfinite(Ad) && Ad > 0.f) {
            const float rd = sqrtf(Ad);
            float acc = 0.f;
            for (int k = 0; k < K; ++k) {
                const float2 a = L.q[k * NT + lane], v = ps[k];
                const float dx = a.x / rd - (v.x - cs.x) / rs, dy = a.y / rd - (v.y - cs.y) / rs;
                acc += dx * dx;
                acc += dy * dy;
            }
            dist = isfinite(acc) ? acc : INFINITY;                          // (an extent so large that n overflows: inf - inf must not reach the output as NaN)
        }
        if (dist_out) dist_out[n] = dist;
        if (area_out) area_out[n] = Ad;
        if (dist < best) {                                                  // ascending j: the earliest of equal distances stays; NaN and +inf never enter
            best = dist;
            best_j = j;
        }
    }
    if (!state) return;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float d2 = __shfl_xor(best, o, 64);
        const int j2 = __shfl_xor(best_j, o, 64);
        if (d2 < best || (d2 == best && j2 < best_j)) {
            best = d2;
            best_j = j2;
        }
    }
    if (lane == 0) {
        PoseState st = state[s];
        if (best < st.best_dist) {
            st.best_dist = best;
            st.best_index = st.frames_seen + best_j;
        }
        st.frames_seen += rep;
        state[s].best_dist = st.best_dist;
        state[s].best_index = st.best_index;
        state[s].frames_seen = st.frames_seen;
    }
}

}  // namespace

extern "C" int mrfa_kp_pose_dist(void* stream, const float* kp_d, const float* kp_s, int B, int rep, int K, float* dist_out, float* area_out, void* state) {
    MRFA_CHECK_ARG(kp_d && kp_s, "kp_pose_dist: null keypoint pointer");
    MRFA_CHECK_ARG(dist_out || area_out || state, "kp_pose_dist: dist_out, area_out and state are all null (nothing to compute)");
    MRFA_CHECK_ARG(B >= 1 && rep >= 1 && K >= 1, "kp_pose_dist: B, rep and K must be >= 1 (B %d, rep %d, K %d)", B, rep, K);
    MRFA_CHECK_ARG(B % rep == 0, "kp_pose_dist: rep must divide B (B %d, rep %d)", B, rep);
    MRFA_CHECK_ARG(K >= 3 && K <= MAXK, "kp_pose_dist: a hull needs 3 <= K <= %d keypoints (K %d)", MAXK, K);
    const uintptr_t a8 = (uintptr_t)kp_d | (uintptr_t)kp_s, a4 = (uintptr_t)dist_out | (uintptr_t)area_out | (uintptr_t)state;
    MRFA_CHECK_ARG((a8 & 7u) == 0 && (a4 & 3u) == 0, "kp_pose_dist: keypoints must be 8-byte aligned (vector loads), the outputs and the state 4-byte aligned");
    hipLaunchKernelGGL(kp_pose_dist_kernel, dim3(B / rep), dim3(NT), 0, (hipStream_t)stream, (const float2*)kp_d, (const float2*)kp_s, rep, K, dist_out,
                       area_out, (PoseState*)state);
    MRFA_CHECK_LAUNCH("mrfa_kp_pose_dist");
    return 0;
}
