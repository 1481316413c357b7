/* C ABI of the equivariance entries of libmrfa_hip.so: the reference's equivariance constraint (modules/model.py:231-247) -- one frame warp, the value term and
 * the Jacobian term -- as three launches, with the thin-plate-spline transform and its first and second derivatives in closed form.  Nothing here needs
 * autograd: the backward entry is a first-order computation from the inputs.
 *
 * A second entry group of the model library beside include/mrfa_hip.h: it shares no name with that header, has its own version number (mrfa_equiv_version)
 * and its own binding (mrfa_amd/equiv_hip.py); errors go through the library's one thread-local message, mrfa_last_error() of mrfa_hip.h.  This comment is the
 * specification; tests/ref_equiv.py restates it in numpy fp64, and mrfa_amd/csrc/equiv_math.h is the one text of U, U', U'' and of the six sums over the
 * control points, which the library and a stand-alone host test both compile.
 *
 * ---------------------------------------------------------------------------------------------------------------------------------------------------
 * The transform.  Per sample b: A_b = theta[b,:,:2], t_b = theta[b,:,2]; control points q_k = (qx_k, qy_k), k < P (shared by all samples); weights
 * c_bk = params[b,k]; eps = 1e-6.  For a point p = (x, y):
 *
 *   dx_k = x - qx_k   dy_k = y - qy_k   d_k = |dx_k| + |dy_k|   sx_k = sign(dx_k)   sy_k = sign(dy_k)      sign(0) = 0
 *   U(d)   = d^2 log(d + eps)
 *   U'(d)  = 2 d log(d + eps) + d^2 / (d + eps)
 *   U''(d) = 2 log(d + eps) + 4 d / (d + eps) - d^2 / (d + eps)^2
 *   s   = sum_k c_bk U(d_k)
 *   gx  = sum_k c_bk U'(d_k) sx_k           gy  = sum_k c_bk U'(d_k) sy_k
 *   hxx = sum_k c_bk U''(d_k) sx_k^2        hxy = sum_k c_bk U''(d_k) sx_k sy_k        hyy = sum_k c_bk U''(d_k) sy_k^2
 *   T_b(p)  = A_b p + t_b + (s, s)                     the spline's scalar is added to BOTH coordinates (model.py:50-67)
 *   JT_b(p) = A_b + [[gx, gy], [gx, gy]]               what Transform.jacobian returns
 *
 * Without a spline (P = 0): s = gx = gy = hxx = hxy = hyy = 0.  The sums run in index order k = 0 .. P-1.
 *
 * The loss terms, with N2 = 2 B K, weights w_e, w_j, inv2x2([[a,b],[c,d]]) = [[d,-b],[-c,a]] / (a d - b c):
 *
 *   value = w_e / N2 * sum |kp_d - T(kp_t)|                                            one scalar
 *   M = JT(kp_t) jac_t     V = inv2x2(jac_d) M     term = w_j |I - V|                  (B,K,2,2), un-reduced as model.py:245 keeps it
 *
 * Backward, from the upstream g_value (one scalar on the device) and g_term (B,K,2,2):
 *
 *   r = kp_d - T(kp_t);   d_kp_d = g_value w_e / N2 sign(r);   gT = -d_kp_d
 *   gV = -w_j g_term (.) sign(I - V)
 *   Ji = inv2x2(jac_d);   gM = Ji^T gV;   gJi = gV M^T;   d_jac_d = -Ji^T gJi Ji^T
 *   d_jac_t = JT^T gM;    gJT = gM jac_t^T
 *   ggx = gJT[0,0] + gJT[1,0];   ggy = gJT[0,1] + gJT[1,1]
 *   d_kp_t = JT^T gT + (ggx hxx + ggy hxy,  ggx hxy + ggy hyy)
 *
 * The frame warp: output pixel (i, j) of sample b samples in[b] at T_b(g_ij), g_ij = (2 (j / (W-1)) - 1, 2 (i / (H-1)) - 1) (make_coordinate_grid),
 * bilinear, align_corners=False (pixel coordinate ((g + 1) size - 1) / 2), reflection about the pixel EDGES -0.5 and size - 0.5 followed by a clip to
 * [0, size - 1], a far tap one past the edge has weight 0: F.grid_sample(padding_mode="reflection"), the rules of mrfa_warp_frame_reflect.
 *
 * ---------------------------------------------------------------------------------------------------------------------------------------------------
 * All tensors are contiguous fp32 on the device.  theta (N,2,3); points (P,2); params (N,P); kp_* (B,K,2); jac_*, term, g_term, d_jac_* (B,K,2,2).
 * points and params may be NULL exactly when P = 0.
 * mrfa_equiv_warp_frame: in and out (N,C,H,W).  One launch, one thread per output pixel and all its channels; a workgroup stays inside one sample and holds
 *   that sample's theta, the points and the weights in LDS; no grid tensor, no other intermediate.
 * mrfa_equiv_loss_fwd / _bwd: one launch of ONE workgroup each, a stride loop over the B K points, the control points (and the weights, where B P <=
 *   MRFA_EQUIV_LDS_PARAMS) in LDS; value is a fixed-order reduction.  Backward recomputes everything from the inputs: no state between the two calls.
 *   jac_d, jac_t, term (forward) and jac_d, jac_t, g_term, d_jac_d, d_jac_t (backward) are all NULL together exactly when w_j == 0 (the tpsm configuration
 *   sets equivariance_jacobian: 0); the Jacobian term then does not exist and d_kp_t = JT^T gT.
 * Every output element is written by every call: nothing needs zeroing (graph replay).  No atomics: two runs give the same bits.
 * Each entry returns 0, or nonzero with the message set BEFORE anything is written: a mix of NULL and non-NULL among the Jacobian pointers, or a set that
 * does not match w_j; P < 0 or P > MRFA_EQUIV_MAX_POINTS; H or W < 2 (the grid divides by size - 1); a dimension < 1; N > 65535; any other NULL pointer. */
#ifndef MRFA_EQUIV_HIP_H
#define MRFA_EQUIV_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define MRFA_EQUIV_ABI_VERSION 1
int mrfa_equiv_version(void);

#define MRFA_EQUIV_MAX_POINTS 64           /* control points of the spline (the reference's configurations use 5 x 5) */
#define MRFA_EQUIV_LDS_PARAMS 2048         /* the loss kernels keep params (B,P) in LDS up to this many floats, and read it from global memory beyond */

int mrfa_equiv_warp_frame(void* stream, const float* in_nchw, int N, int C, int H, int W, const float* theta, const float* points, const float* params, int P,
                          float* out_nchw);

int mrfa_equiv_loss_fwd(void* stream, int B, int K, const float* kp_d, const float* jac_d, const float* kp_t, const float* jac_t, const float* theta,
                        const float* points, const float* params, int P, float w_e, float w_j, float* value, float* term);

int mrfa_equiv_loss_bwd(void* stream, int B, int K, const float* kp_d, const float* jac_d, const float* kp_t, const float* jac_t, const float* theta,
                        const float* points, const float* params, int P, float w_e, float w_j, const float* g_value, const float* g_term, float* d_kp_d,
                        float* d_jac_d, float* d_kp_t, float* d_jac_t);

#ifdef __cplusplus
}
#endif
#endif
