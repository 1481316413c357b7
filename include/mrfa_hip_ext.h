/* libmrfa_hip.so: entries whose CPU specification lives beside their tests (tests/emu_ext.py), not in the ABI emulator.
 *
 * include/mrfa_hip.h is one table with the ctypes binding (mrfa_amd/hip.py: _SIGNATURES) and the emulator: an entry declared there has to appear in
 * all three at once.  An entry declared HERE is bound from the binding's second table (hip._EXT_SIGNATURES), looked up with hip.has() by its one caller,
 * and specified by tests/emu_ext.py::ExtEmulator.  The ABI version of mrfa_hip.h does not move for it: a library without the entry loads, and the caller
 * says that the library has to be rebuilt.
 */
#ifndef MRFA_HIP_EXT_H
#define MRFA_HIP_EXT_H

#ifdef __cplusplus
extern "C" {
#endif

/* Pose distance of driving frames to their source from keypoints, and a running argmin over a clip (demo.py:75-98, find_best_frame, on the model's own
 * keypoints instead of face landmarks).  Inference only.
 *
 *   kp_d (B,K,2), kp_s (B/rep,K,2): frame n belongs to source n / rep.  For a point set p of K points, in this order:
 *     c = mean_k p_k;  q_k = p_k - c;  A = area of the convex hull of q;  n_k = q_k / sqrt(A)
 *     dist(frame) = sum_k |n_k(frame) - n_k(source)|^2   (both coordinates)
 *   The hull is a monotone chain: collinear and duplicate points do not count twice, the area is a continuous function of the points.
 *   dist_out (B), area_out (B): nullable; area_out[n] = A of frame n.  If A <= 0, or A or an input of the frame is not finite, dist = +inf (the area is
 *   written as computed); a degenerate source gives +inf to all of its frames.  dist_out is a finite number or +inf, never NaN: finite inputs so extreme that
 *   the normalised points overflow give +inf as well.
 *   All of this is fp32 arithmetic on the CENTRED points: a set that is exactly collinear as given but whose mean is not representable is collinear only up
 *   to the rounding of the centring, and may come out with a tiny positive area and a finite, meaningless distance instead of 0 and +inf (the area is a
 *   continuous function of the points, not a classifier of degeneracy).
 *   state: nullable, B/rep entries of 16 bytes {float best_dist; int best_index; int frames_seen; int pad}.  Frame j (0-based within the call) of a source
 *   has clip index frames_seen + j; the best entry is replaced only by a strictly smaller finite distance (ties keep the earliest frame, NaN and +inf never
 *   win); then frames_seen += rep.  A fresh state is {+inf, 0, 0, 0}.  The frame offset lives on the device: a captured launch can be replayed group after
 *   group.
 *   3 <= K <= 64; kp_d and kp_s 8-byte aligned (float2 loads), the outputs and the state 4-byte aligned.  One workgroup (one wave) per source, no atomics:
 *   two runs on the same input are bit-identical.  Returns 0, or nonzero with mrfa_last_error() set before anything is written. */
int mrfa_kp_pose_dist(void* stream, const float* kp_d, const float* kp_s, int B, int rep, int K, float* dist_out, float* area_out, void* state);

#ifdef __cplusplus
}
#endif
#endif
