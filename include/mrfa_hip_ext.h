/* libmrfa_hip.so: entries whose CPU specification lives beside their tests (tests/emu_ext.py, tests/emu_metrics.py, tests/emu_frames.py), not in the ABI
 * emulator.
 *
 * include/mrfa_hip.h is one table with the ctypes binding (mrfa_amd/hip.py: _SIGNATURES) and the emulator: an entry declared there has to appear in
 * all three at once.  An entry declared HERE is bound from the binding's second table (hip._EXT_SIGNATURES), looked up with hip.has() by its one caller,
 * and specified by tests/emu_ext.py::ExtEmulator or a subclass of it (tests/emu_metrics.py::MetricsEmulator, tests/emu_frames.py::FramesEmulator).  The
 * ABI version of mrfa_hip.h does not move for it: a library without the entry loads, and the caller says that the library has to be rebuilt.
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

/* Full-reference metrics of a clip, per frame: L1, MSE and SSIM of pred (N,C,H,W) against target (N,C,H,W), frame n against frame n, both contiguous
 * fp32 (reconstruction.py:52-70 reports L1 and PSNR per frame; PSNR is 20 log10(1 / sqrt(mse)), the caller's one line).  Inference only.
 *
 *   out (N,4): out[n] = {l1, mse, ssim, 0};  l1 = mean |p - t| and mse = mean (p - t)^2 over C H W.
 *   ssim (Wang et al. 2004, data range 1): window of 11 taps g_i = exp(-(i - 5)^2 / 4.5) / sum, computed in float64 and rounded to fp32 -- those eleven
 *   fp32 numbers are the definition --, separable and "valid" (no padding: (H - 10) x (W - 10) windows per channel); under it mu_x, mu_y, E[x^2], E[y^2],
 *   E[xy]; s_xx = E[x^2] - mu_x^2, s_yy and s_xy likewise, not clamped; C1 = 0.01^2, C2 = 0.03^2;
 *     S = (2 mu_x mu_y + C1)(2 s_xy + C2) / ((mu_x^2 + mu_y^2 + C1)(s_xx + s_yy + C2));   ssim = mean of S over channels and windows.
 *   want_ssim == 0: ssim is written as 0 (never NaN) and no window is computed; any H, W >= 1.  want_ssim != 0 needs min(H, W) >= 11.
 *   Non-finite inputs propagate through the sums of the frames (and windows) that hold them; the entry does not classify them.
 *   The kernels work in fp32 on tiles of MRFA_METRICS_TILE_H x MRFA_METRICS_TILE_W pixels (second moments on x - 0.5 and y - 0.5: the variances do not
 *   move, the means get the 0.5 back), no fp32 addition chain longer than 16; the tiles' partial sums are added in float64 in a fixed order, divided by
 *   the counts and rounded once.  No atomics: two runs on the same input are bit-identical.  Any H and W: every load is one fp32.
 *   workspace: mrfa_frame_metrics_workspace(N, C, H, W) bytes of scratch (24 per tile, channel and frame; < 0 if a dimension is < 1 or the tiles exceed
 *   one grid), written by every call, whatever it held before.
 *   pred, target and out 4-byte aligned, the workspace 8-byte aligned.  Returns 0, or nonzero with mrfa_last_error() set before anything is written: a null
 *   pointer, a dimension < 1, a workspace smaller than asked for, want_ssim with min(H, W) < 11, a misaligned pointer. */
#define MRFA_METRICS_TILE_H 32
#define MRFA_METRICS_TILE_W 32
long long mrfa_frame_metrics_workspace(int N, int C, int H, int W);
int mrfa_frame_metrics(void* stream, const float* pred, const float* target, int N, int C, int H, int W, int want_ssim, void* workspace,
                       long long workspace_bytes, float* out);

/* Frames as bytes: the two ends of an inference loop as the reference's callers hold them (frames_dataset.py:29-65 reads uint8 H x W x C frames;
 * demo.py:72,160, reconstruction.py:63-76 and logger.py:91-152 write uint8 H x W x 3 frames and grids) against planar fp32 (N,3,H,W) in [0,1].
 * Inference only.  Specified by tests/emu_frames.py::FramesEmulator.
 *
 * mrfa_frames_from_u8: src contiguous uint8 (N,H,W,Cin), Cin in {1,3,4}; dst contiguous fp32 (N,3,H,W).
 *     dst[n,c,y,x] = fl32(v) * fl32(1.0 / 255.0)
 *   ONE fp32 multiply by the fp32-rounded reciprocal: what np.multiply(u8, 1. / 255, dtype=np.float32) gives and what the reference's dtype conversion is
 *   documented to do.  A division v / 255.0f differs from it in the last bit for some v and is not this rule.
 *   v = src[n,y,x,c] for Cin 3 and 4 (channel 3, alpha, is ignored); v = src[n,y,x,0] for all three planes for Cin 1 (grey).
 *   Refuses, nonzero with mrfa_last_error() set before anything is written: a null pointer, N, H or W < 1, any other Cin, a dst that is not 4-byte aligned.
 *   src may lie at any address.  Where W % 4 == 0, src is 4-byte and dst 16-byte aligned, a lane moves four pixels (4 Cin bytes as dwords in, one 16-byte
 *   store per plane out); every other case takes a pixel per lane.
 *
 * mrfa_frames_to_u8: dst contiguous uint8 (N,Hd,Wd,3); tiles: a HOST array of 1 <= n_tiles <= MRFA_U8_MAX_TILES descriptors, which travel to the kernel
 *   as launch arguments (no table on the device, nothing to keep alive: a captured launch replays).  Tile t writes image n of its src (contiguous fp32
 *   (N,3,H,W)) to dst[n, y0:y0+H, x0:x0+W, :].  A tile lies inside Hd x Wd; tiles do not overlap each other (checked, refused); bytes of dst that no tile
 *   covers are not written.
 *   A sample s becomes a byte q:  p = s * 255.0f in fp32 (one multiply), then
 *     rounding == 0 ("nearest": img_as_ubyte, demo.py:160)                q = rint(p), ties to even, clamped to [0,255]
 *     rounding == 1 ("floor": reconstruction.py:73, logger.py:151)        q = trunc(p), clamped to [0,255]
 *   NaN gives 0, +inf 255, -inf 0.  The clamp is this library's definition for inputs outside [0,1] (the reference raises for them in one case and wraps in
 *   the other); for inputs in [0,1] the result is the reference's.
 *   Keypoint discs, kp != NULL: kp (N,K,2), (x, y) in [-1,1], 1 <= K <= MRFA_U8_MAX_KP; colors (K,3) fp32 in [0,1].  Centre in pixels
 *     cx = W (x + 1) / 2, cy = H (y + 1) / 2     (the reference's spatial_size * (kp + 1) / 2, not the align-corners form;
 *                                                   in fp32: fl(fl(W * fl(x + 1)) * 0.5))
 *   pixel (r,c) of the tile takes colour k if (r - cy)^2 + (c - cx)^2 < radius^2 (fp32, each operation rounded once, in this order); for several k the
 *   LARGEST k wins (the reference's loop overwrites in order).  The colour is quantised by the same `rounding`.  Discs are clipped to the tile and never
 *   spill into a neighbouring one.  A non-finite keypoint draws nothing.
 *   Border, border != 0: columns 0 and W - 1 of the tile are 255 in all three channels, applied AFTER the discs; rows are not touched (logger.py:118-121
 *   sets the two columns twice and no rows).
 *   Refuses, before anything is written: a null dst / tiles / src, colors == NULL where kp != NULL, K outside 1..64, a radius <= 0 or not finite (both only
 *   where kp != NULL), H or W < 1, a tile outside dst, two tiles that overlap, n_tiles outside 1..8, rounding not 0 or 1, N, Hd or Wd < 1, a src, kp or colors
 *   that is not 4-byte aligned.  dst may lie at any address.
 *   A lane moves four pixels of a row: one 16-byte load per plane where the tile's W % 4 == 0 and its src is 16-byte aligned, three dword stores where
 *   the four pixels' 12 bytes start 4-byte aligned in dst (with 3 Wd % 4 != 0 that changes from row to row: decided per four pixels); scalar loads and byte
 *   stores otherwise (odd W, odd x0, the tail).  No atomics, every byte has one writer: two runs on the same input are bit-identical. */
#define MRFA_U8_MAX_TILES 8
#define MRFA_U8_MAX_KP 64
typedef struct {
    const float* src;
    int H, W;
    int y0, x0;
    const float* kp;
    int K;
    float radius;
    const float* colors;
    int border;
} mrfa_u8_tile;
int mrfa_frames_from_u8(void* stream, const unsigned char* src, int N, int H, int W, int Cin, float* dst);
int mrfa_frames_to_u8(void* stream, const mrfa_u8_tile* tiles, int n_tiles, int N, unsigned char* dst, int Hd, int Wd, int rounding);

#ifdef __cplusplus
}
#endif
#endif
