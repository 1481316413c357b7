/* C ABI of the resize entries of libmrfa_data_hip.so: uint8 frames (N,Hi,Wi,Cin), as a video decoder returns them, are cropped to a box and resized to the
 * model's size on the device, in one launch, with the bytes of Pillow's Image.resize(size, resample, box) on 8-bit channels.
 *
 * A second entry group of the data library beside include/mrfa_data_hip.h: it shares no name with that header or with include/mrfa_hip.h, has its own version
 * number (mrfa_resize_version) and its own binding (mrfa_amd/resize_hip.py); errors go through the library's one thread-local message,
 * mrfa_data_last_error() of mrfa_data_hip.h.  This comment is the specification; tests/ref_resize.py restates it in numpy, and
 * mrfa_amd/csrc_data/resize_coeffs.h is the one text of the coefficient rules, which the library and a stand-alone host test both compile.
 *
 * ---------------------------------------------------------------------------------------------------------------------------------------------------
 * One axis: input length n, box [in0, in1] (float32 both), output length m, filter f with support s.  "f64": every operation rounded to double, no
 * contraction, no fast-math; (int) is C's truncation.
 *
 *   d = in1 - in0                         formed IN float32; everything below in f64
 *   scale = d / m;  fscale = max(scale, 1.0);  support = s * fscale;  ksize = 2 * (int)ceil(support) + 1;  ss = 1.0 / fscale
 *   for xx in [0, m):
 *       center = in0 + (xx + 0.5) * scale
 *       xmin = max((int)(center - support + 0.5), 0)
 *       cnt  = min((int)(center + support + 0.5), n) - xmin
 *       w[x] = f((x + xmin - center + 0.5) * ss) for x in [0, cnt);  ww = the sum of w in index order;  w[x] = w[x] / ww where ww != 0
 *       kk[xx][x] = (int)(w[x] * 4194304.0 + (w[x] < 0 ? -0.5 : 0.5))           2^22, halves away from zero; the entries from cnt to ksize - 1 are 0
 *       bounds[xx] = (xmin, cnt)
 *   out[xx] = clamp((2^21 + sum over x in [0, cnt) of in[xmin + x] * kk[xx][x]) >> 22, 0, 255)      int32 accumulator, arithmetic shift
 *
 * The filters (support), sin and cos of libm:
 *   BOX (0.5)       1 for -0.5 < x <= 0.5, else 0
 *   BILINEAR (1)    1 - |x| for |x| < 1, else 0
 *   HAMMING (1)     x <- |x|: 1 at 0, 0 for x >= 1, otherwise with p = x * pi:  sin(p) / p * (0.54 + 0.46 * cos(p))
 *   BICUBIC (2)     a = -0.5, x <- |x|:  ((a + 2) x - (a + 3)) x x + 1 for x < 1;  (((x - 5) x + 8) x - 4) a for x < 2;  else 0
 *   LANCZOS (3)     sinc(x) * sinc(x / 3) for -3 <= x < 3, else 0;  sinc(0) = 1, otherwise with p = x * pi:  sin(p) / p
 *
 * Two passes, the horizontal one first: it writes BYTES (rounded and clamped as above), which the vertical pass reads.  Channels are independent.  Both passes
 * always run: where Pillow skips the pass of an axis with m == n and a full box, these coefficients make that pass the identity.
 * Input channels are mrfa_frames_from_u8's: Cin 3 as it is; Cin 1: the byte fills all three channels; Cin 4: the fourth byte is never read -- that is Pillow
 * on a[..., :3], NOT its premultiplied RGBA path.
 * byte -> float: fl32(b) * fl32(1.0 / 255.0), one fp32 multiply (the rule of mrfa_frames_from_u8).
 *
 * ---------------------------------------------------------------------------------------------------------------------------------------------------
 * mrfa_resize_ksize: the taps per output sample of an axis, or < 0 with the message set: in_size or out_size < 1; an unknown filter; a box that is not
 *   finite, lies outside [0, in_size] or has in1 - in0 <= 0 (in float32); more than MRFA_RESIZE_MAX_TAPS taps.
 * mrfa_resize_coeffs: fills the HOST tables bounds (2 out_size ints: xmin, cnt per output sample) and kk (out_size rows of ksize ints) of an axis.  Returns 0,
 *   or nonzero with the message set before anything is written: a null table, or whatever mrfa_resize_ksize refuses.  Every row has xmin >= 0,
 *   0 <= cnt <= ksize and xmin + cnt <= in_size.
 * mrfa_frames_resize_u8: src contiguous uint8 (N,Hi,Wi,Cin) on the device, at any byte address.  bounds_h, kk_h (Wo rows, from the source's width and the
 *   box's left and right) and bounds_v, kk_v (Ho rows, height, upper and lower): DEVICE copies of tables that mrfa_resize_coeffs made; the launch trusts them
 *   and validates nothing on the device.  out_f32: contiguous fp32 (N,3,Ho,Wo), or NULL; out_u8: contiguous uint8 (N,Ho,Wo,3), or NULL.
 *   One launch: a workgroup owns 8 x 32 output pixels, resamples the rows of its vertical footprint horizontally, straight from global memory, into bytes in
 *   LDS and runs the vertical pass out of LDS -- in several rounds where the footprint has more rows than it holds at a time (MRFA_RESIZE_FOOT_ROWS) --,
 *   then writes one float4
 *   per plane and packed dwords of bytes where Wo % 4 == 0 and the outputs are 16- / 4-byte aligned, scalars otherwise.  No atomics, nothing needs zeroing,
 *   every run is bit-identical.
 *   Returns 0, or nonzero with the message set BEFORE anything is written: a null src or table; both outputs null; a dimension < 1, N > 65535 or more than
 *   65535 tiles one way; Cin not in {1,3,4}; ksize_h or ksize_v outside [1, MRFA_RESIZE_MAX_TAPS]; out_f32 not 4-byte aligned.                          */
#ifndef MRFA_RESIZE_HIP_H
#define MRFA_RESIZE_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define MRFA_RESIZE_ABI_VERSION 1
int mrfa_resize_version(void);

/* 3840 x 2160 -> 256 x 256 Lanczos has 91 and 53 taps, a 16x Lanczos reduction 97, a 60x one 361 (ksize is odd: 383 is 2 * 191 + 1) */
#define MRFA_RESIZE_MAX_TAPS 383
#define MRFA_RESIZE_LDS_TAPS 127           /* both axes at most this: the workgroup keeps its rows of both tables in LDS */
#define MRFA_RESIZE_FOOT_ROWS 192          /* horizontally resampled rows a workgroup holds at a time, twice as many where the tables stay in global memory:
                                              >= the taps of one output row either way, so every output row fits a round */

#define MRFA_RESIZE_BOX 0
#define MRFA_RESIZE_BILINEAR 1
#define MRFA_RESIZE_HAMMING 2
#define MRFA_RESIZE_BICUBIC 3
#define MRFA_RESIZE_LANCZOS 4

int mrfa_resize_ksize(int in_size, float in0, float in1, int out_size, int filter);
int mrfa_resize_coeffs(int in_size, float in0, float in1, int out_size, int filter, int* bounds, int* kk);
int mrfa_frames_resize_u8(void* stream, const unsigned char* src, int N, int Hi, int Wi, int Cin, const int* bounds_h, const int* kk_h, int ksize_h,
                          const int* bounds_v, const int* kk_v, int ksize_v, int Ho, int Wo, float* out_f32, unsigned char* out_u8);

#ifdef __cplusplus
}
#endif
#endif
