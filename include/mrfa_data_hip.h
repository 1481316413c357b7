/* C ABI of libmrfa_data_hip.so: the input pipeline's device side.  One entry: a batch of uint8 frame PAIRS, as an image reader returns them, becomes the
 * augmented fp32 `source` / `driving` batches of the training step -- the flips and the colour jitter of the reference's AllAugmentationTransform
 * (augmentation.py:325-355: RandomFlip and ColorJitter, the two transforms both training configs switch on), with arithmetic that is Pillow's to the byte.
 *
 * A library of its own beside libmrfa_hip.so (include/mrfa_hip.h): it shares no exported symbol with it, has its own version number and its own binding
 * (mrfa_amd/data_hip.py).  This comment is the specification; tests/ref_augment.py restates it in numpy, mrfa_amd/csrc_data/augment_math.h is the one text
 * of the per-pixel rules that both the device and the host tests compile.
 *
 * ---------------------------------------------------------------------------------------------------------------------------------------------------
 * The per-pixel rules.  All values are bytes unless stated; "f32" / "f64": every operation rounded to that format, no contraction, no fast-math.
 *
 *   luma      L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16
 *   blend     of a degenerate byte d and a pixel byte x by the f32 factor f:  t = f32(d) + f * (f32(x) - f32(d))  (f32),  result trunc(t) clamped to
 *             [0, 255]
 *   BRIGHTNESS   blend with d = 0, every channel
 *   SATURATION   blend with d = L of that pixel, every channel
 *   CONTRAST     blend with d = m, every pixel and channel;  m = floor((2 S + n) / (2 n)),  S the sum of L over the n = H W pixels of THAT FRAME as it is
 *                when contrast's turn comes (after the ops that precede it in the order): int(mean(L) + 0.5)
 *   HUE          RGB -> HSV,  H = (H + hue_shift) mod 256,  HSV -> RGB.
 *     RGB -> HSV:  V = max.  max == min: H = S = 0.  Otherwise cr = f32(max - min), sat = cr / f32(max), rc, gc, bc = f32(max - c) / cr  (f32 each);
 *                  h = bc - gc (f32) where R == max, else f32(2.0 + rc - bc) where G == max, else f32(4.0 + gc - rc), those two sums in f64;
 *                  h = f32(fmod(f64(h) / 6.0 + 1.0, 1.0));  H = clamp(int(f64(h) * 255.0)),  S = clamp(int(f64(sat) * 255.0))
 *     HSV -> RGB:  S == 0: grey V.  Otherwise hf = f64(H) * 6.0 / 255.0, i = floor(hf), f = f32(hf - i), fs = f32(f64(S) / 255.0);
 *                  p = round(V (1 - fs)), q = round(V (1 - fs f)), t = round(V (1 - fs (1 - f))) in f64, C round() (halves away from zero), clamped;
 *                  i mod 6 selects (V,t,p), (q,V,p), (p,V,t), (p,q,V), (t,p,V), (V,p,q)
 *   byte -> float   fl32(b) * fl32(1.0 / 255.0), ONE fp32 multiply: the rule of mrfa_frames_from_u8.  (The reference forms b / 255 in float64 and casts: both
 *                   round the same number, so they differ by at most one ulp, 2^-24.)
 *
 * ---------------------------------------------------------------------------------------------------------------------------------------------------
 * mrfa_pair_augment: src contiguous uint8 (B,2,H,W,Cin), frame 0 of a pair the earlier one; Cin 1: grey, the byte in all three channels; Cin 4: the fourth
 *   byte is never read.  params: a HOST array of B descriptors, read during the call only -- they travel as launch arguments, nothing on the device needs
 *   keeping alive.  source, driving: contiguous fp32 (B,3,H,W).  Pair b:
 *     the ops params[b].op[0..3] apply in that order to BOTH frames (MRFA_AUG_NONE entries are skipped), each frame with its own contrast mean;
 *     time_flip == 0: frame 0 -> source[b], frame 1 -> driving[b];  != 0: frame 1 -> source[b], frame 0 -> driving[b];
 *     hflip != 0: output column x shows input column W - 1 - x;
 *     then byte -> float.
 *   Two launches at most: a luma-sum pass, only when some pair has CONTRAST (per frame, MRFA_AUG_PARTS integer partial sums into the workspace; no atomics,
 *   nothing needs zeroing, every run bit-identical), and the apply pass.  One lane owns four consecutive pixels of a row where W % 4 == 0 (Cin dwords in where
 *   src is 4-byte aligned, one float4 per plane out where source / driving are 16-byte aligned), one pixel otherwise.  src may lie at any address.
 *   Returns 0, or nonzero with mrfa_data_last_error() set BEFORE anything is written: a null pointer; a dimension < 1 or H W > MRFA_AUG_MAX_PIXELS; B >
 *   MRFA_AUG_MAX_PAIRS; Cin not in {1,3,4}; an op code out of range or an op repeated in one descriptor; a factor that is not finite or < 0; a workspace
 *   smaller than mrfa_pair_augment_workspace(B, H, W) or not 8-byte aligned; source or driving not 4-byte aligned.
 * mrfa_pair_augment_workspace: bytes, or < 0 for a dimension the entry would refuse.                                                                    */
#ifndef MRFA_DATA_HIP_H
#define MRFA_DATA_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define MRFA_DATA_ABI_VERSION 1
int mrfa_data_version(void);
const char* mrfa_data_last_error(void);

#define MRFA_AUG_MAX_PAIRS 32              /* descriptors of one launch: 32 x 20 bytes of kernel arguments */
#define MRFA_AUG_PARTS 64                  /* partial luma sums per frame (32-bit each: H W <= MRFA_AUG_MAX_PIXELS keeps 255 H W / 64 below 2^32) */
#define MRFA_AUG_MAX_PIXELS (1LL << 30)

/* op codes: factor[op - 1] is the factor of BRIGHTNESS, CONTRAST, SATURATION; HUE reads hue_shift */
#define MRFA_AUG_NONE 0
#define MRFA_AUG_BRIGHTNESS 1
#define MRFA_AUG_CONTRAST 2
#define MRFA_AUG_SATURATION 3
#define MRFA_AUG_HUE 4

typedef struct {
    float factor[3];                       /* brightness, contrast, saturation: finite, >= 0 (1: identity) */
    unsigned char op[4];                   /* op codes in application order, MRFA_AUG_NONE as padding */
    unsigned char hue_shift;               /* added to H modulo 256: trunc(255 h) mod 256 of a hue factor h in [-0.5, 0.5] */
    unsigned char time_flip, hflip;
    unsigned char reserved;
} mrfa_pair_aug;

long long mrfa_pair_augment_workspace(int B, int H, int W);
int mrfa_pair_augment(void* stream, const unsigned char* src, int B, int H, int W, int Cin, const mrfa_pair_aug* params, void* workspace,
                      long long workspace_bytes, float* source, float* driving);

#ifdef __cplusplus
}
#endif
#endif
