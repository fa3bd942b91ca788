/* Fourth public header of libvd_hip.so: still clips as first-level operand rows (csrc/still_rows.hip; distill.StillDMTrainer,
 * run_dm --memories static).
 *
 * The first conv level reads its input as padded 16-bit pixel rows (vd_pix2rows, vd_hip.h).  A batch of still clips -- one image
 * repeated over T frames (vd_still.h) -- needs no fp32 clips on the way there: each 16-byte chunk of a row is built once from the
 * image and stored at the T frame positions.
 *
 * Conventions are those of vd_hip.h: raw device pointers (contiguous fp32 `images`, int64 `index`, 16-byte aligned outputs), a
 * hipStream_t passed as void*, work enqueued without synchronising, nothing allocated or freed, 0 on success or a non-zero
 * hipError_t.  The argument checks come before any HIP call: -1 for a non-positive T / H / W, a negative n or a `prec` outside
 * VD_PREC_BF16 .. VD_PREC_F16X3 (0..3), then 0 for n == 0, then -1 for a null `images` / `out_hi`.  16-byte loads are used where
 * W is a multiple of 4 and `images` is 16-byte aligned, 4-byte loads otherwise; element and byte offsets are 64-bit.  `index` is
 * a device array the caller has validated (every entry in [0, N)); it may repeat rows, and may be null for the identity.  These
 * entry points carry the prefix vdsr_ and do not change VD_ABI_VERSION.
 */
#ifndef VD_STILLROWS_H
#define VD_STILLROWS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The first-level operand rows of the n still clips images[index ? index[i] : i] repeated over T frames:
 *   out[clip i][t*3+c][h][pitch], pitch = ((W + 8 + 7) / 8) * 8 16-bit elements, 3 zero pixels in front, zeros behind
 * -- byte for byte what vd_pix2rows(x = vds_still_expand(images, index, n, T, H, W), clip_index = null, n, T, H, W, out_hi,
 * out_lo, prec) writes: out_hi the rn16 values (bf16 for VD_PREC_BF16 / BF16X3, fp16 for VD_PREC_F16 / F16X3), out_lo (may be
 * null) rn16(v - hi).  images [N][3][H][W]; each output plane holds n * T * 3 * H * pitch elements. */
int vdsr_still_rows(const float* images, const int64_t* index, int64_t n, int T, int H, int W, void* out_hi, void* out_lo, int prec,
                    void* stream);

#ifdef __cplusplus
}
#endif

#endif /* VD_STILLROWS_H */
