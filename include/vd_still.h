/* Third public header of libvd_hip.so: still clips (csrc/still.hip; distill.StillGMTrainer, run_dc --memories static).
 *
 * A still clip is one image repeated over T frames: what the reference's `static*` / `single*` datasets hand to ConvNet3D
 * (distill_utils/dataset.py:626-633).  The images stay in HBM, the clips are built per step, and a clip gradient goes back to
 * its image as the sum over the frames.
 *
 * Conventions are those of vd_hip.h: raw device pointers to contiguous fp32 (int64 for `index`), a hipStream_t passed as void*,
 * work enqueued without synchronising, nothing allocated or freed, 0 on success or a non-zero hipError_t.  The argument checks
 * come before any HIP call: -1 for a non-positive T / H / W or a negative n, then 0 for n == 0, then -1 for a null `images` /
 * `out` / `g_clips` / `g_images`.  16-byte accesses are used where 3*H*W is a multiple of 4 and the bases are 16-byte aligned,
 * 4-byte accesses otherwise; element offsets are 64-bit.  `index` is a device array the caller has validated (every entry in
 * [0, N)); it may repeat rows, and may be null for the identity.  These entry points do not change VD_ABI_VERSION.
 */
#ifndef VD_STILL_H
#define VD_STILL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* out[i][t][c][y][x] = images[index ? index[i] : i][c][y][x], t < T.  images [N][3][H][W], out [n][T][3][H][W]. */
int vds_still_expand(const float* images, const int64_t* index, int64_t n, int T, int H, int W, float* out, void* stream);

/* g_images[i][c][y][x] = (((g[i][0] + g[i][1]) + g[i][2]) + ... ) + g[i][T-1]  at [c][y][x]: fp32, ascending t, one add per
 * frame, each rounded on its own.  No atomics: bitwise repeatable.  g_clips [n][T][3][H][W], g_images [n][3][H][W]. */
int vds_still_reduce(const float* g_clips, int64_t n, int T, int H, int W, float* g_images, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* VD_STILL_H */
