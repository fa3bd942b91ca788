/* C ABI of the key-frame memories of libvd_hip.so (csrc/keyframes.hip; distill.KeyframeDMTrainer, run_dm --memories keyframes).
 *
 * A key-frame memory is K learned frames (K, 3, H, W) that stand for a clip of T frames: frame t of the clip is a fixed two-tap
 * combination of two of them.  K = 1 is the still clip of vds_still_expand, K = T with the identity table is the clip itself;
 * in between are the paper's temporal segments ("nearest") and linear interpolation along T with aligned end points ("linear").
 * video_distillation_amd/keyframes.py is the one definition of the tables.
 *
 * A header of its own with the prefix vdk_: include/vd_hip.h and its 93 names are closed (tests/test_cabi.py pins them).  The
 * conventions are those of vd_hip.h: `int` functions return 0 or an error code, `stream` is a hipStream_t (null: the default
 * stream), launches are asynchronous on it, tensors are contiguous fp32 device memory.  The table is HOST memory; it travels to
 * the kernels by value in their arguments, so nothing is uploaded and the caller may free it when the call returns.
 *
 * Argument checks come before any HIP call, in this order: -1 for a table vdk_table_check refuses, a non-positive H or W or a
 * negative n; then 0 for n == 0; then -1 for a null data pointer.  16-byte loads and stores are used where 3*H*W is a multiple of
 * 4 and both bases are 16-byte aligned, 4-byte ones otherwise; element offsets are 64-bit. */
#ifndef VD_KEYFRAMES_H
#define VD_KEYFRAMES_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VDK_MAX_FRAMES 64

/* Frame t < T of a clip = w0[t] * key i0[t] + w1[t] * key i1[t]; entries at t >= T are not read. */
typedef struct VdkTable { int32_t T, K; int32_t i0[64], i1[64]; float w0[64], w1[64]; } VdkTable;

/* Host only.  0, or -1 for: a null table, T or K outside 1..VDK_MAX_FRAMES, K > T, an index i0[t] / i1[t] (t < T) outside
 * 0..K-1, a weight w0[t] / w1[t] (t < T) that is not finite. */
int vdk_table_check(const VdkTable* table);

/* out[i][t] = w0[t] * keys[i][i0[t]] + w1[t] * keys[i][i1[t]] at every [c][y][x]: fp32, each product and the sum rounded on its
 * own (no fused multiply-add).  A term whose weight is exactly zero is skipped (a zero weight never meets an infinity), so a
 * single term of weight 1 is a copy; a frame both of whose weights are zero is 0.  keys [n][K][3][H][W], out [n][T][3][H][W]. */
int vdk_keyframe_expand(const float* keys, int64_t n, const VdkTable* table, int H, int W, float* out, void* stream);

/* The adjoint of vdk_keyframe_expand: g_keys[i][k] = the sum of w * g_clips[i][t] over the non-zero terms (t, w) of the table
 * whose index is k, walked in ascending t and within one t the i0 term before the i1 term; the accumulator starts from the first
 * product, every product and add is rounded on its own, a key with no term gets 0.  No atomics: bitwise repeatable, and equal
 * to a host loop of float operations.  g_clips [n][T][3][H][W], g_keys [n][K][3][H][W]. */
int vdk_keyframe_reduce(const float* g_clips, int64_t n, const VdkTable* table, int H, int W, float* g_keys, void* stream);

#ifdef __cplusplus
}
#endif

#endif
