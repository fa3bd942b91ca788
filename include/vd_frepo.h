/* C ABI of the regression train step of libvd_hip.so (csrc/frepo.hip; video_distillation_amd/frepo.py, train.py).
 *
 * Every network FRePo trains (FRePo/script/distill_s2d.py:145-156, PoolElement.train_steps; FRePo/lib_torch/utils.py:561-601,
 * evaluate_synset) minimises a mean-squared error on soft labels with Adam or AdamW.  These are the two pieces of that step the
 * library did not have: the loss with its logit gradient, standing where vd_ce_loss stands in the cross-entropy step, and the
 * optimiser update of all parameter tensors in one launch.
 *
 * A header of its own with the prefix vdf_: include/vd_hip.h and its 93 names are closed (tests/test_cabi.py pins them).  The
 * conventions are those of vd_hip.h: `int` functions return 0 or a negative error code, `stream` is a hipStream_t (null: the
 * default stream), launches are asynchronous on it and nothing synchronises with the host.  Argument checks come before any HIP
 * call: a null pointer, a non-positive dimension or length, or a segment count outside 1..VDF_ADAM_MAX is -1.  No kernel uses
 * a floating-point atomic and every sum has a fixed order: a second call on the same inputs gives the same bits. */
#ifndef VD_FREPO_H
#define VD_FREPO_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VDF_ADAM_MAX 16

/* nn.MSELoss() (mean over all B*K elements) of logits [B][K] against targets [B][K], and its logit gradient.  One launch.
 *
 *   loss[0]       = (float)( sum_i ((double)l_i - (double)y_i)^2 / (double)(B K) )      the fp64 sum in a fixed order, rounded once
 *   dlogits[i]    = (l_i - y_i) * c,   c = (float)(2 / (double)(B K))                   fp32: the difference and the product each
 *                                                                                      rounded on their own (no fused multiply-add)
 *
 * vd_head_train_bwd consumes dlogits unchanged.  The loss is summed by one workgroup: the op is meant for B K up to a few
 * hundred thousand. */
int vdf_mse_loss(const float* logits, const float* targets, int B, int K, float* loss, float* dlogits, void* stream);

/* One tensor of an Adam step: parameter p, first moment m, second moment v (updated in place), gradient g (read), n elements each.
 * step_size = lr / (1 - beta1^t) and lr_wd = lr * weight_decay (0: Adam; otherwise AdamW's decoupled decay) are per segment, so
 * param groups with different learning rates share a launch.  first_block is filled in by the library. */
typedef struct VdfAdamSeg { float* p; float* m; float* v; const float* g; int64_t n; float step_size; float lr_wd; int32_t first_block; int32_t reserved; } VdfAdamSeg;

/* Up to VDF_ADAM_MAX segments and the constants they share.  bc2_sqrt = sqrt(1 - beta2^t).  The host computes step_size and
 * bc2_sqrt in double, as torch.optim.Adam does, and rounds each to float once; one_minus_beta1 / one_minus_beta2 are
 * (float)(1 - (double)beta) likewise. */
typedef struct VdfAdamBatch { int32_t nseg; int32_t reserved; float beta1; float one_minus_beta1; float beta2; float one_minus_beta2; float bc2_sqrt; float eps; VdfAdamSeg seg[16]; } VdfAdamBatch;

/* One Adam / AdamW step over every segment of *batch (HOST memory, copied into the kernel arguments: nothing is uploaded) in ONE
 * launch.  Per element, in fp32, every multiplication, addition, division and square root rounded on its own, in this order (no
 * contraction to fused multiply-add; a float32 restatement of these lines reproduces the result bit for bit):
 *
 *   if lr_wd != 0:  p = p * (1 - lr_wd)
 *   m = m + one_minus_beta1 * (g - m)
 *   v = beta2 * v + one_minus_beta2 * (g * g)
 *   p = p - (step_size * m) / (sqrt(v) / bc2_sqrt + eps)
 *
 * Any float-aligned pointers and any n >= 1: where the four pointers of a segment share their offset within 16 bytes the aligned
 * body moves in 16-byte accesses with a scalar head and tail, otherwise the segment moves in 4-byte accesses.  Segments must not
 * overlap.  The grid is sized to the chip (at most 2048 workgroups, dealt to the segments by length). */
int vdf_adam_multi(const VdfAdamBatch* batch, void* stream);

#ifdef __cplusplus
}
#endif

#endif
