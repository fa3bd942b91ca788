/* C ABI of the regression test statistics of libvd_hip.so (csrc/regress_stats.hip; video_distillation_amd/evalpool.py, frepo.py).
 *
 * FRePo's evaluation (FRePo/lib_torch/utils.py:522-601, evaluate_synset / epoch) tests a network with a mean-squared error on the
 * soft labels one_hot - 1/K and an argmax accuracy.  vd_eval_stats (include/vd_hip.h) keeps the statistics of a cross-entropy test
 * pass in a record an all-reduce can carry; this is the same record for the regression pass, so that evalpool's exchange and
 * `derive` carry over unchanged.
 *
 * A header of its own with the prefix vdr_: include/vd_hip.h and its 93 names are closed (tests/test_cabi.py pins them), as are
 * vd_keyframes.h, vd_nfr.h and vd_frepo.h.  The conventions are those of vd_hip.h: an `int` function returns 0 or a negative error
 * code, `stream` is a hipStream_t (null: the default stream), the launch is asynchronous on it and nothing synchronises with the
 * host. */
#ifndef VD_REGRESS_H
#define VD_REGRESS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Accumulate (+=) the statistics of one test batch -- logits [B][K] fp32, labels [B] int64 -- into the fp64 record rec[8 + 2K], in
 * ONE launch.  The slots are those of vd_eval_stats:
 *
 *   rec[0]              clips seen (labels in [0, K))
 *   rec[1]              sum over those clips and all K classes of ((double)z_k - (double)y_k)^2, where y_k is the fp32 value
 *                       (k == label ? 1.0f : 0.0f) - (float)(1.0 / K): what frepo.soft_labels(label, K) holds
 *   rec[2] [3] [4]      top-1 / top-3 / top-5 hits: the label's rank -- the number of classes with a strictly greater logit plus
 *                       the number with an equal logit at a lower index -- is below 1 / 3 / 5
 *   rec[5]              labels outside [0, K): counted here and nowhere else
 *   rec[6] rec[7]       not written (zero in a record that started at zero)
 *   rec[8 .. 8+K)       top-1 hits per class
 *   rec[8+K .. 8+2K)    clips per class
 *
 * The mean-squared error of a pass is rec[1] / (K * rec[0]).  Differences and squares are rounded in fp64 one by one (no fused
 * multiply-add); the batch's sum is formed in a fixed order and added to rec[1] by one thread; every other slot counts integers.
 * A second call on the same inputs and record gives the same bits.  A NaN logit makes rec[1] NaN; comparisons with it are false,
 * so the counts still follow the rank rule.
 *
 * B == 0 returns 0 and touches nothing.  B < 0, K < 1, or a null pointer with B > 0 is -1, before any HIP call. */
int vdr_regress_stats(const float* logits, const int64_t* labels, int B, int K, double* rec, void* stream);

#ifdef __cplusplus
}
#endif

#endif
