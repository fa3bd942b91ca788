/* Second public header of libvd_hip.so: the flat-parameter chain of trajectory matching (MTT).
 *
 * distill_baseline.py:231-283 / distill_s2d_ms.py:238-300 of the reference unroll `syn_steps` student updates over ReparamModule's
 * flat parameter vector (3.65 M floats at 50 classes) and let autograd walk back through them; distill.MTTTrainer walks back
 * explicitly.  The entry points below are the elementwise and reducing steps of that walk over the flat vector, one pass each.
 *
 * Conventions are those of vd_hip.h: raw device pointers, a hipStream_t passed as void*, work enqueued without synchronising,
 * nothing allocated or freed, 0 on success or a non-zero hipError_t / negative argument-error code.  The argument checks come
 * before any HIP call: -1 for a null or misaligned pointer (EVERY pointer is 16-byte aligned; only `hv` may be null), -2 for
 * n <= 0.  These entry points do not change VD_ABI_VERSION.
 *
 * Arithmetic.  Every fp32 operation is rounded on its own (no fused multiply-add), so an elementwise output is the float32
 * evaluation of its formula as written.  Sums are fp64 in a fixed order: a first launch, whose grid depends on n only, leaves one
 * partial per workgroup in `scratch`; a second launch of ONE workgroup adds the partials in index order and applies the scalar
 * update.  No atomics and no hand-off between workgroups inside a launch: the same inputs give the same bits.
 */
#ifndef VD_TRAJ_H
#define VD_TRAJ_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* doubles of `scratch` that vdt_traj_loss and vdt_traj_adjoint need for vectors of n floats (0 for n <= 0) */
int64_t vdt_traj_scratch_doubles(int64_t n);

/* theta_out[i] = theta[i] - lr_dev[0] * g[i]      (student_params[-1] - syn_lr * grad; out of place: the tape keeps every theta_s) */
int vdt_traj_step(const float* theta, const float* g, const float* lr_dev, int64_t n, float* theta_out, void* stream);

/* out[0] = dist = sum (theta - target)^2, out[1] = dist0 = sum (theta0 - target)^2 (differences and squares in fp64),
 * out[2] = dist / dist0 (the grand loss), out[3] = 0;  tbar[i] = (2.0f * (theta[i] - target[i])) / (float)dist0.
 * Three launches: partials, the fold into `out`, tbar. */
int vdt_traj_loss(const float* theta, const float* theta0, const float* target, int64_t n, double* scratch, double* out,
                  float* tbar, void* stream);

/* One reverse step, one pass over the vectors:  tbar[i] += hv[i] in place (hv == NULL: tbar as it is, the first reverse step);
 * g_lr[0] -= sum (double)tbar[i] * (double)g[i] with the updated tbar;  v[i] = (-(lr_dev[0] * share)) * tbar[i]. */
int vdt_traj_adjoint(float* tbar, const float* hv, const float* g, const float* lr_dev, float share, int64_t n, double* scratch,
                     double* g_lr, float* v, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* VD_TRAJ_H */
