/* C ABI of the kernel ridge predictor of libvd_hip.so (csrc/nfr.hip; video_distillation_amd/nfr.py).
 *
 * FRePo's "neural feature regression" (FRePo/script/distill_s2d.py:124-137, PoolElement.nfr) predicts the labels of m target
 * clips from n synthetic clips by a kernel ridge solve on their features.  With F_s (n x d), Y_s (n x C), F_t (m x d):
 *
 *   K = F_s F_s^T     K_t = F_t F_s^T     lambda = |reg| tr(K) / n     A = K + lambda I = L L^T     Z = A^-1 Y_s     P = K_t Z
 *
 * and for an upstream gradient R = dl/dP (m x C):
 *
 *   g_Z = K_t^T R     Q = A^-1 g_Z = dl/dY_s     G = -Q Z^T     c = (|reg| / n) tr(G)
 *   dl/dF_s = (G + G^T) F_s + (Z R^T) F_t + 2 c F_s                  (the last term: tr(K) depends on F_s)
 *
 * F_t carries no gradient (the reference takes it under no_grad).  Everything is computed in fp64: cond(A) is bounded only by
 * 1 + n / reg and reaches 1e7 at reg = 1e-6, where an fp32 solve loses the gradient.  The factorisation is a Cholesky without
 * pivoting in a fixed order and no kernel uses a floating-point atomic: a second call gives the same bits.
 *
 * One deliberate difference from the reference: it forms lambda I through a float32 torch.eye, so its lambda is rounded to
 * fp32 even when every other operand is double.  Here lambda is an fp64 number (a relative difference of at most 2^-24 in
 * lambda).
 *
 * A header of its own with the prefix vdn_: include/vd_hip.h and its 93 names are closed (tests/test_cabi.py pins them).  The
 * conventions are those of vd_hip.h: `int` functions return 0 or a negative error code, argument checks come before any HIP
 * call, `stream` is a hipStream_t (null: the default stream), launches are asynchronous on it and nothing synchronises with the
 * host.  Inputs are contiguous fp32 device memory (exact in fp64), outputs contiguous fp64: nothing is rounded inside the
 * library.
 *
 * Dimensions: 1 <= n <= VDN_MAX_SYN and m, d, c >= 1; anything else, or a null pointer, is -1.
 *
 * The workspace (device memory, at least vdn_nfr_workspace_bytes bytes, 16-byte aligned, owned by the caller) carries the
 * factor from forward to backward; one workspace per forward call makes the op re-entrant.  Layout, in 8-byte words:
 *   [0]            int64 status: 0, or k + 1 when pivot k was the first that was not positive and finite (all-zero or
 *                  non-finite features).  When it is not 0 every output of forward and backward is NaN.  Nothing reads it on
 *                  the host unless asked.
 *   [1]            lambda
 *   [2 ..)         L (n x n, row major: L below and on the diagonal, L^T above), then Z (n x c), then K_t (m x n)
 * A factor with n <= VDN_LDS_SYN is held in LDS by the kernels that walk it; a larger one is streamed from the workspace. */
#ifndef VD_NFR_H
#define VD_NFR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VDN_MAX_SYN 1024
#define VDN_LDS_SYN 128

/* Bytes of the workspace of one forward call; -1 for dimensions the op refuses.  Host only. */
int64_t vdn_nfr_workspace_bytes(int n, int m, int d, int c);

/* pred [m][c] = K_t Z, and the workspace filled for vdn_nfr_backward.  feat_syn [n][d], y_syn [n][c], feat_tar [m][d].
 * Four launches: the Gram tiles of [F_s ; F_t] F_s^T on v_mfma_f64_16x16x4_f64, the factorisation (one workgroup), the two
 * triangular solves per block of 8 label columns, the tiles of K_t Z. */
int vdn_nfr_forward(const float* feat_syn, const float* y_syn, const float* feat_tar, int n, int m, int d, int c, double reg,
                    void* workspace, double* pred, void* stream);

/* g_feat_syn [n][d] = dl/dF_s and g_y_syn [n][c] = dl/dY_s for g_pred [m][c] = dl/dP, from the workspace of the forward call
 * with the same feat_syn, feat_tar, dimensions and reg; the workspace is only read.  Three launches: the tiles of K_t^T R, the
 * solves per block of 8 label columns, then [G + G^T | Z R^T] [F_s ; F_t] with both products of every tile on the f64 matrix
 * instruction. */
int vdn_nfr_backward(const float* feat_syn, const float* feat_tar, const float* g_pred, int n, int m, int d, int c, double reg,
                     const void* workspace, double* g_feat_syn, double* g_y_syn, void* stream);

#ifdef __cplusplus
}
#endif

#endif
