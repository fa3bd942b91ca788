// FRePo's kernel ridge predictor ("neural feature regression") and its gradient, in fp64.
//
// Reference: FRePo/script/distill_s2d.py:124-137 (PoolElement.nfr) -- four torch ops in fp32 and a torch.linalg.solve.  The
// algebra and the workspace layout are in include/vd_nfr.h.  The system matrix A = F_s F_s^T + lambda I has a condition number
// of up to 1 + n / reg (1e7 at reg = 1e-6), so every operation here is fp64; the fp32 inputs are widened on load.
//
// Forward, four launches:
//   1. nfr_gram_kernel    : one workgroup per 32 x 32 tile of [F_s ; F_t] F_s^T on v_mfma_f64_16x16x4_f64 (the tiles of K strictly
//                           above the diagonal are skipped: nothing reads them), the next feature stage prefetched into registers.
//   2. nfr_factor_kernel  : one workgroup: lambda from the trace (summed in index order), then a right-looking Cholesky without
//                           pivoting, in LDS when n <= VDN_LDS_SYN and in the workspace otherwise.  L^T is mirrored above the
//                           diagonal, so both triangular solves walk rows.
//   3. nfr_solve_kernel   : one workgroup per block of 8 label columns: L y = Y_s, L^T z = y (right-hand sides in LDS, L in LDS
//                           when it fits) -> Z.
//   4. nfr_product_kernel : pred = K_t Z, one workgroup per 32 x 32 tile on the matrix instruction.
// Backward, three launches:
//   1. nfr_product_kernel : g_Z = K_t^T R into the buffer of dl/dY_s.
//   2. nfr_solve_kernel   : the same two solves in place -> Q = dl/dY_s.
//   3. nfr_grad_kernel    : one workgroup per 32 x 64 tile of dl/dF_s = [M_s | M_t] [F_s ; F_t].  M = [-(Q Z^T + Z Q^T) | Z R^T] is
//                           never stored: each 32 x 32 tile of it is itself a product over the label columns, formed on the matrix
//                           instruction into LDS and consumed from there as the A operand of the feature product.
// No floating-point atomics and no data-dependent order anywhere: a second call gives the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vd_nfr.h"

typedef double f64x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int TM = 32;             // rows / columns of a tile (2 x 2 waves of 16 x 16 MFMA blocks)
constexpr int KC = 32;             // contraction elements per LDS stage
constexpr int KP = KC + 1;         // padded LDS row (doubles)
constexpr int DT = 64;             // feature columns of a gradient tile (two 16-wide blocks per wave)
constexpr int FP = DT + 1;
constexpr int CB = 8;              // label columns per solve workgroup
constexpr int WS_HEAD = 2;         // status word and lambda in front of L

// [F_s ; F_t] F_s^T: rows < n go to K (n x n), the others to K_t (m x n).
__global__ __launch_bounds__(256) void nfr_gram_kernel(const float* __restrict__ fs, const float* __restrict__ ft, int n, int64_t m,
                                                       int d, double* __restrict__ K, double* __restrict__ Kt) {
    const int64_t r0 = (int64_t)blockIdx.x * TM;
    const int c0 = blockIdx.y * TM;
    if (r0 + TM <= n && (int64_t)c0 > r0) return;       // a tile of K strictly above the diagonal (uniform over the workgroup)
    __shared__ double sA[TM * KP], sB[TM * KP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int64_t rows = (int64_t)n + m;
    float ra[4], rb[4];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = tid + 256 * u, r = e >> 5, dd = k0 + (e & 31);
            const int64_t row = r0 + r;
            const int col = c0 + r;
            float va = 0.f, vb = 0.f;
            if (dd < d) {
                if (row < n) va = fs[row * d + dd];
                else if (row < rows) va = ft[(row - n) * d + dd];
                if (col < n) vb = fs[(int64_t)col * d + dd];
            }
            ra[u] = va;
            rb[u] = vb;
        }
    };
    f64x4 acc = {0.0, 0.0, 0.0, 0.0};
    fetch(0);
    for (int k0 = 0; k0 < d; k0 += KC) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = tid + 256 * u;
            sA[(e >> 5) * KP + (e & 31)] = (double)ra[u];
            sB[(e >> 5) * KP + (e & 31)] = (double)rb[u];
        }
        __syncthreads();
        if (k0 + KC < d) fetch(k0 + KC);
#pragma unroll
        for (int k = 0; k < KC; k += 4) {
            // A[i][k] = row i of the row tile, B[k][j] = row j of the column tile (operand map as in coreset_gram_kernel)
            const double a = sA[(wr * 16 + (lane & 15)) * KP + k + (lane >> 4)];
            const double b = sB[(wc * 16 + (lane & 15)) * KP + k + (lane >> 4)];
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
        }
        __syncthreads();
    }
    // f64 C/D map: col = lane & 15, row = (lane >> 4) + 4 * reg
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t row = r0 + wr * 16 + (lane >> 4) + 4 * r;
        const int col = c0 + wc * 16 + (lane & 15);
        if (col < n) {
            if (row < n) K[row * n + col] = acc[r];
            else if (row < rows) Kt[(row - n) * n + col] = acc[r];
        }
    }
}

// lambda, then A = K + lambda I = L L^T in place (ws + WS_HEAD), L^T mirrored above the diagonal.  One workgroup.
template <bool IN_LDS>
__global__ __launch_bounds__(1024) void nfr_factor_kernel(double* __restrict__ ws, int n, double reg) {
    extern __shared__ double sm[];
    double* Lg = ws + WS_HEAD;
    double* dg = sm;                                       // [VDN_MAX_SYN] the diagonal of K
    const int ld = IN_LDS ? (n | 1) : n;
    double* A = IN_LDS ? sm + VDN_MAX_SYN : Lg;
    const int tid = threadIdx.x;
    for (int j = tid; j < n; j += 1024) dg[j] = Lg[(int64_t)j * n + j];
    __syncthreads();
    double tr = 0.0;
    for (int j = 0; j < n; ++j) tr += dg[j];               // index order, the same in every thread
    const double lambda = __builtin_fabs(reg) * tr / (double)n;
    if (IN_LDS) {
        for (int e = tid; e < n * n; e += 1024) {
            const int i = e / n, j = e % n;
            if (j <= i) A[i * ld + j] = Lg[e] + (i == j ? lambda : 0.0);
        }
    } else {
        for (int j = tid; j < n; j += 1024) A[(int64_t)j * ld + j] = dg[j] + lambda;
    }
    __syncthreads();
    const int tr_ = tid >> 5, tc = tid & 31;                // 32 rows x 32 columns of the trailing block per pass
    for (int k = 0; k < n; ++k) {
        const double p = A[(int64_t)k * ld + k];
        if (!(p > 0.0 && p < __builtin_huge_val())) {     // (uniform: every thread reads the same pivot)
            if (tid == 0) {
                reinterpret_cast<int64_t*>(ws)[0] = (int64_t)k + 1;
                ws[1] = lambda;
            }
            return;
        }
        const double dk = __builtin_sqrt(p);
        __syncthreads();                                   // every thread has read the pivot
        for (int i = k + tid; i < n; i += 1024) {
            const double v = i == k ? dk : A[(int64_t)i * ld + k] / dk;
            A[(int64_t)i * ld + k] = v;
            A[(int64_t)k * ld + i] = v;
        }
        __syncthreads();
        for (int i = k + 1 + tr_; i < n; i += 32) {
            const double lik = A[(int64_t)i * ld + k];
            for (int j = k + 1 + tc; j <= i; j += 32) A[(int64_t)i * ld + j] -= lik * A[(int64_t)k * ld + j];
        }
        __syncthreads();
    }
    if (IN_LDS)
        for (int e = tid; e < n * n; e += 1024) Lg[e] = A[(e / n) * ld + e % n];
    if (tid == 0) {
        reinterpret_cast<int64_t*>(ws)[0] = 0;
        ws[1] = lambda;
    }
}

// C (M x N) = op(A) (M x Kd) B (Kd x N) in fp64 on the matrix instruction, one workgroup per 32 x 32 tile; NaN when the status
// word is set.  TRANS_A false: A is M x Kd row major (pred = K_t Z); true: A is Kd x M row major (g_Z = K_t^T R, B the fp32 R).
template <bool TRANS_A, typename TB>
__global__ __launch_bounds__(256) void nfr_product_kernel(const int64_t* __restrict__ status, const double* __restrict__ A,
                                                          const TB* __restrict__ B, int64_t M, int N, int64_t Kd,
                                                          double* __restrict__ out) {
    __shared__ double sA[KC * KP], sB[KC * KP];          // both [k][row or column of the tile]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int64_t r0 = (int64_t)blockIdx.x * TM;
    const int c0 = blockIdx.y * TM;
    const bool failed = *status != 0;
    f64x4 acc = {0.0, 0.0, 0.0, 0.0};
    for (int64_t k0 = 0; k0 < Kd && !failed; k0 += KC) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = tid + 256 * u, hi = e >> 5, lo = e & 31;
            // A: the contiguous index of the source is the fast index of the lanes; B: N is contiguous
            const int kk = TRANS_A ? hi : lo, mm = TRANS_A ? lo : hi;
            double va = 0.0, vb = 0.0;
            if (k0 + kk < Kd && r0 + mm < M) va = TRANS_A ? A[(k0 + kk) * M + r0 + mm] : A[(r0 + mm) * Kd + k0 + kk];
            if (k0 + hi < Kd && c0 + lo < N) vb = (double)B[(k0 + hi) * N + c0 + lo];
            sA[kk * KP + mm] = va;
            sB[hi * KP + lo] = vb;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < KC; k += 4) {
            const double a = sA[(k + (lane >> 4)) * KP + wr * 16 + (lane & 15)];
            const double b = sB[(k + (lane >> 4)) * KP + wc * 16 + (lane & 15)];
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
        }
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t row = r0 + wr * 16 + (lane >> 4) + 4 * r;
        const int col = c0 + wc * 16 + (lane & 15);
        if (row < M && col < N) out[row * N + col] = failed ? __builtin_nan("") : acc[r];
    }
}

// A^-1 of 8 right-hand-side columns, in place in x (n x C, fp64): forward the columns of Y_s (fp32, read from rhs) -> Z,
// backward the columns of g_Z = K_t^T R that nfr_product_kernel left in x -> Q.  NaN when the status word is set.
template <bool IN_LDS, bool BWD>
__global__ __launch_bounds__(256) void nfr_solve_kernel(const int64_t* __restrict__ status, const double* __restrict__ Lg,
                                                        const float* __restrict__ rhs, int n, int C, double* __restrict__ x) {
    extern __shared__ double sm[];
    const int tid = threadIdx.x, cc = tid & (CB - 1), ig = tid >> 3;
    const int64_t col = (int64_t)blockIdx.x * CB + cc;
    const bool valid = col < C;
    if (*status != 0) {
        if (valid)
            for (int i = ig; i < n; i += 32) x[(int64_t)i * C + col] = __builtin_nan("");
        return;
    }
    double* z = sm;                          // [n][CB]
    double* w = z + n * CB;                  // [n][CB]
    const int ld = IN_LDS ? (n | 1) : n;
    double* Ls = w + n * CB;                 // [n][ld] when IN_LDS
    const double* L = IN_LDS ? Ls : Lg;
    for (int i = ig; i < n; i += 32) {
        double s = 0.0;
        if (valid) s = BWD ? x[(int64_t)i * C + col] : (double)rhs[(int64_t)i * C + col];
        z[i * CB + cc] = s;
    }
    if (IN_LDS)
        for (int e = tid; e < n * n; e += 256) Ls[(e / n) * ld + e % n] = Lg[e];
    __syncthreads();
    for (int k = 0; k < n; ++k) {                                    // L y = b, by the rows of L^T
        const double* Uk = L + (int64_t)k * ld;
        const double zk = z[k * CB + cc] / Uk[k];
        for (int i = k + 1 + ig; i < n; i += 32) z[i * CB + cc] -= Uk[i] * zk;
        if (ig == 0) w[k * CB + cc] = zk;
        __syncthreads();
    }
    for (int i = n - 1; i >= 0; --i) {                               // L^T x = y, by the rows of L
        const double* Li = L + (int64_t)i * ld;
        const double xi = w[i * CB + cc] / Li[i];
        for (int k = ig; k < i; k += 32) w[k * CB + cc] -= Li[k] * xi;
        if (ig == 0) z[i * CB + cc] = xi;
        __syncthreads();
    }
    if (!valid) return;
    for (int i = ig; i < n; i += 32) x[(int64_t)i * C + col] = z[i * CB + cc];
}

// dl/dF_s = [M_s | M_t] [F_s ; F_t] + 2 c F_s, M_s = -(Q Z^T + Z Q^T), M_t = Z R^T, c = -(|reg| / n) sum Q . Z.
__global__ __launch_bounds__(256) void nfr_grad_kernel(const float* __restrict__ fs, const float* __restrict__ ft,
                                                       const float* __restrict__ R, const int64_t* __restrict__ status,
                                                       const double* __restrict__ Z, const double* __restrict__ Q, int n, int64_t m,
                                                       int d, int C, double reg, double* __restrict__ out) {
    __shared__ double sQi[TM * KP], sZi[TM * KP], sX[TM * KP], sY[TM * KP], sA[TM * KP], sF[TM * FP], red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int i0 = blockIdx.y * TM;
    const int64_t d0 = (int64_t)blockIdx.x * DT;
    if (*status != 0) {
        for (int e = tid; e < TM * DT; e += 256) {
            const int row = i0 + e / DT;
            const int64_t col = d0 + e % DT;
            if (row < n && col < d) out[(int64_t)row * d + col] = __builtin_nan("");
        }
        return;
    }
    // tr(G) = -sum Q . Z: a fixed assignment and a fixed tree, the same in every workgroup
    double part = 0.0;
    for (int64_t e = tid; e < (int64_t)n * C; e += 256) part += Q[e] * Z[e];
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) part += __shfl_xor(part, s, 64);
    if (lane == 0) red[wave] = part;
    __syncthreads();
    const double two_c = -2.0 * (__builtin_fabs(reg) / (double)n) * (((red[0] + red[1]) + red[2]) + red[3]);

    f64x4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
    const int64_t nks = (n + TM - 1) / TM, nkt = (m + TM - 1) / TM;
    for (int64_t kt = 0; kt < nks + nkt; ++kt) {
        const bool is_s = kt < nks;
        const int64_t kb = (is_s ? kt : kt - nks) * TM;      // first row of this stage in F_s / F_t
        const int64_t klim = is_s ? (int64_t)n : m;
        // the 32 x 32 tile of M at rows i0.., columns kb..: a product over the label columns
        f64x4 accM = {0.0, 0.0, 0.0, 0.0};
        for (int cb = 0; cb < C; cb += KC) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int e = tid + 256 * u, r = e >> 5, q = e & 31, ccol = cb + q;
                const bool oki = ccol < C && i0 + r < n, okk = ccol < C && kb + r < klim;
                const int64_t ai = (int64_t)(i0 + r) * C + ccol, ak = (kb + r) * C + ccol;
                sQi[r * KP + q] = oki ? Q[ai] : 0.0;
                sZi[r * KP + q] = oki ? Z[ai] : 0.0;
                sX[r * KP + q] = okk ? (is_s ? Z[ak] : (double)R[ak]) : 0.0;
                sY[r * KP + q] = okk && is_s ? Q[ak] : 0.0;
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < KC; q += 4) {
                const int ia = (wr * 16 + (lane & 15)) * KP + q + (lane >> 4), ib = (wc * 16 + (lane & 15)) * KP + q + (lane >> 4);
                if (is_s) {
                    accM = __builtin_amdgcn_mfma_f64_16x16x4f64(sQi[ia], sX[ib], accM, 0, 0, 0);      // Q_i . Z_k
                    accM = __builtin_amdgcn_mfma_f64_16x16x4f64(sZi[ia], sY[ib], accM, 0, 0, 0);      // Z_i . Q_k
                } else {
                    accM = __builtin_amdgcn_mfma_f64_16x16x4f64(sZi[ia], sX[ib], accM, 0, 0, 0);      // Z_i . R_k
                }
            }
            __syncthreads();
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
            sA[(wr * 16 + (lane >> 4) + 4 * r) * KP + wc * 16 + (lane & 15)] = is_s ? -accM[r] : accM[r];
        const float* f = is_s ? fs : ft;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int e = tid + 256 * u, r = e >> 6, q = e & 63;
            const int64_t row = kb + r, col = d0 + q;
            sF[r * FP + q] = (row < klim && col < d) ? (double)f[row * d + col] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < KC; q += 4) {
            const double a = sA[(wr * 16 + (lane & 15)) * KP + q + (lane >> 4)];
            const int ib = (q + (lane >> 4)) * FP + wc * 32 + (lane & 15);
            acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, sF[ib], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, sF[ib + 16], acc1, 0, 0, 0);
        }
        // (the next stage writes sA and sF only after the two barriers of its label loop: C >= 1)
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = i0 + wr * 16 + (lane >> 4) + 4 * r;
        const int64_t col = d0 + wc * 32 + (lane & 15);
        if (row < n) {
            const int64_t o = (int64_t)row * d + col;
            if (col < d) out[o] = acc0[r] + two_c * (double)fs[o];
            if (col + 16 < d) out[o + 16] = acc1[r] + two_c * (double)fs[o + 16];
        }
    }
}

bool bad_dims(int n, int m, int d, int c) { return n < 1 || n > VDN_MAX_SYN || m < 1 || d < 1 || c < 1; }

template <typename Kern>
hipError_t allow_lds(Kern kern, size_t bytes) {
    if (bytes <= 64 * 1024) return hipSuccess;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

size_t solve_lds_bytes(int n) {
    return ((size_t)2 * n * CB + (n <= VDN_LDS_SYN ? (size_t)n * (n | 1) : 0)) * sizeof(double);
}

template <bool BWD>
hipError_t launch_solve(const double* ws, const float* rhs, int n, int c, double* x, hipStream_t st) {
    const int64_t* status = reinterpret_cast<const int64_t*>(ws);
    const double* L = ws + WS_HEAD;
    const size_t lds = solve_lds_bytes(n);
    const dim3 grid((unsigned)((c + CB - 1) / CB)), block(256);
    hipError_t e;
    if (n <= VDN_LDS_SYN) {
        if ((e = allow_lds(nfr_solve_kernel<true, BWD>, lds)) != hipSuccess) return e;
        hipLaunchKernelGGL((nfr_solve_kernel<true, BWD>), grid, block, lds, st, status, L, rhs, n, c, x);
    } else {
        if ((e = allow_lds(nfr_solve_kernel<false, BWD>, lds)) != hipSuccess) return e;
        hipLaunchKernelGGL((nfr_solve_kernel<false, BWD>), grid, block, lds, st, status, L, rhs, n, c, x);
    }
    return hipGetLastError();
}

dim3 tile_grid(int64_t rows, int cols) { return dim3((unsigned)((rows + TM - 1) / TM), (unsigned)((cols + TM - 1) / TM)); }

}  // namespace

extern "C" int64_t vdn_nfr_workspace_bytes(int n, int m, int d, int c) {
    if (bad_dims(n, m, d, c)) return -1;
    return (WS_HEAD + (int64_t)n * n + (int64_t)n * c + (int64_t)m * n) * (int64_t)sizeof(double);
}

extern "C" int vdn_nfr_forward(const float* feat_syn, const float* y_syn, const float* feat_tar, int n, int m, int d, int c,
                               double reg, void* workspace, double* pred, void* stream) {
    if (feat_syn == nullptr || y_syn == nullptr || feat_tar == nullptr || workspace == nullptr || pred == nullptr) return -1;
    if (bad_dims(n, m, d, c)) return -1;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    double* ws = reinterpret_cast<double*>(workspace);
    double* L = ws + WS_HEAD;
    double* Z = L + (int64_t)n * n;
    double* Kt = Z + (int64_t)n * c;
    const int64_t rows = (int64_t)n + m;
    hipLaunchKernelGGL(nfr_gram_kernel, tile_grid(rows, n), dim3(256), 0, st, feat_syn, feat_tar, n, (int64_t)m, d, L, Kt);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return -(int)e;
    if (n <= VDN_LDS_SYN) {
        const size_t lds = ((size_t)VDN_MAX_SYN + (size_t)n * (n | 1)) * sizeof(double);
        if ((e = allow_lds(nfr_factor_kernel<true>, lds)) != hipSuccess) return -(int)e;
        hipLaunchKernelGGL(nfr_factor_kernel<true>, dim3(1), dim3(1024), lds, st, ws, n, reg);
    } else {
        hipLaunchKernelGGL(nfr_factor_kernel<false>, dim3(1), dim3(1024), VDN_MAX_SYN * sizeof(double), st, ws, n, reg);
    }
    if ((e = hipGetLastError()) != hipSuccess) return -(int)e;
    if ((e = launch_solve<false>(ws, y_syn, n, c, Z, st)) != hipSuccess) return -(int)e;
    hipLaunchKernelGGL((nfr_product_kernel<false, double>), tile_grid(m, c), dim3(256), 0, st, reinterpret_cast<const int64_t*>(ws), Kt,
                       Z, (int64_t)m, c, (int64_t)n, pred);
    e = hipGetLastError();
    return e == hipSuccess ? 0 : -(int)e;
}

extern "C" int vdn_nfr_backward(const float* feat_syn, const float* feat_tar, const float* g_pred, int n, int m, int d, int c,
                                double reg, const void* workspace, double* g_feat_syn, double* g_y_syn, void* stream) {
    if (feat_syn == nullptr || feat_tar == nullptr || g_pred == nullptr || workspace == nullptr || g_feat_syn == nullptr ||
        g_y_syn == nullptr)
        return -1;
    if (bad_dims(n, m, d, c)) return -1;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const double* ws = reinterpret_cast<const double*>(workspace);
    const double* Z = ws + WS_HEAD + (int64_t)n * n;
    const double* Kt = Z + (int64_t)n * c;
    hipLaunchKernelGGL((nfr_product_kernel<true, float>), tile_grid(n, c), dim3(256), 0, st, reinterpret_cast<const int64_t*>(ws), Kt,
                       g_pred, (int64_t)n, c, (int64_t)m, g_y_syn);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return -(int)e;
    if ((e = launch_solve<true>(ws, nullptr, n, c, g_y_syn, st)) != hipSuccess) return -(int)e;
    hipLaunchKernelGGL(nfr_grad_kernel, dim3((unsigned)((d + DT - 1) / DT), (unsigned)((n + TM - 1) / TM)), dim3(256), 0, st, feat_syn,
                       feat_tar, g_pred, reinterpret_cast<const int64_t*>(ws), Z, g_y_syn, n, (int64_t)m, d, c, reg, g_feat_syn);
    e = hipGetLastError();
    return e == hipSuccess ? 0 : -(int)e;
}
