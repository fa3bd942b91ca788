// Coreset selection (herding and greedy k-center) on the centred Gram matrix of each class.
//
// Reference: distill_coreset.py:72-105 -- per class, embed every clip, then pick ipc clips by a per-step loop of torch ops.
// Both criteria are translation invariant, so they depend on the features only through the centred Gram matrix
// G~ = (F - m)(F - m)^T of the class (N x N, fp64):
//   herding   : pick argmin_{j not chosen} G~[j][j] + 2 sum_{s chosen} G~[s][j]        (||-sum_S f~_s - f~_j||^2 minus a constant)
//   k-center  : first pick argmin_j G~[j][j]; then argmax_{j not chosen} min_{c chosen} G~[j][j] + G~[c][c] - 2 G~[c][j]
// Ties go to the lowest index (torch's argmin / argmax).  Two launches, no host synchronisation:
//   1. coreset_gram_kernel  : one workgroup per (class, 32-row tile): the class mean in fp64 (into LDS), then the tiles
//                             (row tile, col tile <= row tile) of G~ on v_mfma_f64_16x16x4_f64, the features read as fp32 and
//                             centred in fp64 on load; both triangles are stored.
//   2. coreset_select_kernel: one workgroup per class runs all ipc steps, G~ held in LDS when it fits, streamed from the
//                             workspace otherwise.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vd_hip.h"

typedef double f64x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int TM = 32;             // rows of a Gram tile (2 x 2 waves of 16 x 16 MFMA blocks)
constexpr int KC = 32;             // feature elements per LDS stage
constexpr int KP = KC + 1;         // padded LDS row (doubles)
constexpr int LDS_MAX = 160 * 1024;

__global__ __launch_bounds__(256) void coreset_gram_kernel(const float* __restrict__ feats, int dim,
                                                           const int64_t* __restrict__ offsets, const int32_t* __restrict__ counts,
                                                           int max_count, double* __restrict__ gram) {
    const int c = blockIdx.y, it = blockIdx.x;
    const int n = counts[c];
    if (n <= 0 || n > max_count || it * TM >= n) return;       // (uniform over the workgroup)
    extern __shared__ double sm[];
    double* mean = sm;                                       // [dim]
    double* sA = sm + ((dim + 1) & ~1);                      // [TM][KP]
    double* sB = sA + TM * KP;                               // [TM][KP]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const float* f = feats + offsets[c] * (int64_t)dim;
    // class mean in fp64, clips summed in index order
    for (int d = tid; d < dim; d += 256) {
        double s = 0.0;
        for (int r = 0; r < n; ++r) s += (double)f[(int64_t)r * dim + d];
        mean[d] = s / (double)n;
    }
    __syncthreads();
    double* g = gram + (int64_t)c * max_count * max_count;
    for (int jt = 0; jt <= it; ++jt) {
        f64x4 acc = {0.0, 0.0, 0.0, 0.0};
        for (int k0 = 0; k0 < dim; k0 += KC) {
            for (int e = tid; e < TM * KC; e += 256) {
                const int r = e / KC, k = e % KC, d = k0 + k;
                const int ra = it * TM + r, rb = jt * TM + r;
                double va = 0.0, vb = 0.0;
                if (d < dim) {
                    if (ra < n) va = (double)f[(int64_t)ra * dim + d] - mean[d];
                    if (rb < n) vb = (double)f[(int64_t)rb * dim + d] - mean[d];
                }
                sA[r * KP + k] = va;
                sB[r * KP + k] = vb;
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < KC; k += 4) {
                // A[m][k] = centred row m of the row tile, B[k][n] = centred row n of the column tile (f32 16x16x4 operand map)
                const double a = sA[(wr * 16 + (lane & 15)) * KP + k + (lane >> 4)];
                const double b = sB[(wc * 16 + (lane & 15)) * KP + k + (lane >> 4)];
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
            }
            __syncthreads();
        }
        // f64 C/D map: col = lane & 15, row = (lane >> 4) + 4 * reg.  The diagonal tile stores its lower half and mirrors it, so
        // G~ is exactly symmetric.
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = it * TM + wr * 16 + (lane >> 4) + 4 * r;
            const int col = jt * TM + wc * 16 + (lane & 15);
            if (row < n && col < n && (jt < it || col <= row)) {
                g[(int64_t)row * max_count + col] = acc[r];
                g[(int64_t)col * max_count + row] = acc[r];
            }
        }
    }
}

__device__ __forceinline__ void argmin_pair(double& v, int& i, double ov, int oi) {
    if (ov < v || (ov == v && oi < i)) { v = ov; i = oi; }
}

__global__ __launch_bounds__(256) void coreset_select_kernel(const double* __restrict__ gram, const int64_t* __restrict__ offsets,
                                                             const int32_t* __restrict__ counts, int max_count, int ipc, int method,
                                                             int64_t lds_gram_cap, int64_t* __restrict__ out) {
    const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = counts[c];
    int64_t* o = out + (int64_t)c * ipc;
    if (n < ipc || n > max_count) {           // a short class (or a count the workspace was not sized for): -1 picks
        for (int t = tid; t < ipc; t += 256) o[t] = -1;
        return;
    }
    extern __shared__ double sm[];
    double* diag = sm;                                   // [max_count]
    double* vec = diag + max_count;                      // [max_count] herding: sum_S G~[s][j]; k-center: min distance^2
    double* wv = vec + max_count;                        // [4] per-wave best value
    double* lg = wv + 4;                                 // [n][n] when it fits
    int* wi = reinterpret_cast<int*>(lg + lds_gram_cap); // [4] per-wave best index
    int* chosen = wi + 4;                                // [max_count]
    const double* G = gram + (int64_t)c * max_count * max_count;
    const bool in_lds = (int64_t)n * n <= lds_gram_cap;
    if (in_lds)
        for (int e = tid; e < n * n; e += 256) lg[e] = G[(int64_t)(e / n) * max_count + e % n];
    for (int j = tid; j < n; j += 256) {
        diag[j] = G[(int64_t)j * max_count + j];
        vec[j] = method == VD_CORESET_HERDING ? 0.0 : __builtin_huge_val();
        chosen[j] = 0;
    }
    __syncthreads();
    const int64_t base = offsets[c];
    for (int t = 0; t < ipc; ++t) {
        // every criterion as an argmin: herding diag + 2 acc; k-center's first pick diag, later picks -(min distance)
        double bv = __builtin_huge_val();
        int bi = 0x7fffffff;
        for (int j = tid; j < n; j += 256) {
            if (chosen[j]) continue;
            const double v = method == VD_CORESET_HERDING ? diag[j] + 2.0 * vec[j] : (t == 0 ? diag[j] : -vec[j]);
            argmin_pair(bv, bi, v, j);
        }
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) {
            const double ov = __shfl_xor(bv, s, 64);
            const int oi = __shfl_xor(bi, s, 64);
            argmin_pair(bv, bi, ov, oi);
        }
        if (lane == 0) { wv[wave] = bv; wi[wave] = bi; }
        __syncthreads();
        bv = wv[0]; bi = wi[0];
        for (int w = 1; w < 4; ++w) argmin_pair(bv, bi, wv[w], wi[w]);
        const int p = bi;
        if (p < 0 || p >= n) {                  // no comparable candidate (non-finite features): the remaining picks are -1
            for (int u = t + tid; u < ipc; u += 256) o[u] = -1;
            return;
        }
        if (tid == 0) { o[t] = base + p; chosen[p] = 1; }
        const double* row = in_lds ? lg + (int64_t)p * n : G + (int64_t)p * max_count;
        const double dp = diag[p];
        for (int j = tid; j < n; j += 256) {
            if (method == VD_CORESET_HERDING) {
                vec[j] += row[j];
            } else {
                const double d = diag[j] + dp - 2.0 * row[j];
                vec[j] = d < vec[j] ? d : vec[j];
            }
        }
        __syncthreads();
    }
}

int64_t select_vec_bytes(int max_count) {        // diag + vec + 4 wave values (doubles), 4 wave indices + chosen flags (ints)
    return (2 * (int64_t)max_count + 4) * 8 + (4 + (int64_t)max_count) * 4;
}

}  // namespace

extern "C" int64_t vd_coreset_workspace_bytes(int nclass, int max_count) {
    if (nclass <= 0 || max_count <= 0 || max_count > VD_CORESET_MAX_COUNT) return -2;
    return (int64_t)nclass * max_count * max_count * (int64_t)sizeof(double);
}

extern "C" int vd_coreset_select(const float* feats, int dim, const int64_t* offsets, const int32_t* counts, int nclass,
                                 int max_count, int ipc, int method, int64_t* out_idx, void* workspace, int64_t workspace_bytes,
                                 void* stream) {
    if (feats == nullptr || offsets == nullptr || counts == nullptr || out_idx == nullptr || workspace == nullptr) return -1;
    if (dim <= 0 || dim > VD_CORESET_MAX_DIM || nclass <= 0 || max_count <= 0 || max_count > VD_CORESET_MAX_COUNT || ipc <= 0 ||
        (method != VD_CORESET_HERDING && method != VD_CORESET_KCENTER))
        return -2;
    if (workspace_bytes < vd_coreset_workspace_bytes(nclass, max_count)) return -2;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    double* gram = reinterpret_cast<double*>(workspace);
    const int lds_gram = (int)((((dim + 1) & ~1) + 2 * TM * KP) * sizeof(double));
    if (lds_gram > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void*)coreset_gram_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_gram);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(coreset_gram_kernel, dim3((unsigned)((max_count + TM - 1) / TM), (unsigned)nclass), dim3(256), lds_gram, st,
                       feats, dim, offsets, counts, max_count, gram);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    // LDS of the selection: the O(N) vectors, plus as much of G~ as fits (a class whose N x N block fits is served from LDS)
    const int64_t vec = select_vec_bytes(max_count);
    int64_t cap = (LDS_MAX - vec) / 8;
    if (cap > (int64_t)max_count * max_count) cap = (int64_t)max_count * max_count;
    if (cap < 0) cap = 0;
    const int lds_sel = (int)(vec + cap * 8);
    if (lds_sel > 64 * 1024) {
        e = hipFuncSetAttribute((const void*)coreset_select_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_sel);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(coreset_select_kernel, dim3((unsigned)nclass), dim3(256), lds_sel, st, gram, offsets, counts, max_count, ipc,
                       method, cap, out_idx);
    return (int)hipGetLastError();
}
