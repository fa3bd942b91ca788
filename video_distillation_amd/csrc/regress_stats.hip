// vdr_regress_stats: the statistics FRePo's epoch('test') keeps per batch (lib_torch/utils.py:522-560 of the reference: the MSE
// against the soft labels one_hot - 1/K and the argmax accuracy) as ONE launch that accumulates into the fixed-layout fp64 record
// of vd_eval_stats (include/vd_regress.h), so that evalpool.py deals FRePo's test passes over ranks as it deals the cross-entropy
// ones.
//
// The shape of eval_stats.hip: one workgroup of 16 waves for the whole batch (B <= 256 clips of K <= 400 logits: the launch is
// latency-bound), no scratch buffer, no LDS beyond the per-wave partials.  Wave w takes clips w, w + 16, ...; lane l takes classes
// l, l + 64, ... of a clip: the squared differences in fp64, added in ascending k, and the label's rank.  The order of every
// addition that reaches rec[1] is fixed:
//
//   per lane      ceil(K / 64) terms in ascending k                  (starting from 0.0)
//   per clip      the 6-step xor butterfly over the 64 lanes         (every lane ends with the same bits)
//   per wave      its ceil(B / 16) clips in ascending order          (lane 0, starting from 0.0)
//   per batch     the 16 waves in index order                        (one thread, starting from 0.0)
//   record        rec[1] += that                                     (the same thread)
//
// so the longest chain of additions behind any term is ceil(K / 64) + 6 + ceil(B / 16) + 16 + 1 (tests/test_gpu_regress_stats.py
// derives its bound from this).  The counts are integers in fp64: exact in any order, the per-class ones by one atomic add per clip.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vd_regress.h"

namespace {

constexpr int WAVES = 16;
constexpr int NSUM = 6;       // record slots 0..5: clips, sum of squared errors, top-1, top-3, top-5, labels out of range

__global__ __launch_bounds__(WAVES * 64) void regress_stats_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                                   int B, int K, float inv_k, double* __restrict__ rec) {
    __shared__ double part[WAVES][NSUM];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float y_on = 1.0f - inv_k, y_off = 0.0f - inv_k;      // one_hot - 1/K in fp32, as frepo.soft_labels forms it
    double acc[NSUM] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};          // (meaningful on lane 0)
    for (int clip = wave; clip < B; clip += WAVES) {
        const int64_t yl = labels[clip];
        if (yl < 0 || yl >= K) {               // counted in slot 5 and nowhere else
            acc[5] += 1.0;
            continue;
        }
        const int y = (int)yl;
        const float* z = logits + (int64_t)clip * K;
        const float zy = z[y];
        double se = 0.0;
        int above = 0;
        for (int k = lane; k < K; k += 64) {
            const float v = z[k];
            const double d = __dsub_rn((double)v, (double)(k == y ? y_on : y_off));
            se = __dadd_rn(se, __dmul_rn(d, d));          // (each rounded on its own: no contraction to a fused multiply-add)
            above += (v > zy || (v == zy && k < y)) ? 1 : 0;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            se += __shfl_xor(se, o, 64);
            above += __shfl_xor(above, o, 64);
        }
        if (lane == 0) {
            acc[0] += 1.0;
            acc[1] += se;
            acc[2] += above < 1 ? 1.0 : 0.0;
            acc[3] += above < 3 ? 1.0 : 0.0;
            acc[4] += above < 5 ? 1.0 : 0.0;
            if (above < 1) atomicAdd(&rec[8 + y], 1.0);
            atomicAdd(&rec[8 + K + y], 1.0);
        }
    }
    if (lane == 0)
        for (int s = 0; s < NSUM; ++s) part[wave][s] = acc[s];
    __syncthreads();
    if (threadIdx.x < NSUM) {                  // one thread per slot; the waves in index order
        double t = 0.0;
        for (int w = 0; w < WAVES; ++w) t += part[w][threadIdx.x];
        rec[threadIdx.x] += t;
    }
}

}  // namespace

extern "C" int vdr_regress_stats(const float* logits, const int64_t* labels, int B, int K, double* rec, void* stream) {
    if (B < 0 || K < 1) return -1;
    if (B == 0) return 0;
    if (logits == nullptr || labels == nullptr || rec == nullptr) return -1;
    const float inv_k = (float)(1.0 / (double)K);
    hipLaunchKernelGGL(regress_stats_kernel, dim3(1), dim3(WAVES * 64), 0, reinterpret_cast<hipStream_t>(stream), logits, labels, B, K,
                       inv_k, rec);
    return (int)hipGetLastError();
}
