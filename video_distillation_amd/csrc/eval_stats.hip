// vd_eval_stats: the statistics utils.epoch('test') keeps per batch (utils.py:793-824 of the reference: loss, top-1 / top-3 / top-5
// hits, hits and clips per class) as ONE launch that accumulates into a fixed-layout fp64 record (include/vd_hip.h), so that a
// test pass dealt to another rank comes back as a tensor an all-reduce can carry (evalpool.py).
//
// One workgroup of 16 waves for the whole batch (B <= 256 clips of K <= 400 logits in evaluation: the launch is latency-bound,
// and one workgroup needs neither a scratch buffer nor a ticket to form the batch's cross-entropy sum in a fixed order).  Wave w
// takes clips w, w + 16, ...: row maximum, fp64 log-sum-exp as ce_loss_kernel does, and the label's rank = the number of
// classes with a strictly greater logit plus the number with an equal logit at a lower index -- a pure function of the fp32
// logits, so top-1 is argmax-with-first-maximum == label, and top-k is rank < k.  Lane 0 of each wave keeps the wave's sums in
// registers; thread 0 folds the 16 waves in index order and adds the result to the record.  The per-class slots take one fp64
// atomic add per clip (integers: exact in any order).  A record is therefore bitwise reproducible.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vd_hip.h"

namespace {

constexpr int WAVES = 16;
constexpr int NSUM = 6;       // record slots 0..5: clips, sum of CE, top-1, top-3, top-5, labels out of range

__device__ inline double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(WAVES * 64) void eval_stats_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                                int B, int K, double* __restrict__ rec) {
    __shared__ double part[WAVES][NSUM];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
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
        float m = -3.402823466e38f;
        int above = 0;
        for (int k = lane; k < K; k += 64) {
            const float v = z[k];
            m = fmaxf(m, v);
            above += (v > zy || (v == zy && k < y)) ? 1 : 0;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            m = fmaxf(m, __shfl_xor(m, o, 64));
            above += __shfl_xor(above, o, 64);
        }
        double sum = 0.0;
        for (int k = lane; k < K; k += 64) sum += exp((double)z[k] - (double)m);
        sum = wave_sum_f64(sum);
        if (lane == 0) {
            acc[0] += 1.0;
            acc[1] += ((double)m + log(sum)) - (double)zy;
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

extern "C" int vd_eval_stats(const float* logits, const int64_t* labels, int B, int K, double* rec, void* stream) {
    if (B < 0 || K < 1) return -1;
    if (B == 0) return 0;
    if (logits == nullptr || labels == nullptr || rec == nullptr) return -1;
    hipLaunchKernelGGL(eval_stats_kernel, dim3(1), dim3(WAVES * 64), 0, reinterpret_cast<hipStream_t>(stream), logits, labels, B, K,
                       rec);
    return (int)hipGetLastError();
}
