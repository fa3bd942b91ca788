// The regression train step's two helper kernels (include/vd_frepo.h has the contract and the formulas as they are evaluated):
//
//   vdf_mse_loss     nn.MSELoss() (mean) and its logit gradient, one launch.  Every workgroup writes its grid-stride share of
//                    dlogits in fp32; workgroup 0 also sums the squared differences in fp64 -- thread-strided partial sums
//                    in four accumulators walked in a fixed order, then a fixed LDS tree -- and rounds the mean to float once.
//   vdf_adam_multi   one Adam / AdamW step over up to VDF_ADAM_MAX tensors in one launch: the batch travels by value in the
//                    kernel arguments with a first-workgroup index per segment (as VdPackBatch does), a workgroup finds its
//                    segment by a block-uniform walk over those indices and grid-strides inside it.  HBM-bound: four streams
//                    read, three written; 16-byte accesses on the aligned body, 4-byte ones on head and tail.
//
// No floating-point atomics, no host synchronisation; argument checks come before any HIP call.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vd_frepo.h"

namespace {

constexpr int MSE_THREADS = 1024;
constexpr int MSE_MAX_BLOCKS = 256;

__global__ __launch_bounds__(MSE_THREADS) void mse_loss_kernel(const float* __restrict__ logits, const float* __restrict__ targets,
                                                                int64_t n, float scale, double inv_n, float* __restrict__ loss,
                                                                float* __restrict__ dlogits) {
    const int64_t stride = (int64_t)gridDim.x * MSE_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * MSE_THREADS + threadIdx.x; i < n; i += stride) {
        // the difference and the product each rounded on their own: the fp32 evaluation of the header's line as written
#pragma clang fp contract(off)
        const float d = logits[i] - targets[i];
        dlogits[i] = d * scale;
    }
    if (blockIdx.x != 0) return;
    __shared__ double part[MSE_THREADS];
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    int64_t i = threadIdx.x;
    for (; i + 3 * MSE_THREADS < n; i += 4 * MSE_THREADS) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const double d = (double)logits[i + u * MSE_THREADS] - (double)targets[i + u * MSE_THREADS];
            a[u] += d * d;
        }
    }
    for (int u = 0; i < n; i += MSE_THREADS, ++u) {
        const double d = (double)logits[i] - (double)targets[i];
        a[u & 3] += d * d;
    }
    part[threadIdx.x] = (a[0] + a[1]) + (a[2] + a[3]);
    __syncthreads();
    for (int s = MSE_THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = (float)(part[0] * inv_n);
}

constexpr int ADAM_THREADS = 256;
constexpr int ADAM_CHUNK = ADAM_THREADS * 4;          // floats one workgroup moves per grid-stride iteration of the 16-byte body
constexpr int ADAM_MAX_BLOCKS = 2048;          // 256 CUs x 8 workgroups: the streaming-kernel grid of the chip

struct AdamConsts {
    float beta1, one_minus_beta1, beta2, one_minus_beta2, bc2_sqrt, eps, step_size, lr_wd;
};

// One element of the header's formula.  Every operation rounded on its own, in the header's order.
__device__ __forceinline__ void adam_one(float& p, float& m, float& v, const float g, const AdamConsts& c) {
#pragma clang fp contract(off)
    float pw = p;
    if (c.lr_wd != 0.f) {
        const float keep = 1.f - c.lr_wd;
        pw = pw * keep;
    }
    const float dm = g - m;
    const float tm = c.one_minus_beta1 * dm;
    const float mn = m + tm;
    const float av = c.beta2 * v;
    const float gg = g * g;
    const float bv = c.one_minus_beta2 * gg;
    const float vn = av + bv;
    const float s = sqrtf(vn);
    const float q = s / c.bc2_sqrt;
    const float den = q + c.eps;
    const float num = c.step_size * mn;
    const float u = num / den;
    p = pw - u;
    m = mn;
    v = vn;
}

__global__ __launch_bounds__(ADAM_THREADS) void adam_multi_kernel(const VdfAdamBatch b) {
    int k = 0;
#pragma unroll 1
    while (k + 1 < b.nseg && (int)blockIdx.x >= b.seg[k + 1].first_block) ++k;      // (block-uniform: scalar loads of the kernel arguments)
    const VdfAdamSeg& sg = b.seg[k];
    const int nb = (k + 1 < b.nseg ? b.seg[k + 1].first_block : (int)gridDim.x) - sg.first_block;      // workgroups of this segment
    const int j = (int)blockIdx.x - sg.first_block;
    const AdamConsts c = {b.beta1, b.one_minus_beta1, b.beta2, b.one_minus_beta2, b.bc2_sqrt, b.eps, sg.step_size, sg.lr_wd};
    float* __restrict__ p = sg.p;
    float* __restrict__ m = sg.m;
    float* __restrict__ v = sg.v;
    const float* __restrict__ g = sg.g;
    const int64_t n = sg.n;
    const unsigned off = (unsigned)((uintptr_t)p & 15u);
    const bool same = (((uintptr_t)m & 15u) == off) && (((uintptr_t)v & 15u) == off) && (((uintptr_t)g & 15u) == off);
    if (!same) {      // the four streams disagree about where a 16-byte line starts: 4-byte accesses throughout
        for (int64_t i = (int64_t)j * ADAM_THREADS + threadIdx.x; i < n; i += (int64_t)nb * ADAM_THREADS) {
            float pv = p[i], mv = m[i], vv = v[i];
            adam_one(pv, mv, vv, g[i], c);
            p[i] = pv; m[i] = mv; v[i] = vv;
        }
        return;
    }
    int64_t head = (int64_t)((4u - (off >> 2)) & 3u);      // floats in front of the first 16-byte boundary
    if (head > n) head = n;
    const int64_t quads = (n - head) >> 2;
    const int64_t tail0 = head + (quads << 2);
    float4* __restrict__ p4 = reinterpret_cast<float4*>(p + head);
    float4* __restrict__ m4 = reinterpret_cast<float4*>(m + head);
    float4* __restrict__ v4 = reinterpret_cast<float4*>(v + head);
    const float4* __restrict__ g4 = reinterpret_cast<const float4*>(g + head);
    for (int64_t q = (int64_t)j * ADAM_THREADS + threadIdx.x; q < quads; q += (int64_t)nb * ADAM_THREADS) {
        float4 pv = p4[q], mv = m4[q], vv = v4[q];
        const float4 gv = g4[q];
        adam_one(pv.x, mv.x, vv.x, gv.x, c);
        adam_one(pv.y, mv.y, vv.y, gv.y, c);
        adam_one(pv.z, mv.z, vv.z, gv.z, c);
        adam_one(pv.w, mv.w, vv.w, gv.w, c);
        p4[q] = pv; m4[q] = mv; v4[q] = vv;
    }
    if (j == 0 && threadIdx.x < 8) {      // head (threads 0..3) and tail (threads 4..7) of the segment: at most 3 floats each
        const int t = (int)threadIdx.x;
        const int64_t i = t < 4 ? (int64_t)t : tail0 + (t - 4);
        const bool live = t < 4 ? (int64_t)t < head : i < n;
        if (live) {
            float pv = p[i], mv = m[i], vv = v[i];
            adam_one(pv, mv, vv, g[i], c);
            p[i] = pv; m[i] = mv; v[i] = vv;
        }
    }
}

}  // namespace

extern "C" int vdf_mse_loss(const float* logits, const float* targets, int B, int K, float* loss, float* dlogits, void* stream) {
    if (logits == nullptr || targets == nullptr || loss == nullptr || dlogits == nullptr) return -1;
    if (B <= 0 || K <= 0) return -1;
    const int64_t n = (int64_t)B * K;
    int64_t blocks = (n + MSE_THREADS - 1) / MSE_THREADS;
    if (blocks > MSE_MAX_BLOCKS) blocks = MSE_MAX_BLOCKS;
    const double inv_n = 1.0 / (double)n;
    const float scale = (float)(2.0 / (double)n);
    hipLaunchKernelGGL(mse_loss_kernel, dim3((unsigned)blocks), dim3(MSE_THREADS), 0, reinterpret_cast<hipStream_t>(stream), logits,
                       targets, n, scale, inv_n, loss, dlogits);
    return (int)hipGetLastError();
}

extern "C" int vdf_adam_multi(const VdfAdamBatch* batch, void* stream) {
    if (batch == nullptr || batch->nseg < 1 || batch->nseg > VDF_ADAM_MAX) return -1;
    int64_t want_total = 0;
    for (int k = 0; k < batch->nseg; ++k) {
        const VdfAdamSeg& sg = batch->seg[k];
        if (sg.p == nullptr || sg.m == nullptr || sg.v == nullptr || sg.g == nullptr || sg.n <= 0) return -1;
        want_total += (sg.n + ADAM_CHUNK - 1) / ADAM_CHUNK;
    }
    VdfAdamBatch b = *batch;
    int64_t blocks = 0;
    for (int k = 0; k < b.nseg; ++k) {      // one workgroup per chunk while the chip has room, otherwise a share of the grid by length
        const int64_t want = (b.seg[k].n + ADAM_CHUNK - 1) / ADAM_CHUNK;
        int64_t nb = want_total <= ADAM_MAX_BLOCKS ? want : (int64_t)((double)want * (double)ADAM_MAX_BLOCKS / (double)want_total);
        if (nb < 1) nb = 1;
        if (nb > want) nb = want;
        b.seg[k].first_block = (int32_t)blocks;
        blocks += nb;
    }
    hipLaunchKernelGGL(adam_multi_kernel, dim3((unsigned)blocks), dim3(ADAM_THREADS), 0, reinterpret_cast<hipStream_t>(stream), b);
    return (int)hipGetLastError();
}
