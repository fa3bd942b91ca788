// The flat-parameter chain of trajectory matching (include/vd_hip.h): the student update, the normalised distance with its
// adjoint seed, and one reverse step, each ONE pass over the 3.65 M-float parameter vector instead of a string of elementwise and
// reduction launches with a temporary apiece.
//
// All three are streaming kernels: float4 loads and stores, 256-thread workgroups, a grid-stride loop under a capped grid
// (MAX_BLOCKS workgroups cover BLOCK * MAX_BLOCKS * 4 = 2 097 152 floats per pass; longer vectors take more passes), the n % 4
// tail elements taken one each by the first threads of workgroup 0.
//
// Rounding: `#pragma clang fp contract(off)` in every body -- each fp32 (and fp64) operation is rounded on its own, as in
// sgd_momentum_kernel, so the elementwise outputs are the float32 evaluation of the header's formulas as written.
//
// Sums: fp64, fixed order.  A thread adds its elements in loop order, a wave folds its 64 lanes with the xor butterfly, lane 0 of
// the 4 waves leave their sums in LDS and thread 0 adds them in wave order: one partial per workgroup in `scratch`.  The grid is
// a function of n alone, so the partials are too.  A second launch of one workgroup adds the partials in index order (thread t
// the contiguous run t * per .. t * per + per - 1, then 16 threads 16 runs each, then thread 0 the 16) and applies the scalar
// update.  Nothing is handed between workgroups inside a launch and there is no atomic: the bits repeat from run to run.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vd_hip.h"

namespace {

constexpr int BLOCK = 256;
constexpr int MAX_BLOCKS = 2048;

inline int64_t grid_for(int64_t n) {
    const int64_t n4 = n / 4;
    int64_t blocks = (n4 + BLOCK - 1) / BLOCK;
    if (blocks < 1) blocks = 1;          // (n < 4: the tail alone)
    return blocks > MAX_BLOCKS ? MAX_BLOCKS : blocks;
}

inline bool misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) != 0; }
inline bool bad(const void* p) { return p == nullptr || misaligned(p); }

__device__ inline double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// the workgroup's sum of `acc` -> scratch[slot] (thread 0); `part` is LDS for the 4 waves
__device__ inline void block_partial(double acc, double* part, double* __restrict__ scratch, int64_t slot) {
    acc = wave_sum_f64(acc);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) scratch[slot] = ((part[0] + part[1]) + part[2]) + part[3];
    __syncthreads();
}

// sum of scratch[0 .. count) in index order, by one workgroup of BLOCK threads; the result is valid on thread 0
__device__ inline double fold_partials(const double* __restrict__ scratch, int count, double* lds) {
    const int per = (count + BLOCK - 1) / BLOCK;
    const int t = threadIdx.x;
    double s = 0.0;
    for (int k = t * per; k < (t + 1) * per && k < count; ++k) s += scratch[k];
    lds[t] = s;
    __syncthreads();
    if (t < 16) {
        double u = 0.0;
        for (int k = 0; k < 16; ++k) u += lds[t * 16 + k];
        lds[BLOCK + t] = u;
    }
    __syncthreads();
    double total = 0.0;
    if (t == 0)
        for (int k = 0; k < 16; ++k) total += lds[BLOCK + k];
    __syncthreads();
    return total;
}

__global__ __launch_bounds__(BLOCK) void traj_step_kernel(const float* __restrict__ theta, const float* __restrict__ g,
                                                          const float* __restrict__ lr_dev, int64_t n,
                                                          float* __restrict__ out) {
#pragma clang fp contract(off)
    const float lr = lr_dev[0];
    const int64_t n4 = n / 4;
    const int64_t stride = (int64_t)gridDim.x * BLOCK;
    const int64_t tid = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const float4* t4 = reinterpret_cast<const float4*>(theta);
    const float4* g4 = reinterpret_cast<const float4*>(g);
    float4* o4 = reinterpret_cast<float4*>(out);
    for (int64_t i = tid; i < n4; i += stride) {
        const float4 a = t4[i], b = g4[i];
        float4 r;
        r.x = a.x - lr * b.x;
        r.y = a.y - lr * b.y;
        r.z = a.z - lr * b.z;
        r.w = a.w - lr * b.w;
        o4[i] = r;
    }
    const int64_t j = n4 * 4 + tid;
    if (tid < 3 && j < n) out[j] = theta[j] - lr * g[j];
}

__device__ inline double sq_diff(float a, float b) {
#pragma clang fp contract(off)
    const double d = (double)a - (double)b;
    return d * d;
}

__global__ __launch_bounds__(BLOCK) void traj_dist_kernel(const float* __restrict__ theta, const float* __restrict__ theta0,
                                                          const float* __restrict__ target, int64_t n,
                                                          double* __restrict__ scratch) {
#pragma clang fp contract(off)
    __shared__ double part[4];
    const int64_t n4 = n / 4;
    const int64_t stride = (int64_t)gridDim.x * BLOCK;
    const int64_t tid = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const float4* a4 = reinterpret_cast<const float4*>(theta);
    const float4* b4 = reinterpret_cast<const float4*>(theta0);
    const float4* c4 = reinterpret_cast<const float4*>(target);
    double d1 = 0.0, d0 = 0.0;
    for (int64_t i = tid; i < n4; i += stride) {
        const float4 a = a4[i], b = b4[i], c = c4[i];
        d1 += sq_diff(a.x, c.x); d1 += sq_diff(a.y, c.y); d1 += sq_diff(a.z, c.z); d1 += sq_diff(a.w, c.w);
        d0 += sq_diff(b.x, c.x); d0 += sq_diff(b.y, c.y); d0 += sq_diff(b.z, c.z); d0 += sq_diff(b.w, c.w);
    }
    const int64_t j = n4 * 4 + tid;
    if (tid < 3 && j < n) {
        d1 += sq_diff(theta[j], target[j]);
        d0 += sq_diff(theta0[j], target[j]);
    }
    block_partial(d1, part, scratch, blockIdx.x);
    block_partial(d0, part, scratch, (int64_t)gridDim.x + blockIdx.x);
}

__global__ __launch_bounds__(BLOCK) void traj_dist_fold_kernel(const double* __restrict__ scratch, int count,
                                                               double* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ double lds[BLOCK + 16];
    const double dist = fold_partials(scratch, count, lds);
    const double dist0 = fold_partials(scratch + count, count, lds);
    if (threadIdx.x == 0) {
        out[0] = dist;
        out[1] = dist0;
        out[2] = dist / dist0;
        out[3] = 0.0;
    }
}

__global__ __launch_bounds__(BLOCK) void traj_tbar_kernel(const float* __restrict__ theta, const float* __restrict__ target,
                                                          const double* __restrict__ out, int64_t n, float* __restrict__ tbar) {
#pragma clang fp contract(off)
    const float dist0 = (float)out[1];
    const int64_t n4 = n / 4;
    const int64_t stride = (int64_t)gridDim.x * BLOCK;
    const int64_t tid = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const float4* a4 = reinterpret_cast<const float4*>(theta);
    const float4* c4 = reinterpret_cast<const float4*>(target);
    float4* o4 = reinterpret_cast<float4*>(tbar);
    for (int64_t i = tid; i < n4; i += stride) {
        const float4 a = a4[i], c = c4[i];
        float4 r;
        r.x = (2.0f * (a.x - c.x)) / dist0;
        r.y = (2.0f * (a.y - c.y)) / dist0;
        r.z = (2.0f * (a.z - c.z)) / dist0;
        r.w = (2.0f * (a.w - c.w)) / dist0;
        o4[i] = r;
    }
    const int64_t j = n4 * 4 + tid;
    if (tid < 3 && j < n) tbar[j] = (2.0f * (theta[j] - target[j])) / dist0;
}

__device__ inline double prod_f64(float a, float b) {
#pragma clang fp contract(off)
    return (double)a * (double)b;
}

template <bool HAS_HV>
__global__ __launch_bounds__(BLOCK) void traj_adjoint_kernel(float* __restrict__ tbar, const float* __restrict__ hv,
                                                             const float* __restrict__ g, const float* __restrict__ lr_dev,
                                                             float share, int64_t n, double* __restrict__ scratch,
                                                             float* __restrict__ v) {
#pragma clang fp contract(off)
    __shared__ double part[4];
    const float scaled = lr_dev[0] * share;
    const float c = -scaled;
    const int64_t n4 = n / 4;
    const int64_t stride = (int64_t)gridDim.x * BLOCK;
    const int64_t tid = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    float4* t4 = reinterpret_cast<float4*>(tbar);
    const float4* h4 = reinterpret_cast<const float4*>(hv);
    const float4* g4 = reinterpret_cast<const float4*>(g);
    float4* v4 = reinterpret_cast<float4*>(v);
    double acc = 0.0;
    for (int64_t i = tid; i < n4; i += stride) {
        float4 t = t4[i];
        const float4 b = g4[i];
        if (HAS_HV) {
            const float4 h = h4[i];
            t.x = t.x + h.x; t.y = t.y + h.y; t.z = t.z + h.z; t.w = t.w + h.w;
            t4[i] = t;
        }
        acc += prod_f64(t.x, b.x); acc += prod_f64(t.y, b.y); acc += prod_f64(t.z, b.z); acc += prod_f64(t.w, b.w);
        float4 r;
        r.x = c * t.x; r.y = c * t.y; r.z = c * t.z; r.w = c * t.w;
        v4[i] = r;
    }
    const int64_t j = n4 * 4 + tid;
    if (tid < 3 && j < n) {
        float t = tbar[j];
        if (HAS_HV) {
            t = t + hv[j];
            tbar[j] = t;
        }
        acc += prod_f64(t, g[j]);
        v[j] = c * t;
    }
    block_partial(acc, part, scratch, blockIdx.x);
}

__global__ __launch_bounds__(BLOCK) void traj_adjoint_fold_kernel(const double* __restrict__ scratch, int count,
                                                                  double* __restrict__ g_lr) {
#pragma clang fp contract(off)
    __shared__ double lds[BLOCK + 16];
    const double total = fold_partials(scratch, count, lds);
    if (threadIdx.x == 0) g_lr[0] = g_lr[0] - total;
}

}  // namespace

extern "C" int64_t vdt_traj_scratch_doubles(int64_t n) {
    return n <= 0 ? 0 : 2 * grid_for(n);
}

extern "C" int vdt_traj_step(const float* theta, const float* g, const float* lr_dev, int64_t n, float* theta_out, void* stream) {
    if (bad(theta) || bad(g) || bad(lr_dev) || bad(theta_out)) return -1;
    if (n <= 0) return -2;
    hipLaunchKernelGGL(traj_step_kernel, dim3((unsigned)grid_for(n)), dim3(BLOCK), 0, reinterpret_cast<hipStream_t>(stream), theta,
                       g, lr_dev, n, theta_out);
    return (int)hipGetLastError();
}

extern "C" int vdt_traj_loss(const float* theta, const float* theta0, const float* target, int64_t n, double* scratch, double* out,
                             float* tbar, void* stream) {
    if (bad(theta) || bad(theta0) || bad(target) || bad(scratch) || bad(out) || bad(tbar)) return -1;
    if (n <= 0) return -2;
    const int64_t blocks = grid_for(n);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(traj_dist_kernel, dim3((unsigned)blocks), dim3(BLOCK), 0, s, theta, theta0, target, n, scratch);
    hipLaunchKernelGGL(traj_dist_fold_kernel, dim3(1), dim3(BLOCK), 0, s, scratch, (int)blocks, out);
    hipLaunchKernelGGL(traj_tbar_kernel, dim3((unsigned)blocks), dim3(BLOCK), 0, s, theta, target, out, n, tbar);
    return (int)hipGetLastError();
}

extern "C" int vdt_traj_adjoint(float* tbar, const float* hv, const float* g, const float* lr_dev, float share, int64_t n,
                                double* scratch, double* g_lr, float* v, void* stream) {
    if (bad(tbar) || (hv != nullptr && misaligned(hv)) || bad(g) || bad(lr_dev) || bad(scratch) || bad(g_lr) || bad(v)) return -1;
    if (n <= 0) return -2;
    const int64_t blocks = grid_for(n);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (hv != nullptr)
        hipLaunchKernelGGL(traj_adjoint_kernel<true>, dim3((unsigned)blocks), dim3(BLOCK), 0, s, tbar, hv, g, lr_dev, share, n,
                           scratch, v);
    else
        hipLaunchKernelGGL(traj_adjoint_kernel<false>, dim3((unsigned)blocks), dim3(BLOCK), 0, s, tbar, hv, g, lr_dev, share, n,
                           scratch, v);
    hipLaunchKernelGGL(traj_adjoint_fold_kernel, dim3(1), dim3(BLOCK), 0, s, scratch, (int)blocks, g_lr);
    return (int)hipGetLastError();
}
