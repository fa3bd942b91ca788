// Still clips: one image repeated over T frames, and the sum of a clip gradient over its frames (distill.StillGMTrainer).
//
// Reference: the `static*` / `single*` datasets hand ConvNet3D a frame stacked `frames` times (distill_utils/dataset.py:626-633),
// and the hallucinator's static branch feeds it the same image in every frame.  Gradient matching on such clips keeps the
// IMAGES in HBM -- a sixteenth of the clips -- and builds the clips per step:
//   vds_still_expand : out[i][t][c][y][x] = images[index ? index[i] : i][c][y][x]       (a gather with `index`, identity without)
//   vds_still_reduce : g_images[i][c][y][x] = ((g[i][0] + g[i][1]) + ...) + g[i][T-1]    (the adjoint of expand with identity index)
// Both are HBM-bound copies: expand reads an element once and writes it T times, reduce reads T and writes one.  No LDS, no
// atomics; reduce adds in ascending t, one fp32 add per frame (adds only: nothing for the compiler to contract), so its result
// is bitwise repeatable and equals a host loop of float adds.
//   *_vec_kernel    : 3*H*W % 4 == 0 and 16-byte aligned bases: a lane owns one float4 of an image and walks the frames;
//                     grid x = 256-quad chunks of an image, grid y strides over the images, so `index[i]` is workgroup-uniform
//   *_scalar_kernel : everything else, one element per lane, 64-bit grid-stride loop
// Element offsets are 64-bit throughout (256 clips of 16x3x112x112 are 154 M floats; nothing here assumes they fit 2^31).
// `index` is not checked on the device: hip.still_expand refuses a row outside the images before it is uploaded.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vd_hip.h"

namespace {

__global__ __launch_bounds__(256) void still_expand_vec_kernel(const float4* __restrict__ images, const int64_t* __restrict__ index,
                                                               int64_t n, int T, int64_t quads, float4* __restrict__ out) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= quads) return;
    for (int64_t i = blockIdx.y; i < n; i += gridDim.y) {
        const int64_t row = index ? index[i] : i;
        const float4 v = images[row * quads + q];
        float4* d = out + i * T * quads + q;
        for (int t = 0; t < T; ++t) d[(int64_t)t * quads] = v;
    }
}

__global__ __launch_bounds__(256) void still_expand_scalar_kernel(const float* __restrict__ images, const int64_t* __restrict__ index,
                                                                  int64_t n, int T, int64_t chw, float* __restrict__ out) {
    const int64_t total = n * chw;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t i = e / chw, p = e - i * chw;
        const int64_t row = index ? index[i] : i;
        const float v = images[row * chw + p];
        float* d = out + i * T * chw + p;
        for (int t = 0; t < T; ++t) d[(int64_t)t * chw] = v;
    }
}

__global__ __launch_bounds__(256) void still_reduce_vec_kernel(const float4* __restrict__ g, int64_t n, int T, int64_t quads,
                                                               float4* __restrict__ out) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= quads) return;
    for (int64_t i = blockIdx.y; i < n; i += gridDim.y) {
        const float4* s = g + i * T * quads + q;
        float4 a = s[0];
#pragma unroll 4
        for (int t = 1; t < T; ++t) {          // ascending t, one add per frame (the loads of an unrolled group are issued together)
            const float4 b = s[(int64_t)t * quads];
            a.x = a.x + b.x; a.y = a.y + b.y; a.z = a.z + b.z; a.w = a.w + b.w;
        }
        out[i * quads + q] = a;
    }
}

__global__ __launch_bounds__(256) void still_reduce_scalar_kernel(const float* __restrict__ g, int64_t n, int T, int64_t chw,
                                                                  float* __restrict__ out) {
    const int64_t total = n * chw;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t i = e / chw, p = e - i * chw;
        const float* s = g + i * T * chw + p;
        float a = s[0];
#pragma unroll 4
        for (int t = 1; t < T; ++t) a = a + s[(int64_t)t * chw];
        out[e] = a;
    }
}

inline bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

// grid of the vector kernels: x = chunks of an image, y = images (strided when there are more than the y limit)
inline dim3 vec_grid(int64_t quads, int64_t n) {
    const int64_t gx = (quads + 255) / 256;
    return dim3((unsigned)gx, (unsigned)(n < 65535 ? n : 65535));
}

inline unsigned scalar_blocks(int64_t total) {
    const int64_t b = (total + 255) / 256;
    return (unsigned)(b < 16384 ? b : 16384);
}

}  // namespace

extern "C" int vds_still_expand(const float* images, const int64_t* index, int64_t n, int T, int H, int W, float* out, void* stream) {
    if (T <= 0 || H <= 0 || W <= 0 || n < 0) return -1;
    if (n == 0) return 0;
    if (!images || !out) return -1;
    const int64_t chw = (int64_t)3 * H * W;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (chw % 4 == 0 && aligned16(images) && aligned16(out)) {
        hipLaunchKernelGGL(still_expand_vec_kernel, vec_grid(chw / 4, n), dim3(256), 0, st, reinterpret_cast<const float4*>(images),
                           index, n, T, chw / 4, reinterpret_cast<float4*>(out));
    } else {
        hipLaunchKernelGGL(still_expand_scalar_kernel, dim3(scalar_blocks(n * chw)), dim3(256), 0, st, images, index, n, T, chw, out);
    }
    return (int)hipGetLastError();
}

extern "C" int vds_still_reduce(const float* g_clips, int64_t n, int T, int H, int W, float* g_images, void* stream) {
    if (T <= 0 || H <= 0 || W <= 0 || n < 0) return -1;
    if (n == 0) return 0;
    if (!g_clips || !g_images) return -1;
    const int64_t chw = (int64_t)3 * H * W;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (chw % 4 == 0 && aligned16(g_clips) && aligned16(g_images)) {
        hipLaunchKernelGGL(still_reduce_vec_kernel, vec_grid(chw / 4, n), dim3(256), 0, st, reinterpret_cast<const float4*>(g_clips), n,
                           T, chw / 4, reinterpret_cast<float4*>(g_images));
    } else {
        hipLaunchKernelGGL(still_reduce_scalar_kernel, dim3(scalar_blocks(n * chw)), dim3(256), 0, st, g_clips, n, T, chw, g_images);
    }
    return (int)hipGetLastError();
}
