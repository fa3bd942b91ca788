// Key-frame memories: K learned frames per clip, expanded to T frames by a fixed two-tap table, and the adjoint that folds a clip
// gradient back onto the K frames (distill.KeyframeDMTrainer; the tables: video_distillation_amd/keyframes.py).
//
// Reference: the paper's temporal-compression sweep stores a synthetic video as a few frames and brings it to the network's T
// frames by repeating them over segments or interpolating between them; the reference's code has neither.  K = 1 is
// the still clip of still.hip, K = T the clip itself.
//   vdk_keyframe_expand : out[i][t] = w0[t] * keys[i][i0[t]] + w1[t] * keys[i][i1[t]]
//   vdk_keyframe_reduce : g_keys[i][k] = sum over the terms (t, w) with index k of w * g[i][t], ascending t, i0 before i1
// fp32 with __fmul_rn / __fadd_rn (nothing contracts to a fused multiply-add); a term of weight exactly 0 is skipped, so a zero
// weight never meets an infinity and a single term of weight 1 is a copy.  Both are HBM-bound: expand reads K frames and writes
// T, reduce reads a gradient frame once per key that references it (at most twice) and writes K.  No LDS, no atomics: reduce is
// bitwise repeatable and equals a host loop of float operations.
//   *_vec_kernel    : 3*H*W % 4 == 0 and 16-byte aligned bases: a lane owns one float4 of a clip (expand) or of a (clip, key)
//                     pair (reduce) and walks the frames; grid x = 256-quad chunks of a frame, grid y strides over the clips /
//                     pairs.  Every table lookup is indexed by the frame counter or by blockIdx: workgroup-uniform, served from
//                     the kernel-argument segment by scalar loads, and every `if` on a table value is a uniform branch.
//   *_scalar_kernel : everything else, one element per lane, 64-bit grid-stride loop (the key of a lane differs within a wave in
//                     reduce; the table is still indexed by the frame counter only, never a register array by a lane's key)
// The table travels BY VALUE in the kernel arguments (1032 bytes): no device table, no upload.  Element offsets are 64-bit.
// The indices are checked on the host (vdk_table_check) before a launch: the kernels do not check them.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/vd_keyframes.h"

namespace {

__device__ __forceinline__ float4 mul4(float w, float4 v) {
    return make_float4(__fmul_rn(w, v.x), __fmul_rn(w, v.y), __fmul_rn(w, v.z), __fmul_rn(w, v.w));
}

__device__ __forceinline__ float4 add4(float4 a, float4 b) {
    return make_float4(__fadd_rn(a.x, b.x), __fadd_rn(a.y, b.y), __fadd_rn(a.z, b.z), __fadd_rn(a.w, b.w));
}

// c ? a : b per component: a ternary on the float4 struct itself selects between two ADDRESSES and sends both values to scratch
__device__ __forceinline__ float4 sel4(bool c, float4 a, float4 b) {
    return make_float4(c ? a.x : b.x, c ? a.y : b.y, c ? a.z : b.z, c ? a.w : b.w);
}

__global__ __launch_bounds__(256) void keyframe_expand_vec_kernel(const float4* __restrict__ keys, int64_t n, const VdkTable tab,
                                                                   int64_t quads, float4* __restrict__ out) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= quads) return;
    const int T = tab.T, K = tab.K;
    for (int64_t i = blockIdx.y; i < n; i += gridDim.y) {
        const float4* s = keys + i * K * quads + q;
        float4* d = out + i * T * quads + q;
        // the two keys last read stay in registers: along t the tables of keyframes.py move from one key to the next, so each
        // key is read once per clip (any other table is still computed right, with more loads)
        int ja = -1, jb = -1;
        float4 va = make_float4(0.f, 0.f, 0.f, 0.f), vb = va;
        for (int t = 0; t < T; ++t) {
            const float w0 = tab.w0[t], w1 = tab.w1[t];
            const int i0 = tab.i0[t], i1 = tab.i1[t];
            float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
            bool have = false;
            if (w0 != 0.f) {
                if (i0 != ja) {
                    if (i0 == jb) { const float4 x = va; va = vb; vb = x; jb = ja; }
                    else va = s[(int64_t)i0 * quads];
                    ja = i0;
                }
                r = w0 == 1.f ? va : mul4(w0, va);
                have = true;
            }
            if (w1 != 0.f) {
                float4 v;
                if (i1 == ja) v = va;
                else {
                    if (i1 != jb) { vb = s[(int64_t)i1 * quads]; jb = i1; }
                    v = vb;
                }
                const float4 p = w1 == 1.f ? v : mul4(w1, v);
                r = have ? add4(r, p) : p;
            }
            d[(int64_t)t * quads] = r;
        }
    }
}

__global__ __launch_bounds__(256) void keyframe_expand_scalar_kernel(const float* __restrict__ keys, int64_t n, const VdkTable tab,
                                                                      int64_t chw, float* __restrict__ out) {
    const int64_t total = n * chw;
    const int T = tab.T, K = tab.K;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t i = e / chw, p = e - i * chw;
        const float* s = keys + i * K * chw + p;
        float* d = out + i * T * chw + p;
        for (int t = 0; t < T; ++t) {
            const float w0 = tab.w0[t], w1 = tab.w1[t];
            float r = 0.f;
            bool have = false;
            if (w0 != 0.f) {
                const float v = s[(int64_t)tab.i0[t] * chw];
                r = w0 == 1.f ? v : __fmul_rn(w0, v);
                have = true;
            }
            if (w1 != 0.f) {
                const float v = s[(int64_t)tab.i1[t] * chw];
                const float pr = w1 == 1.f ? v : __fmul_rn(w1, v);
                r = have ? __fadd_rn(r, pr) : pr;
            }
            d[(int64_t)t * chw] = r;
        }
    }
}

// grid y = clip * K + key, strided past the y limit: k is workgroup-uniform, every test below is a uniform branch, and a frame's
// gradient is loaded only by the (at most two) keys whose terms name it
__global__ __launch_bounds__(256) void keyframe_reduce_vec_kernel(const float4* __restrict__ g, int64_t n, const VdkTable tab,
                                                                   int64_t quads, float4* __restrict__ out) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= quads) return;
    const int T = tab.T, K = tab.K;
    const int64_t pairs = n * K;
    for (int64_t pr = blockIdx.y; pr < pairs; pr += gridDim.y) {
        const int64_t i = pr / K;
        const int k = (int)(pr - i * K);
        const float4* s = g + i * T * quads + q;
        // the frames lo..hi that hold a term of key k (scalar work): contiguous for the tables of keyframes.py, so every frame
        // of the walk below is one the key needs; for any other table the frames in between are read and not used
        int lo = 0, hi = T - 1;
        while (lo < T && !((tab.i0[lo] == k && tab.w0[lo] != 0.f) || (tab.i1[lo] == k && tab.w1[lo] != 0.f))) ++lo;
        while (hi >= lo && !((tab.i0[hi] == k && tab.w0[hi] != 0.f) || (tab.i1[hi] == k && tab.w1[hi] != 0.f))) --hi;
        // the walk has no branch: a term that is not the key's, or has weight 0, is computed and dropped by a select on a uniform
        // condition (it never reaches the accumulator), so the loads of an unrolled group are issued together as in still.hip
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
        bool have = false;
#pragma unroll 4
        for (int t = lo; t <= hi; ++t) {
            const float4 v = s[(int64_t)t * quads];
            const float w0 = tab.i0[t] == k ? tab.w0[t] : 0.f;
            const float w1 = tab.i1[t] == k ? tab.w1[t] : 0.f;
            const float4 p0 = sel4(w0 == 1.f, v, mul4(w0, v));
            a = sel4(w0 != 0.f, sel4(have, add4(a, p0), p0), a);
            have = have || w0 != 0.f;
            const float4 p1 = sel4(w1 == 1.f, v, mul4(w1, v));
            a = sel4(w1 != 0.f, sel4(have, add4(a, p1), p1), a);
            have = have || w1 != 0.f;
        }
        out[pr * quads + q] = a;
    }
}

__global__ __launch_bounds__(256) void keyframe_reduce_scalar_kernel(const float* __restrict__ g, int64_t n, const VdkTable tab,
                                                                      int64_t chw, float* __restrict__ out) {
    const int T = tab.T, K = tab.K;
    const int64_t per = (int64_t)K * chw, total = n * per;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t i = e / per, r = e - i * per;
        const int k = (int)(r / chw);
        const int64_t p = r - (int64_t)k * chw;
        const float* s = g + i * T * chw + p;
        float a = 0.f;
        bool have = false;
        for (int t = 0; t < T; ++t) {
            const float w0 = tab.i0[t] == k ? tab.w0[t] : 0.f;
            const float w1 = tab.i1[t] == k ? tab.w1[t] : 0.f;
            if (w0 == 0.f && w1 == 0.f) continue;
            const float v = s[(int64_t)t * chw];
            if (w0 != 0.f) {
                const float pr = w0 == 1.f ? v : __fmul_rn(w0, v);
                a = have ? __fadd_rn(a, pr) : pr;
                have = true;
            }
            if (w1 != 0.f) {
                const float pr = w1 == 1.f ? v : __fmul_rn(w1, v);
                a = have ? __fadd_rn(a, pr) : pr;
                have = true;
            }
        }
        out[e] = a;
    }
}

inline bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

// grid of the vector kernels: x = chunks of a frame, y = clips or (clip, key) pairs (strided when there are more than the y limit)
inline dim3 vec_grid(int64_t quads, int64_t rows) {
    const int64_t gx = (quads + 255) / 256;
    return dim3((unsigned)gx, (unsigned)(rows < 65535 ? rows : 65535));
}

inline unsigned scalar_blocks(int64_t total) {
    const int64_t b = (total + 255) / 256;
    return (unsigned)(b < 16384 ? b : 16384);
}

}  // namespace

extern "C" int vdk_table_check(const VdkTable* table) {
    if (!table) return -1;
    const int T = table->T, K = table->K;
    if (T < 1 || T > VDK_MAX_FRAMES || K < 1 || K > T) return -1;
    for (int t = 0; t < T; ++t) {
        if (table->i0[t] < 0 || table->i0[t] >= K || table->i1[t] < 0 || table->i1[t] >= K) return -1;
        if (!std::isfinite(table->w0[t]) || !std::isfinite(table->w1[t])) return -1;
    }
    return 0;
}

extern "C" int vdk_keyframe_expand(const float* keys, int64_t n, const VdkTable* table, int H, int W, float* out, void* stream) {
    if (vdk_table_check(table) != 0 || H <= 0 || W <= 0 || n < 0) return -1;
    if (n == 0) return 0;
    if (!keys || !out) return -1;
    const int64_t chw = (int64_t)3 * H * W;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (chw % 4 == 0 && aligned16(keys) && aligned16(out)) {
        hipLaunchKernelGGL(keyframe_expand_vec_kernel, vec_grid(chw / 4, n), dim3(256), 0, st, reinterpret_cast<const float4*>(keys), n,
                           *table, chw / 4, reinterpret_cast<float4*>(out));
    } else {
        hipLaunchKernelGGL(keyframe_expand_scalar_kernel, dim3(scalar_blocks(n * chw)), dim3(256), 0, st, keys, n, *table, chw, out);
    }
    return (int)hipGetLastError();
}

extern "C" int vdk_keyframe_reduce(const float* g_clips, int64_t n, const VdkTable* table, int H, int W, float* g_keys, void* stream) {
    if (vdk_table_check(table) != 0 || H <= 0 || W <= 0 || n < 0) return -1;
    if (n == 0) return 0;
    if (!g_clips || !g_keys) return -1;
    const int64_t chw = (int64_t)3 * H * W;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (chw % 4 == 0 && aligned16(g_clips) && aligned16(g_keys)) {
        hipLaunchKernelGGL(keyframe_reduce_vec_kernel, vec_grid(chw / 4, n * table->K), dim3(256), 0, st,
                           reinterpret_cast<const float4*>(g_clips), n, *table, chw / 4, reinterpret_cast<float4*>(g_keys));
    } else {
        hipLaunchKernelGGL(keyframe_reduce_scalar_kernel, dim3(scalar_blocks(n * table->K * chw)), dim3(256), 0, st, g_clips, n, *table,
                           chw, g_keys);
    }
    return (int)hipGetLastError();
}
