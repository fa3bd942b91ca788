// HBM-bound helper kernels of the DM / gradient-matching hot path (gfx950).
// Each is a coalesced streaming kernel: 16-byte accesses per lane where the layout allows,
// wave64 shuffle reductions, one atomic (or one plain store) per workgroup.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/vd_hip.h"
#include "frame_norm.h"
#include "split16.h"      // split16p (shared with still_rows.hip)

typedef __bf16 bf16_t;

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// block-wide sum; result valid in thread 0.  blockDim.x <= 1024, multiple of 64.
__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[w] = v;
    __syncthreads();
    float t = 0.f;
    if (threadIdx.x == 0) {
        const int nw = (blockDim.x + 63) >> 6;
        for (int i = 0; i < nw; ++i) t += red[i];
    }
    return t;
}

// VD_PREC_F16X3 operands hold W x 2^VD_F16X3_WSHIFT (vd_hip.h: an unscaled fp16 pair of a weight of 0.006 is exact to 3e-6 only --
// its low part is a subnormal; the tile programs undo the shift in their fp32 epilogues)
__device__ __forceinline__ float pack_shift(int prec) { return prec == VD_PREC_F16X3 ? (float)(1 << VD_F16X3_WSHIFT) : 1.f; }

// ------------------------------------------------------------------------------------------
__global__ void pack_weights_kernel(const float* __restrict__ w, const int32_t* __restrict__ widx, int64_t n,
                                    uint16_t* __restrict__ hi, uint16_t* __restrict__ lo, int prec) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t k = widx[i];
    const float v = (k >= 0) ? w[k] * pack_shift(prec) : 0.f;
    uint16_t h, l;
    split16p(prec, v, h, l);
    hi[i] = h;
    if (lo != nullptr) lo[i] = l;
}

extern "C" int vd_pack_weights(const float* w, const int32_t* widx, int64_t n, void* out_hi, void* out_lo,
                               int prec, void* stream) {
    if (n <= 0) return 0;
    const int bs = 256;
    hipLaunchKernelGGL(pack_weights_kernel, dim3((unsigned)((n + bs - 1) / bs)), dim3(bs), 0,
                       reinterpret_cast<hipStream_t>(stream), w, widx, n, (uint16_t*)out_hi, (uint16_t*)out_lo, prec);
    return (int)hipGetLastError();
}

__global__ void pack_weights_multi_kernel(const VdPackBatch b) {
    int k = 0;
#pragma unroll 1
    while (k + 1 < b.nseg && (int)blockIdx.x >= b.seg[k + 1].first_block) ++k;      // (block-uniform: scalar loads of the kernel arguments)
    const VdPackSeg& sg = b.seg[k];
    const int64_t i = (int64_t)((int)blockIdx.x - sg.first_block) * blockDim.x + threadIdx.x;
    if (i >= sg.n) return;
    const int32_t j = sg.widx[i];
    const float v = (j >= 0) ? sg.w[j] * pack_shift(sg.prec) : 0.f;
    uint16_t h, l;
    split16p(sg.prec, v, h, l);
    reinterpret_cast<uint16_t*>(sg.out_hi)[i] = h;
    if (sg.out_lo != nullptr) reinterpret_cast<uint16_t*>(sg.out_lo)[i] = l;
}

extern "C" int vd_pack_weights_multi(const VdPackBatch* batch, void* stream) {
    if (batch == nullptr || batch->nseg < 0 || batch->nseg > VD_PACK_MAX) return -2;
    VdPackBatch b = *batch;
    const int bs = 256;
    int64_t blocks = 0;
    int m = 0;
    for (int k = 0; k < batch->nseg; ++k) {
        const VdPackSeg& sg = batch->seg[k];
        if (sg.n <= 0) continue;
        if (sg.w == nullptr || sg.widx == nullptr || sg.out_hi == nullptr) return -1;
        b.seg[m] = sg;
        b.seg[m].first_block = (int32_t)blocks;
        blocks += (sg.n + bs - 1) / bs;
        ++m;
    }
    if (m == 0) return 0;
    if (blocks > 0x7fffffff) return -2;
    b.nseg = m;
    hipLaunchKernelGGL(pack_weights_multi_kernel, dim3((unsigned)blocks), dim3(bs), 0, reinterpret_cast<hipStream_t>(stream), b);
    return (int)hipGetLastError();
}

// DITHERED single-pass weights: the real clips of a class are dealt to `groups` (a power of two) launch groups, and group g
// multiplies by the weights rounded DOWN or UP to the neighbouring 16-bit values such that, for every weight, the mean over
// the groups equals the fp32 value to 1/(2 groups) ulp: with lam = (w - lo) / (hi - lo) the weight rounds up in
// round(lam * groups) of the groups -- those whose slot (bit-reversed group number, rotated per weight by a hash of its
// index) falls below lam.  Plain rn16(W) perturbs the class mean of the real features SYSTEMATICALLY (1.9e-4 |f|, it does
// not average out over the clips of a batch); the dithered groups' perturbations cancel to first order in the mean
// (CPU simulation tests/sim_dither_tool.py: 3.0e-5 |f| at 8 groups, 2.2e-5 at 16; the value pass it replaces leaves 8e-5).
// out[g][i] = packed operand element i of group g (same gather table as vd_pack_weights).
__device__ __forceinline__ uint16_t f16_step(uint16_t b, bool up) {
    // next representable value above (up) / below a 16-bit sign-magnitude float (f16 and bf16 alike); +-0 handled
    const bool neg = (b & 0x8000u) != 0;
    const uint16_t mag = b & 0x7FFFu;
    if (mag == 0) return up ? (uint16_t)0x0001u : (uint16_t)0x8001u;
    return (neg == up) ? (uint16_t)(b - 1) : (uint16_t)(b + 1);
}

__global__ void pack_weights_dither_kernel(const float* __restrict__ w, const int32_t* __restrict__ widx, int64_t n, int groups,
                                           int log2g, uint16_t* __restrict__ out, int prec) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t k = widx[i];
    const float v = (k >= 0) ? w[k] : 0.f;
    const bool bf = (prec == VD_PREC_BF16 || prec == VD_PREC_BF16X3);
    uint16_t qb; float qf;
    if (bf) { const __bf16 q = (__bf16)v; qb = __builtin_bit_cast(uint16_t, q); qf = (float)q; }
    else { const _Float16 q = (_Float16)v; qb = __builtin_bit_cast(uint16_t, q); qf = (float)q; }
    uint16_t lob = qb, hib = qb;
    float lo = qf, hi = qf;
    const bool finite = (qb & 0x7FFFu) < (bf ? 0x7F80u : 0x7C00u);
    if (finite && qf < v) { hib = f16_step(qb, true); hi = bf ? (float)__builtin_bit_cast(__bf16, hib) : (float)__builtin_bit_cast(_Float16, hib); }
    if (finite && qf > v) { lob = f16_step(qb, false); lo = bf ? (float)__builtin_bit_cast(__bf16, lob) : (float)__builtin_bit_cast(_Float16, lob); }
    const bool split = hi > lo && hi < 3.0e38f && lo > -3.0e38f;
    const float lam = split ? (v - lo) / (hi - lo) : 0.f;
    const uint32_t rot = (((uint32_t)k * 2654435761u) >> 7) & (uint32_t)(groups - 1);
    for (int g = 0; g < groups; ++g) {
        const uint32_t rev = log2g ? (__brev((uint32_t)g) >> (32 - log2g)) : 0u;
        const uint32_t slot = (rev + rot) & (uint32_t)(groups - 1);
        const float t = ((float)slot + 0.5f) / (float)groups;
        out[(int64_t)g * n + i] = (t < lam) ? hib : lob;
    }
}

// Operand planes of a VD_PREC_F16C8 program (include/vd_hip.h): plane 0 = the fp16 fragments vd_pack_weights writes; plane 1 = per
// (chunk, group of four K steps, N tile, lane) 64 bytes -- the 16-byte pieces the kernel loads at steps 4g .. 4g+3 -- holding the
// fp8 (e4m3) fragment of W_hi = rn16(W) scaled by s (pieces 0, 1: elements j = 0..31) and of W_lo = W - W_hi scaled by s * 2^11
// (pieces 2, 3), element j = 8 q + e = (step 4g + q, this lane's tap half, channel e).  s = the power of two that brings max|W| into
// [128, 256) (vd_absmax_scale); scales[0..1] receive the E8M0 codes 127 - log2(s) and 127 - log2(s) - 11 the kernel hands to the
// matrix instruction, scales[2..5] are scratch of the max reduction.
__global__ void pack_weights_c8_kernel(const float* __restrict__ w, const int32_t* __restrict__ widx, int CC, int S, int NT,
                                       const float* __restrict__ sc, uint4* __restrict__ plane1, int* __restrict__ codes) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;      // one 16-byte piece per thread
    const int64_t npieces = (int64_t)CC * S * NT * 64;
    const float s_hi = sc[0], s_lo = sc[0] * 2048.f;
    if (i == 0) {
        const int e = (int)(__float_as_uint(s_hi) >> 23) - 127;          // s_hi is a power of two
        codes[0] = 127 - e; codes[1] = 127 - e - 11;
    }
    if (i >= npieces) return;
    const int lane = (int)(i & 63);
    int64_t r = i >> 6;
    const int nt = (int)(r % NT); r /= NT;
    const int st = (int)(r % S);
    const int cc = (int)(r / S);
    const int g = st >> 2, q = st & 3;
    const bool lo = q >= 2;
    uint32_t out[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        float v[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int j = 16 * (q & 1) + 4 * d + b;                      // element of the 32-byte fragment half this piece holds
            const int qs = j >> 3, e = j & 7;
            const int32_t wi = widx[((((int64_t)cc * S + 4 * g + qs) * NT + nt) * 64 + lane) * 8 + e];
            const float x = wi >= 0 ? w[wi] : 0.f;
            const float hi = (float)(_Float16)x;
            float y = lo ? (x - hi) * s_lo : hi * s_hi;
            v[b] = fminf(fmaxf(y, -448.f), 448.f);
        }
        int word = 0;
        word = __builtin_amdgcn_cvt_pk_fp8_f32(v[0], v[1], word, false);
        word = __builtin_amdgcn_cvt_pk_fp8_f32(v[2], v[3], word, true);
        out[d] = (uint32_t)word;
    }
    plane1[i] = make_uint4(out[0], out[1], out[2], out[3]);
}

extern "C" int vd_pack_weights_c8(const float* w, int64_t w_elems, const int32_t* widx, int CC, int S, int NT, void* out_hi, void* out_c8,
                                  float* scales6, void* stream) {
    if (w == nullptr || widx == nullptr || out_hi == nullptr || out_c8 == nullptr || scales6 == nullptr) return -1;
    if (CC <= 0 || S <= 0 || NT <= 0 || S % 4 != 0 || w_elems <= 0) return -2;
    const int64_t n = (int64_t)CC * S * NT * 64 * 8;
    int rc = vd_pack_weights(w, widx, n, out_hi, nullptr, VD_PREC_F16, stream);
    if (rc) return rc;
    if ((rc = vd_absmax_scale(w, w_elems, 256.0f, scales6 + 2, stream))) return rc;       // scales6[2] = s, [3] = 1 / s, [4] = max bits
    const int64_t npieces = n / 8;
    hipLaunchKernelGGL(pack_weights_c8_kernel, dim3((unsigned)((npieces + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       w, widx, CC, S, NT, scales6 + 2, reinterpret_cast<uint4*>(out_c8), reinterpret_cast<int*>(scales6));
    return (int)hipGetLastError();
}

extern "C" int vd_pack_weights_dither(const float* w, const int32_t* widx, int64_t n, int groups, void* out, int prec, void* stream) {
    if (groups < 1 || groups > 64 || (groups & (groups - 1)) != 0) return -2;
    if (prec != VD_PREC_F16 && prec != VD_PREC_BF16) return -2;          // single-pass formats: the hi+lo formats carry the weights exactly
    if (n <= 0) return 0;
    if (!w || !widx || !out) return -1;
    int log2g = 0;
    while ((1 << log2g) < groups) ++log2g;
    hipLaunchKernelGGL(pack_weights_dither_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       w, widx, n, groups, log2g, (uint16_t*)out, prec);
    return (int)hipGetLastError();
}

// out = (float) rn16(w): the network's weights rounded ONCE to the single-pass operand format, so that
// every pass of a step (single-pass real-clip forward, split-precision synthetic-clip forward, input
// gradient) multiplies by the SAME weights -- the step is then the exact step of the network rn16(W),
// and weight rounding cannot show up as a bias between mean f_real and mean f_syn.
__global__ void round_operand_kernel(const float* __restrict__ w, int64_t n, int prec, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float v = w[i];
    out[i] = (prec == VD_PREC_BF16 || prec == VD_PREC_BF16X3) ? (float)(__bf16)v : (float)(_Float16)v;
}

extern "C" int vd_round_operand(const float* w, int64_t n, int prec, float* out, void* stream) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(round_operand_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), w, n, prec, out);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// one thread per 8 output elements (16 bytes) of a padded 16-bit pixel row:
// out[row][8j .. 8j+7] = x[row][8j-3 .. 8j+4] (zero outside [0,W))
__global__ void pix2rows_kernel(const float* __restrict__ x, const int64_t* __restrict__ clip_index, int64_t nchunks,
                                int rows_per_clip, int W, int cpr,
                                uint4* __restrict__ hi, uint4* __restrict__ lo, int prec) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nchunks) return;
    const int j = (int)(i % cpr);
    int64_t row = i / cpr;                      // (clip, f, h) flattened == row of x
    if (clip_index != nullptr) {                // gather: clip b of the batch is pool clip clip_index[b]
        const int64_t b = row / rows_per_clip;
        row = clip_index[b] * rows_per_clip + (row - b * rows_per_clip);
    }
    const float* xr = x + row * W;
    const int w0 = 8 * j - 3;
    uint16_t h16[8], l16[8];
    if ((W & 3) == 0) {
        // three aligned 16-byte loads cover x[8j-4 .. 8j+7]; the wanted window is elements 1..8
        float f[12];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const int wq = 8 * j - 4 + 4 * q;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (wq >= 0 && wq < W) v = *reinterpret_cast<const float4*>(xr + wq);
            f[4 * q] = v.x; f[4 * q + 1] = v.y; f[4 * q + 2] = v.z; f[4 * q + 3] = v.w;
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) split16p(prec, f[k + 1], h16[k], l16[k]);
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int ww = w0 + k;
            const float v = (ww >= 0 && ww < W) ? xr[ww] : 0.f;
            split16p(prec, v, h16[k], l16[k]);
        }
    }
    uint4 vh, vl;
    vh.x = h16[0] | ((uint32_t)h16[1] << 16); vh.y = h16[2] | ((uint32_t)h16[3] << 16);
    vh.z = h16[4] | ((uint32_t)h16[5] << 16); vh.w = h16[6] | ((uint32_t)h16[7] << 16);
    hi[i] = vh;
    if (lo != nullptr) {
        vl.x = l16[0] | ((uint32_t)l16[1] << 16); vl.y = l16[2] | ((uint32_t)l16[3] << 16);
        vl.z = l16[4] | ((uint32_t)l16[5] << 16); vl.w = l16[6] | ((uint32_t)l16[7] << 16);
        lo[i] = vl;
    }
}

extern "C" int vd_pix2rows(const float* x, const int64_t* clip_index, int64_t nclips, int T, int H, int W,
                           void* out_hi, void* out_lo, int prec, void* stream) {
    const int cpr = ((W + 8) + 7) / 8;          // 16-byte chunks per padded row
    const int64_t nchunks = nclips * T * 3 * H * cpr;
    if (nchunks <= 0) return 0;
    const int bs = 256;
    hipLaunchKernelGGL(pix2rows_kernel, dim3((unsigned)((nchunks + bs - 1) / bs)), dim3(bs), 0,
                       reinterpret_cast<hipStream_t>(stream), x, clip_index, nchunks, T * 3 * H, W, cpr, (uint4*)out_hi,
                       (uint4*)out_lo, prec);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// Backward of ReLU+MaxPool: one thread per output slot (clip, cc, t, oh, ow) of the dense conv grid.
__global__ void unpool_relu_bwd_kernel(const float* __restrict__ g, const uint8_t* __restrict__ amax, int64_t nslots,
                                       int C, int To, int Ho, int Wo, int pool_t, int T, int OH, int OW,
                                       int g_layout, uint4* __restrict__ hi, uint4* __restrict__ lo, int prec,
                                       const float* __restrict__ scale) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nslots) return;
    const float sc = (scale != nullptr) ? scale[0] : 1.f;
    int64_t r = i;
    const int ow = (int)(r % OW); r /= OW;
    const int oh = (int)(r % OH); r /= OH;
    const int t = (int)(r % T); r /= T;
    const int CC = C >> 3;
    const int cc = (int)(r % CC);
    const int64_t clip = r / CC;
    const int pt = t / pool_t, pr = oh >> 1, pc = ow >> 1;
    uint16_t h16[8], l16[8];
    const bool inside = (pt < To) && (pr < Ho) && (pc < Wo);
    const int j = (pool_t == 2 ? ((t & 1) << 2) : 0) | ((oh & 1) << 1) | (ow & 1);
    const int64_t npos = (int64_t)To * Ho * Wo;
    const int64_t pos = ((int64_t)pt * Ho + pr) * Wo + pc;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        float v = 0.f;
        if (inside) {
            const int n = cc * 8 + e;
            int64_t gi, ai;
            if (g_layout == 0) { gi = (clip * C + n) * npos + pos; ai = gi; }
            else { gi = (clip * npos + pos) * C + n; ai = ((clip * CC + cc) * npos + pos) * 8 + e; }
            if (amax[ai] == (uint8_t)j) v = g[gi] * sc;
        }
        split16p(prec, v, h16[e], l16[e]);
    }
    uint4 vh, vl;
    vh.x = h16[0] | ((uint32_t)h16[1] << 16); vh.y = h16[2] | ((uint32_t)h16[3] << 16);
    vh.z = h16[4] | ((uint32_t)h16[5] << 16); vh.w = h16[6] | ((uint32_t)h16[7] << 16);
    hi[i] = vh;
    if (lo != nullptr) {
        vl.x = l16[0] | ((uint32_t)l16[1] << 16); vl.y = l16[2] | ((uint32_t)l16[3] << 16);
        vl.z = l16[4] | ((uint32_t)l16[5] << 16); vl.w = l16[6] | ((uint32_t)l16[7] << 16);
        lo[i] = vl;
    }
}

// The same scatter with one thread per 2 x 2 spatial pool WINDOW of one conv frame (even conv grids: every dense position
// belongs to exactly one window): the window's 8 arg-max bytes and 8 gradient values are read ONCE instead of four times (the
// channels-last layout holds both as one 8-byte / 32-byte run), and the four slots it writes are two 32-byte runs per plane,
// contiguous across neighbouring threads.  Same values bit for bit; 0.31 -> 0.22 ms for the first level's 640 MB of 50 clips.
__global__ void unpool_relu_bwd_win_kernel(const float* __restrict__ g, const uint8_t* __restrict__ amax, int64_t nwin,
                                           int C, int To, int Ho, int Wo, int pool_t, int T, int OH, int OW,
                                           uint4* __restrict__ hi, uint4* __restrict__ lo, int prec, const float* __restrict__ scale) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nwin) return;
    const float sc = (scale != nullptr) ? scale[0] : 1.f;
    const int hw = OW >> 1, hh = OH >> 1;
    int64_t r = i;
    const int pc = (int)(r % hw); r /= hw;
    const int pr = (int)(r % hh); r /= hh;
    const int t = (int)(r % T); r /= T;
    const int CC = C >> 3;
    const int cc = (int)(r % CC);
    const int64_t clip = r / CC;
    const int pt = t / pool_t;
    const bool inside = (pt < To) && (pr < Ho) && (pc < Wo);
    const int jt = (pool_t == 2) ? ((t & 1) << 2) : 0;
    const int64_t npos = (int64_t)To * Ho * Wo;
    const int64_t pos = ((int64_t)pt * Ho + pr) * Wo + pc;
    float gv[8];
    int code[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { gv[e] = 0.f; code[e] = -1; }
    if (inside) {       // channels-last: (clip, pos) holds the C gradient values / arg-max bytes of 8 channels contiguously
        const float4 a = *reinterpret_cast<const float4*>(g + (clip * npos + pos) * C + cc * 8);
        const float4 b = *reinterpret_cast<const float4*>(g + (clip * npos + pos) * C + cc * 8 + 4);
        const uint2 am = *reinterpret_cast<const uint2*>(amax + ((clip * CC + cc) * npos + pos) * 8);
        gv[0] = a.x * sc; gv[1] = a.y * sc; gv[2] = a.z * sc; gv[3] = a.w * sc;
        gv[4] = b.x * sc; gv[5] = b.y * sc; gv[6] = b.z * sc; gv[7] = b.w * sc;
#pragma unroll
        for (int e = 0; e < 4; ++e) { code[e] = (am.x >> (8 * e)) & 0xff; code[4 + e] = (am.y >> (8 * e)) & 0xff; }
    }
    const int64_t base = (((clip * CC + cc) * T + t) * OH + 2 * pr) * (int64_t)OW + 2 * pc;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int dr = q >> 1, dc = q & 1, j = jt | (dr << 1) | dc;
        uint16_t h16[8], l16[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) split16p(prec, code[e] == j ? gv[e] : 0.f, h16[e], l16[e]);
        const int64_t o = base + (int64_t)dr * OW + dc;
        uint4 vh, vl;
        vh.x = h16[0] | ((uint32_t)h16[1] << 16); vh.y = h16[2] | ((uint32_t)h16[3] << 16);
        vh.z = h16[4] | ((uint32_t)h16[5] << 16); vh.w = h16[6] | ((uint32_t)h16[7] << 16);
        hi[o] = vh;
        if (lo != nullptr) {
            vl.x = l16[0] | ((uint32_t)l16[1] << 16); vl.y = l16[2] | ((uint32_t)l16[3] << 16);
            vl.z = l16[4] | ((uint32_t)l16[5] << 16); vl.w = l16[6] | ((uint32_t)l16[7] << 16);
            lo[o] = vl;
        }
    }
}

extern "C" int vd_unpool_relu_bwd(const float* g, const uint8_t* argmax, int64_t nclips, int C, int To, int Ho, int Wo,
                                  int pool_t, int T, int OH, int OW, int g_layout, void* out_hi, void* out_lo,
                                  int prec, const float* scale, void* stream) {
    if (C % 8 != 0 || (pool_t != 1 && pool_t != 2)) return -2;
    const int64_t nslots = nclips * (C / 8) * T * OH * OW;
    if (nslots <= 0) return 0;
    const int bs = 256;
    // window form: channels-last gradient, even conv grid (every position in exactly one window), 16-byte aligned gradient rows
    if (g_layout == 1 && (OH & 1) == 0 && (OW & 1) == 0 && (reinterpret_cast<uintptr_t>(g) & 15) == 0 &&
        (reinterpret_cast<uintptr_t>(argmax) & 7) == 0) {
        const int64_t nwin = nslots / 4;
        hipLaunchKernelGGL(unpool_relu_bwd_win_kernel, dim3((unsigned)((nwin + bs - 1) / bs)), dim3(bs), 0,
                           reinterpret_cast<hipStream_t>(stream), g, argmax, nwin, C, To, Ho, Wo, pool_t, T, OH, OW,
                           (uint4*)out_hi, (uint4*)out_lo, prec, scale);
        return (int)hipGetLastError();
    }
    hipLaunchKernelGGL(unpool_relu_bwd_kernel, dim3((unsigned)((nslots + bs - 1) / bs)), dim3(bs), 0,
                       reinterpret_cast<hipStream_t>(stream), g, argmax, nslots, C, To, Ho, Wo, pool_t, T, OH, OW,
                       g_layout, (uint4*)out_hi, (uint4*)out_lo, prec, scale);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// Power-of-two scale that brings max|g| to [target/2, target): single-pass fp16 operands keep their
// 11 bits only inside fp16's narrow exponent range, so gradients are scaled before the 16-bit
// conversion and the result is multiplied by 1/scale in the fp32 epilogue (exact: powers of two).
__global__ void absmax_kernel(const float* __restrict__ g, int64_t n, unsigned int* __restrict__ bits) {
    __shared__ float red[16];
    float m = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        m = fmaxf(m, fabsf(g[i]));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) red[w] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < (int)(blockDim.x >> 6); ++i) m = fmaxf(m, red[i]);
        atomicMax(bits, __float_as_uint(m));     // non-negative floats order like their bit patterns
    }
}

// value = mant * 2^(e - 23) with mant in [2^23, 2^24): exponent and significand of a positive finite float from its bits
// (subnormals normalised), so that the scale's exponent is integer arithmetic -- no log2f rounding at powers of two, no overflow
// of target / m for a subnormal maximum
__device__ __forceinline__ void float_decompose(unsigned int bits, int& e, unsigned int& mant) {
    e = (int)(bits >> 23);
    mant = bits & 0x7fffffu;
    if (e == 0) {
        const int sh = __clz(mant) - 8;
        mant <<= sh;
        e = 1 - sh;
    } else {
        mant |= 0x800000u;
    }
    e -= 127;
}

__global__ void scale_from_absmax_kernel(const unsigned int* __restrict__ bits, float target, float* __restrict__ out) {
    const unsigned int mb = bits[0], tb = __float_as_uint(target);
    int k = 0;       // scale 1: all-zero input, non-finite maximum, target not positive and finite
    if (mb != 0u && mb < 0x7f800000u && tb != 0u && tb < 0x7f800000u) {
        int em, et;
        unsigned int mm, mt;
        float_decompose(mb, em, mm);
        float_decompose(tb, et, mt);
        // the largest k with m * 2^k < target: significand of target above m's -> the exponent difference, else one less
        // (equal significands: m * 2^(et - em) == target, outside the half-open interval)
        k = et - em - (mt > mm ? 0 : 1);
        // the widest clamp under which 2^k and 2^-k are both normal floats.  (+-100, the clamp of the log2f version, would
        // break the interval for a maximum near FLT_MAX: 3e38 against a target of 1024 needs k = -118.)  A scale that far out
        // has no headroom left for a product with another scale (vd_scale_combine mode 0); the interval is what is promised.
        k = k < -126 ? -126 : (k > 126 ? 126 : k);
    }
    out[0] = __uint_as_float((unsigned int)(127 + k) << 23);
    out[1] = __uint_as_float((unsigned int)(127 - k) << 23);
}

extern "C" int vd_absmax_scale(const float* g, int64_t n, float target, float* out, void* stream) {
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    unsigned int* bits = reinterpret_cast<unsigned int*>(out + 2);
    hipError_t e = hipMemsetAsync(bits, 0, sizeof(unsigned int), st);
    if (e != hipSuccess) return (int)e;
    if (n > 0) {
        int64_t blocks = (n + 256 * 8 - 1) / (256 * 8);
        if (blocks > 1024) blocks = 1024;
        hipLaunchKernelGGL(absmax_kernel, dim3((unsigned)blocks), dim3(256), 0, st, g, n, bits);
    }
    hipLaunchKernelGGL(scale_from_absmax_kernel, dim3(1), dim3(1), 0, st, bits, target, out);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// DM class term: one workgroup per class; threads stride the feature dimension (coalesced
// rows of the [b][d] matrices), wave-shuffle + LDS reduction of the squared distance.
__global__ __launch_bounds__(1024) void dm_loss_kernel(const float* __restrict__ fr, const float* __restrict__ fs,
                                                        int nreal, int nsyn, int dim, float* __restrict__ loss,
                                                        float* __restrict__ gsyn) {
    __shared__ float red[16];
    const int c = blockIdx.x;
    const float* r = fr + (int64_t)c * nreal * dim;
    const float* s = fs + (int64_t)c * nsyn * dim;
    const float inv_r = 1.f / (float)nreal, inv_s = 1.f / (float)nsyn;
    float part = 0.f;
    for (int d = threadIdx.x; d < dim; d += blockDim.x) {
        // column sums: 8 independent loads in flight per thread (the kernel sits on the critical
        // path between the real-clip features and the backward pass; it is latency- not bandwidth-bound)
        float m[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        int b = 0;
        for (; b + 8 <= nreal; b += 8) {
#pragma unroll
            for (int k = 0; k < 8; ++k) m[k] += r[(int64_t)(b + k) * dim + d];
        }
        for (; b < nreal; ++b) m[0] += r[(int64_t)b * dim + d];
        const float mr = ((m[0] + m[1]) + (m[2] + m[3])) + ((m[4] + m[5]) + (m[6] + m[7]));
        float ms = 0.f;
        for (int k = 0; k < nsyn; ++k) ms += s[(int64_t)k * dim + d];
        const float diff = mr * inv_r - ms * inv_s;
        part += diff * diff;
        if (gsyn != nullptr) {
            const float gv = -2.f * diff * inv_s;
            for (int k = 0; k < nsyn; ++k) gsyn[((int64_t)c * nsyn + k) * dim + d] = gv;
        }
    }
    const float tot = block_sum(part, red);
    if (threadIdx.x == 0) loss[c] = tot;
}

extern "C" int vd_dm_loss(const float* feat_real, const float* feat_syn, int nclass, int nreal, int nsyn, int dim,
                          float* loss_per_class, float* g_syn, void* stream) {
    if (nclass <= 0) return 0;
    if (nreal <= 0 || nsyn <= 0 || dim <= 0) return -2;
    hipLaunchKernelGGL(dm_loss_kernel, dim3(nclass), dim3(1024), 0, reinterpret_cast<hipStream_t>(stream), feat_real,
                       feat_syn, nreal, nsyn, dim, loss_per_class, g_syn);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// out[g][d] = scale * sum_{b<per} x[g*per + b][d]  (per-class partial feature sums of a rank's slice
// of the real batch, exchanged by one all-reduce when the real batch is sharded over ranks)
__global__ void group_sum_kernel(const float* __restrict__ x, int per, int dim, float scale, float* __restrict__ out) {
    const int g = blockIdx.y;
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= dim) return;
    const float* r = x + (int64_t)g * per * dim + d;
    float m[4] = {0.f, 0.f, 0.f, 0.f};
    int b = 0;
    for (; b + 4 <= per; b += 4) {
#pragma unroll
        for (int k = 0; k < 4; ++k) m[k] += r[(int64_t)(b + k) * dim];
    }
    for (; b < per; ++b) m[0] += r[(int64_t)b * dim];
    out[(int64_t)g * dim + d] = ((m[0] + m[1]) + (m[2] + m[3])) * scale;
}

extern "C" int vd_group_sum(const float* x, int groups, int per, int dim, float scale, float* out, void* stream) {
    if (groups <= 0 || dim <= 0) return 0;
    if (per <= 0) return -2;
    hipLaunchKernelGGL(group_sum_kernel, dim3((dim + 255) / 256, groups), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), x, per, dim, scale, out);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------
__global__ void sgd_momentum_kernel(float* __restrict__ x, float* __restrict__ buf, const float* __restrict__ g,
                                    int64_t n, float lr, float mu, int first) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        // every operation rounded on its own (no fused multiply-add): the fp32 evaluation of the header's formula as written
#pragma clang fp contract(off)
        const float gv = g[i];
        const float prev = buf[i] * mu;
        const float b = first ? gv : prev + gv;
        buf[i] = b;
        const float step = lr * b;
        x[i] = x[i] - step;
    }
}

extern "C" int vd_sgd_momentum(float* x, float* buf, const float* g, int64_t n, float lr, float momentum, int first,
                               void* stream) {
    if (n <= 0) return 0;
    const int bs = 256;
    int64_t blocks = (n + bs - 1) / bs;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(sgd_momentum_kernel, dim3((unsigned)blocks), dim3(bs), 0, reinterpret_cast<hipStream_t>(stream),
                       x, buf, g, n, lr, momentum, first);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// Hallucinator (Conv3d 4->3, 3x3x3, pad 1 over [static x3 broadcast in T | dynamic x1]); utils.py:1178-1197.
//
// All three kernels give one thread a pixel column (clip, y, x) and walk the T frames with a sliding three-frame
// window in registers, so every input element is loaded once per thread instead of once per tap (the first version
// -- one thread per (clip, t, y, x), 108 loads each -- ran at 2-5 % of HBM bandwidth).  The static image does not
// depend on t, so its part of the convolution collapses to three 2-D sums S_kt per output channel, computed once
// per column; likewise its gradient needs only the temporal sum / first / last frame of the upstream gradient.
// The 324 weights are wave-uniform: they are read through the scalar path (constant indices after unrolling).
// HBM-bound: forward reads 4 and writes 3*T floats per pixel column of T frames; algorithmic bytes per clip =
// (3 + T + 3 T) * H * W * 4.
#define HAL_W(co, ci, kt, kh, kw) w[(((co) * 4 + (ci)) * 3 + (kt)) * 9 + (kh) * 3 + (kw)]

// The column walk of both forward kernels: output clip `clip`, pixel column `pix` = y * W + x of it, `sp` / `dp` the static
// image and the dynamic memory the clip is composed from, `w` / `b` its hallucinator (wave-uniform in both callers).
__device__ __forceinline__ void hal_fwd_column(int64_t clip, int pix, const float* __restrict__ sp, const float* __restrict__ dp,
                                               const float* __restrict__ w, const float* __restrict__ b, int T, int H, int W,
                                               float* __restrict__ out) {
    const int x = pix % W;
    const int y = pix / W;
    bool ok[9];
    int off[9];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int yy = y + a - 1, xx = x + c - 1;
            ok[a * 3 + c] = yy >= 0 && yy < H && xx >= 0 && xx < W;
            off[a * 3 + c] = yy * W + xx;
        }
    // static part: S[kt][co] = sum_{ci,kh,kw} w[co][ci][kt][kh][kw] * stat[ci][y+kh-1][x+kw-1]
    float S[3][3];
#pragma unroll
    for (int kt = 0; kt < 3; ++kt)
#pragma unroll
        for (int co = 0; co < 3; ++co) S[kt][co] = 0.f;
#pragma unroll
    for (int ci = 0; ci < 3; ++ci)
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const float v = ok[k] ? sp[(int64_t)ci * H * W + off[k]] : 0.f;
#pragma unroll
            for (int kt = 0; kt < 3; ++kt)
#pragma unroll
                for (int co = 0; co < 3; ++co) S[kt][co] += HAL_W(co, ci, kt, k / 3, k % 3) * v;
        }
    const float b0 = b[0], b1 = b[1], b2 = b[2];
    float d[3][9];         // dynamic frames t-1, t, t+1 (zero outside the clip)
#pragma unroll
    for (int k = 0; k < 9; ++k) { d[0][k] = 0.f; d[1][k] = ok[k] ? dp[off[k]] : 0.f; }
    const int64_t HW = (int64_t)H * W;
    for (int t = 0; t < T; ++t) {
        const bool nxt = t + 1 < T;
#pragma unroll
        for (int k = 0; k < 9; ++k) d[2][k] = (nxt && ok[k]) ? dp[(int64_t)(t + 1) * HW + off[k]] : 0.f;
        float a0 = b0 + S[1][0], a1 = b1 + S[1][1], a2 = b2 + S[1][2];
        if (t > 0) { a0 += S[0][0]; a1 += S[0][1]; a2 += S[0][2]; }
        if (nxt) { a0 += S[2][0]; a1 += S[2][1]; a2 += S[2][2]; }
#pragma unroll
        for (int kt = 0; kt < 3; ++kt)
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                const float v = d[kt][k];
                a0 += HAL_W(0, 3, kt, k / 3, k % 3) * v;
                a1 += HAL_W(1, 3, kt, k / 3, k % 3) * v;
                a2 += HAL_W(2, 3, kt, k / 3, k % 3) * v;
            }
        float* op = out + ((clip * T + t) * 3) * HW + (int64_t)y * W + x;
        op[0] = a0;
        op[HW] = a1;
        op[2 * HW] = a2;
#pragma unroll
        for (int k = 0; k < 9; ++k) { d[0][k] = d[1][k]; d[1][k] = d[2][k]; }
    }
}

__global__ __launch_bounds__(256) void hal_fwd_kernel(const float* __restrict__ stat, const float* __restrict__ dyn,
                                                       const int64_t* __restrict__ sidx, const int64_t* __restrict__ didx,
                                                       const float* __restrict__ w, const float* __restrict__ b,
                                                       int n, int T, int H, int W, float* __restrict__ out) {
    const int64_t total = (int64_t)n * H * W;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int64_t clip = i / ((int64_t)W * H);
    const int64_t si = sidx ? sidx[clip] : clip, di = didx ? didx[clip] : clip;
    hal_fwd_column(clip, (int)(i % ((int64_t)W * H)), stat + si * 3 * H * W, dyn + di * (int64_t)T * H * W, w, b, T, H, W, out);
}

// One hallucinator per clip (MultiStaticSharedDataset, utils.py:462-496): blockIdx.y = clip, blockIdx.x over its H*W pixel
// columns, so the set index hidx[blockIdx.y] -- and with it every one of the 324 weight addresses -- is block-uniform and the
// weights stay on the scalar path.  (Under the 1-D grid above a wave may span two clips: a per-thread set would turn the 81
// scalar operands per frame into vector loads.)
__global__ __launch_bounds__(256) void hal_fwd_multi_kernel(const float* __restrict__ stat, const float* __restrict__ dyn,
                                                             const int64_t* __restrict__ sidx, const int64_t* __restrict__ didx,
                                                             const int32_t* __restrict__ hidx, const float* __restrict__ w,
                                                             const float* __restrict__ b, int T, int H, int W,
                                                             float* __restrict__ out) {
    const int pix = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (pix >= H * W) return;
    const int64_t clip = blockIdx.y;
    const int64_t si = sidx ? sidx[clip] : clip, di = didx ? didx[clip] : clip;
    const int set = hidx ? hidx[clip] : 0;
    hal_fwd_column(clip, pix, stat + si * 3 * H * W, dyn + di * (int64_t)T * H * W, w + (int64_t)set * 324, b + (int64_t)set * 3,
                   T, H, W, out);
}

extern "C" int vd_hallucinator_fwd_multi(const float* stat, const float* dyn, const int64_t* sidx, const int64_t* didx,
                                         const int32_t* hidx, const float* w, const float* b, int nh, int n, int T, int H, int W,
                                         float* out, void* stream) {
    if (!stat || !dyn || !w || !b || !out || nh <= 0) return -1;
    if (n > 65535) return -2;          // gridDim.y
    if (n <= 0 || T <= 0 || H <= 0 || W <= 0) return 0;
    const int64_t hw = (int64_t)H * W;
    hipLaunchKernelGGL(hal_fwd_multi_kernel, dim3((unsigned)((hw + 255) / 256), (unsigned)n), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), stat, dyn, sidx, didx, hidx, w, b, T, H, W, out);
    return (int)hipGetLastError();
}

extern "C" int vd_hallucinator_fwd(const float* stat, const float* dyn, const int64_t* sidx, const int64_t* didx,
                                   const float* w, const float* b, int n, int T, int H, int W, float* out, void* stream) {
    const int64_t total = (int64_t)n * H * W;
    if (total <= 0 || T <= 0) return 0;
    hipLaunchKernelGGL(hal_fwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), stat, dyn, sidx, didx, w, b, n, T, H, W, out);
    return (int)hipGetLastError();
}

// Backward, data part.  One thread per (clip, y, x); nb[f][co][k] = upstream gradient of frames t-1, t, t+1 at the 3x3
// neighbourhood (k = a*3+c -> pixel (y+a-1, x+c-1); the tap it meets is (kh, kw) = (2-a, 2-c)):
//   g_dyn[didx[clip], t, y, x] += sum_{co,kt,k} nb[frame t-kt+1][co][k] * w[co][3][kt][2-a][2-c]
//   g_stat[sidx[clip], ci, y, x] += sum_{co,k} ( w[.,ci,1,.] * SUM + w[.,ci,0,.] * (SUM - FIRST) + w[.,ci,2,.] * (SUM - LAST) )
// with SUM / FIRST / LAST the temporal sum, first and last frame of the neighbourhood.  Both are accumulated with fp32
// atomics (several clips may share a memory; the caller passes zeroed buffers).
__global__ __launch_bounds__(256) void hal_bwd_data_kernel(const float* __restrict__ go, const int64_t* __restrict__ sidx,
                                                            const int64_t* __restrict__ didx, const float* __restrict__ w,
                                                            int n, int T, int H, int W, float* __restrict__ g_dyn,
                                                            float* __restrict__ g_stat) {
    const int64_t total = (int64_t)n * H * W;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int x = (int)(i % W);
    const int y = (int)((i / W) % H);
    const int64_t clip = i / ((int64_t)W * H);
    const int64_t HW = (int64_t)H * W;
    bool ok[9];
    int off[9];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int yy = y + a - 1, xx = x + c - 1;
            ok[a * 3 + c] = yy >= 0 && yy < H && xx >= 0 && xx < W;
            off[a * 3 + c] = yy * W + xx;
        }
    const float* gp = go + clip * (int64_t)T * 3 * HW;
    float nb[3][3][9], sum[3][9], first[3][9];
#pragma unroll
    for (int co = 0; co < 3; ++co)
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            nb[0][co][k] = 0.f;
            const float v = ok[k] ? gp[(int64_t)co * HW + off[k]] : 0.f;
            nb[1][co][k] = v; first[co][k] = v; sum[co][k] = 0.f;
        }
    const int64_t di = didx ? didx[clip] : clip;
    float* gd = g_dyn + di * (int64_t)T * HW + (int64_t)y * W + x;
    for (int t = 0; t < T; ++t) {
        const bool nxt = t + 1 < T;
#pragma unroll
        for (int co = 0; co < 3; ++co)
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                nb[2][co][k] = (nxt && ok[k]) ? gp[((int64_t)(t + 1) * 3 + co) * HW + off[k]] : 0.f;
                sum[co][k] += nb[1][co][k];
            }
        float acc = 0.f;
#pragma unroll
        for (int f = 0; f < 3; ++f)          // frame t+f-1 = t-kt+1  ->  kt = 2-f
#pragma unroll
            for (int co = 0; co < 3; ++co)
#pragma unroll
                for (int k = 0; k < 9; ++k) acc += nb[f][co][k] * HAL_W(co, 3, 2 - f, 2 - k / 3, 2 - k % 3);
        atomicAdd(gd + (int64_t)t * HW, acc);
        if (nxt) {
#pragma unroll
            for (int co = 0; co < 3; ++co)
#pragma unroll
                for (int k = 0; k < 9; ++k) { nb[0][co][k] = nb[1][co][k]; nb[1][co][k] = nb[2][co][k]; }
        }
    }
    if (g_stat != nullptr) {       // nb[1] is now the LAST frame
        const int64_t si = sidx ? sidx[clip] : clip;
#pragma unroll
        for (int ci = 0; ci < 3; ++ci) {
            float acc = 0.f;
#pragma unroll
            for (int co = 0; co < 3; ++co)
#pragma unroll
                for (int k = 0; k < 9; ++k) {
                    const int kh = 2 - k / 3, kw = 2 - k % 3;
                    const float sm = sum[co][k];
                    acc += HAL_W(co, ci, 1, kh, kw) * sm + HAL_W(co, ci, 0, kh, kw) * (sm - first[co][k]) +
                           HAL_W(co, ci, 2, kh, kw) * (sm - nb[1][co][k]);
                }
            atomicAdd(&g_stat[(si * 3 + ci) * HW + (int64_t)y * W + x], acc);
        }
    }
}

// Backward, parameter part.  grid.y = job: 0..2 -> the 27 weights of the dynamic input channel for output channel job
// (+ its bias gradient), 3..5 -> the 81 weights of the three static input channels for output channel job-3.  A thread
// strides over pixel columns (clip, y, x) with its accumulators in registers and walks the frames of a column once.  The
// jobs are kept small (<= 81 accumulators, dynamic jobs ~70 registers) on purpose: the frame walk is a chain of dependent
// load -> FMA steps, so it is thread-level parallelism (many resident waves), not per-thread work, that hides the memory
// latency (a single 84-accumulator job for all three output channels ran 4x slower at two waves per SIMD).
// For the static channels  g_w[co][ci][kt][kh][kw] = sum_{y,x} stat[ci][y+kh-1][x+kw-1] * G_kt[co][y][x]  with G_kt the
// temporal sum of the upstream gradient over the frames whose tap kt is inside the clip (all / all but the first / last).
__global__ __launch_bounds__(256) void hal_bwd_param_kernel(const float* __restrict__ go, const float* __restrict__ stat,
                                                             const float* __restrict__ dyn, const int64_t* __restrict__ sidx,
                                                             const int64_t* __restrict__ didx, int n, int T, int H, int W,
                                                             float* __restrict__ g_w, float* __restrict__ g_b) {
    __shared__ float part[4][81];
    const int job = blockIdx.y;
    const int64_t total = (int64_t)n * H * W;
    const int64_t HW = (int64_t)H * W;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (job < 3) {
        const int co = job;
        float acc[27], accb = 0.f;
#pragma unroll
        for (int k = 0; k < 27; ++k) acc[k] = 0.f;
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
            const int x = (int)(i % W);
            const int y = (int)((i / W) % H);
            const int64_t clip = i / HW;
            const int64_t di = didx ? didx[clip] : clip;
            const float* dp = dyn + di * (int64_t)T * HW + (int64_t)y * W + x;
            const float* gp = go + (clip * (int64_t)T * 3 + co) * HW + (int64_t)y * W + x;
            unsigned okm = 0;
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                const int yy = y + k / 3 - 1, xx = x + k % 3 - 1;
                if (yy >= 0 && yy < H && xx >= 0 && xx < W) okm |= 1u << k;
            }
            float d[3][9];
#pragma unroll
            for (int k = 0; k < 9; ++k) { d[0][k] = 0.f; d[1][k] = ((okm >> k) & 1) ? dp[(k / 3 - 1) * W + (k % 3 - 1)] : 0.f; }
            for (int t = 0; t < T; ++t) {
                const bool nxt = t + 1 < T;
#pragma unroll
                for (int k = 0; k < 9; ++k)
                    d[2][k] = (nxt && ((okm >> k) & 1)) ? dp[(int64_t)(t + 1) * HW + (k / 3 - 1) * W + (k % 3 - 1)] : 0.f;
                const float g = gp[(int64_t)t * 3 * HW];
                accb += g;
#pragma unroll
                for (int kt = 0; kt < 3; ++kt)
#pragma unroll
                    for (int k = 0; k < 9; ++k) acc[kt * 9 + k] += g * d[kt][k];
#pragma unroll
                for (int k = 0; k < 9; ++k) { d[0][k] = d[1][k]; d[1][k] = d[2][k]; }
            }
        }
#pragma unroll
        for (int k = 0; k < 27; ++k) {
            const float tot = wave_sum(acc[k]);
            if (lane == 0) part[wv][k] = tot;
        }
        const float tb = wave_sum(accb);
        if (lane == 0) part[wv][27] = tb;
        __syncthreads();
        if (threadIdx.x < 28) {
            const int k = threadIdx.x;
            const float tot = part[0][k] + part[1][k] + part[2][k] + part[3][k];
            if (k < 27) atomicAdd(&g_w[(co * 4 + 3) * 27 + k], tot);                 // [co][ci=3][kt][kh][kw]
            else atomicAdd(&g_b[co], tot);
        }
        return;
    }
    const int co = job - 3;
    float acc[81];
#pragma unroll
    for (int k = 0; k < 81; ++k) acc[k] = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % W);
        const int y = (int)((i / W) % H);
        const int64_t clip = i / HW;
        const float* gp = go + (clip * (int64_t)T * 3 + co) * HW + (int64_t)y * W + x;
        float gs = 0.f, gfirst = 0.f, glast = 0.f;
        for (int t = 0; t < T; ++t) {
            const float g = gp[(int64_t)t * 3 * HW];
            gs += g;
            if (t == 0) gfirst = g;
            if (t == T - 1) glast = g;
        }
        const float G[3] = {gs - gfirst, gs, gs - glast};      // kt = 0: frames 1..T-1; kt = 1: all; kt = 2: frames 0..T-2
        const int64_t si = sidx ? sidx[clip] : clip;
        const float* sp = stat + si * 3 * HW + (int64_t)y * W + x;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const int yy = y + k / 3 - 1, xx = x + k % 3 - 1;
            const bool ok = yy >= 0 && yy < H && xx >= 0 && xx < W;
#pragma unroll
            for (int ci = 0; ci < 3; ++ci) {
                const float v = ok ? sp[(int64_t)ci * HW + (k / 3 - 1) * W + (k % 3 - 1)] : 0.f;
#pragma unroll
                for (int kt = 0; kt < 3; ++kt) acc[(ci * 3 + kt) * 9 + k] += G[kt] * v;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 81; ++k) {
        const float tot = wave_sum(acc[k]);
        if (lane == 0) part[wv][k] = tot;
    }
    __syncthreads();
    if (threadIdx.x < 81) {
        const int k = threadIdx.x;
        atomicAdd(&g_w[(co * 4 + k / 27) * 27 + (k % 27)], part[0][k] + part[1][k] + part[2][k] + part[3][k]);   // [co][ci][kt][kh][kw]
    }
}

// Backward, FUSED (round 5): the upstream gradient is read from HBM ONCE.  (The two kernels above read it three times -- the data
// part once through the L1 with nine requests per element, the parameter part once per job group -- and ran at 1.28 / 0.89 TB/s of
// algorithmic bytes.)  A workgroup owns a tile of 8 x 32 pixels of one clip and walks its T frames; the tile + one-pixel halo of
// the upstream gradient (3 channels) and of the dynamic memory is staged per frame into a three-slot ring in LDS (the loads of
// frame t + 2 are in flight while frame t is computed), and every thread reads its 3 x 3 x 3 neighbourhoods from there:
//   * g_dyn of its pixel and frame (81 multiply-adds with scalar weights), added with an atomic (clips may share a memory);
//   * the dynamic channel's 81 weight gradients + the bias gradient, accumulated in registers over all tiles of the workgroup;
//   * per pixel of tile + halo the temporal SUM / FIRST / LAST of the upstream gradient; after the walk g_stat of its pixel
//     gathers them (243 multiply-adds once per column);
//   * the static channels' 243 weight gradients are the 27 x 9 product (stat neighbourhood) x (G_kt[co] of the centre pixel)
//     summed over pixels -- a small GEMM with the pixel as K: each wave runs it over its 64 columns on the fp32 matrix
//     instruction (v_mfma_f32_32x32x2f32, operands straight from the LDS tiles), accumulators kept across tiles.
// Grid-stride over tiles (<= 512 workgroups), one closing reduction + 327 atomics per workgroup.
#define HAL_TH 8
#define HAL_TW 32
#define HAL_PITCH 36
#define HAL_HALO ((HAL_TH + 2) * (HAL_TW + 2))          // 340 pixels of tile + halo
#define HAL_AREA ((HAL_TH + 2) * HAL_PITCH)             // 360 floats per staged channel
typedef float hal_f32x16 __attribute__((ext_vector_type(16)));

__global__ __launch_bounds__(256, 2) void hal_bwd_fused_kernel(const float* __restrict__ go, const float* __restrict__ stat,
                                                               const float* __restrict__ dyn, const int64_t* __restrict__ sidx,
                                                               const int64_t* __restrict__ didx, const float* __restrict__ w,
                                                               int n, int T, int H, int W, int tiles_x, int tiles_y,
                                                               float* __restrict__ g_dyn, float* __restrict__ g_stat,
                                                               float* __restrict__ g_w, float* __restrict__ g_b) {
    __shared__ float go_w[3][3][HAL_AREA];       // ring slot, channel
    __shared__ float dy_w[3][HAL_AREA];
    __shared__ float sfl[3][3][HAL_AREA];        // SUM / FIRST / LAST, channel
    __shared__ float st_t[3][HAL_AREA];          // static tile
    __shared__ float g_t[256][9];                // G_kt[co] of every centre pixel: [kt * 3 + co]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int ly = tid / HAL_TW, lx = tid % HAL_TW;
    const int ctr = (ly + 1) * HAL_PITCH + lx + 1;          // this thread's pixel inside a staged channel
    const int64_t HW = (int64_t)H * W;
    const int64_t ntiles = (int64_t)n * tiles_x * tiles_y;
    // halo-inclusive pixels this thread stages / sums: p0 = tid, p1 = tid + 256 (< 340)
    const int p0 = tid, p1 = tid + 256;
    const bool has1 = p1 < HAL_HALO;
    const int h0y = p0 / (HAL_TW + 2), h0x = p0 % (HAL_TW + 2);
    const int h1y = has1 ? p1 / (HAL_TW + 2) : 0, h1x = has1 ? p1 % (HAL_TW + 2) : 0;
    const int l0 = h0y * HAL_PITCH + h0x, l1 = h1y * HAL_PITCH + h1x;
    float accw[81];          // d/d w[co][3][kt][kh][kw]: index co * 27 + kt * 9 + kh * 3 + kw
#pragma unroll
    for (int k = 0; k < 81; ++k) accw[k] = 0.f;
    float accb[3] = {0.f, 0.f, 0.f};
    hal_f32x16 accs;         // static channels: rows r = ci * 9 + kh * 3 + kw (27 of 32), columns kt * 3 + co (9 of 32)
#pragma unroll
    for (int k = 0; k < 16; ++k) accs[k] = 0.f;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t clip = tile / (tiles_x * tiles_y);
        const int tr = (int)(tile % (tiles_x * tiles_y));
        const int ty0 = (tr / tiles_x) * HAL_TH, tx0 = (tr % tiles_x) * HAL_TW;
        const int64_t si = sidx ? sidx[clip] : clip, di = didx ? didx[clip] : clip;
        const float* gp = go + clip * (int64_t)T * 3 * HW;
        const float* dp = dyn + di * (int64_t)T * HW;
        const float* sp = stat + si * 3 * HW;
        // image coordinates of the two staged pixels
        const int y0 = ty0 - 1 + h0y, x0 = tx0 - 1 + h0x, y1 = ty0 - 1 + h1y, x1 = tx0 - 1 + h1x;
        const bool in0 = y0 >= 0 && y0 < H && x0 >= 0 && x0 < W;
        const bool in1 = has1 && y1 >= 0 && y1 < H && x1 >= 0 && x1 < W;
        const int64_t o0 = in0 ? (int64_t)y0 * W + x0 : 0, o1 = in1 ? (int64_t)y1 * W + x1 : 0;
        float r0[4], r1[4];         // staged values of one frame: go[0..2], dyn
        auto fetch = [&](int t) {
            const bool tv = t >= 0 && t < T;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                r0[c] = (tv && in0) ? gp[((int64_t)t * 3 + c) * HW + o0] : 0.f;
                r1[c] = (tv && in1) ? gp[((int64_t)t * 3 + c) * HW + o1] : 0.f;
            }
            r0[3] = (tv && in0) ? dp[(int64_t)t * HW + o0] : 0.f;
            r1[3] = (tv && in1) ? dp[(int64_t)t * HW + o1] : 0.f;
        };
        auto stage = [&](int slot) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                go_w[slot][c][l0] = r0[c];
                if (has1) go_w[slot][c][l1] = r1[c];
            }
            dy_w[slot][l0] = r0[3];
            if (has1) dy_w[slot][l1] = r1[3];
        };
        // static tile; ring slots: frame t lives in slot (t + 3) % 3, frame -1 is zeros
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            st_t[c][l0] = in0 ? sp[(int64_t)c * HW + o0] : 0.f;
            if (has1) st_t[c][l1] = in1 ? sp[(int64_t)c * HW + o1] : 0.f;
        }
        fetch(-1); stage(2);
        fetch(0); stage(0);
        fetch(1); stage(1);
        float s0[3] = {0.f, 0.f, 0.f}, s1[3] = {0.f, 0.f, 0.f}, f0[3], f1[3], e0[3], e1[3];      // SUM, FIRST, LAST of the two staged pixels
#pragma unroll
        for (int c = 0; c < 3; ++c) { f0[c] = 0.f; f1[c] = 0.f; e0[c] = 0.f; e1[c] = 0.f; }
        const int gy = ty0 + ly, gx = tx0 + lx;
        const bool valid = gy < H && gx < W;
        float* gd = g_dyn + di * (int64_t)T * HW + (int64_t)gy * W + gx;
        __syncthreads();
        // data gradient in SCATTER form: the 27 upstream values of frame tau (3 channels x 3 x 3 neighbours) are read from LDS once
        // and added into the three outputs they meet -- out[tau + 1] through tap kt = 2, out[tau] through kt = 1, out[tau - 1]
        // through kt = 0 -- so a step reads 27 values instead of the 81 of its three-frame window
        float o0a = 0.f, o1a = 0.f, o2a = 0.f;             // outputs t, t + 1, t + 2 under construction
        auto scatter = [&](int slot) {
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                const int off = ctr + (k / 3 - 1) * HAL_PITCH + (k % 3 - 1);
                const int kh = 2 - k / 3, kw = 2 - k % 3;
#pragma unroll
                for (int co = 0; co < 3; ++co) {
                    const float v = go_w[slot][co][off];
                    o0a += v * HAL_W(co, 3, 0, kh, kw);
                    o1a += v * HAL_W(co, 3, 1, kh, kw);
                    o2a += v * HAL_W(co, 3, 2, kh, kw);
                }
            }
        };
        scatter(0);                                        // frame 0 -> out[-1] (dropped), out[0], out[1]
        o0a = o1a; o1a = o2a; o2a = 0.f;
        for (int t = 0; t < T; ++t) {
            fetch(t + 2);                                  // lands under this frame's arithmetic
            const int sm1 = (t + 2) % 3, sc = t % 3, sp1 = (t + 1) % 3;      // slots of frames t - 1, t, t + 1
            // temporal sums of the staged pixels
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float a = go_w[sc][c][l0];
                s0[c] += a;
                if (t == 0) f0[c] = a;
                if (t == T - 1) e0[c] = a;
                if (has1) {
                    const float b = go_w[sc][c][l1];
                    s1[c] += b;
                    if (t == 0) f1[c] = b;
                    if (t == T - 1) e1[c] = b;
                }
            }
            scatter(sp1);                                  // frame t + 1 (zeros past the clip): completes out[t]
            if (valid) atomicAdd(gd + (int64_t)t * HW, o0a);
            o0a = o1a; o1a = o2a; o2a = 0.f;
            // the dynamic channel's weight gradients: g(t) at the centre x dyn(t + kt - 1) at the neighbours
            const float gc0 = go_w[sc][0][ctr], gc1 = go_w[sc][1][ctr], gc2 = go_w[sc][2][ctr];
            accb[0] += gc0; accb[1] += gc1; accb[2] += gc2;
#pragma unroll
            for (int f = 0; f < 3; ++f) {
                const int slot = (f == 0) ? sm1 : (f == 1) ? sc : sp1;
#pragma unroll
                for (int k = 0; k < 9; ++k) {
                    const float d = dy_w[slot][ctr + (k / 3 - 1) * HAL_PITCH + (k % 3 - 1)];
                    accw[0 * 27 + f * 9 + k] += gc0 * d;
                    accw[1 * 27 + f * 9 + k] += gc1 * d;
                    accw[2 * 27 + f * 9 + k] += gc2 * d;
                }
            }
            __syncthreads();                               // everybody is done with frame t - 1's slot ...
            stage(sm1);                                    // ... which takes frame t + 2
            __syncthreads();
        }
        // SUM / FIRST / LAST tiles
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            sfl[0][c][l0] = s0[c]; sfl[1][c][l0] = f0[c]; sfl[2][c][l0] = e0[c];
            if (has1) { sfl[0][c][l1] = s1[c]; sfl[1][c][l1] = f1[c]; sfl[2][c][l1] = e1[c]; }
        }
        __syncthreads();
        {   // G_kt[co] of the centre pixel: kt = 0: frames 1..T-1; kt = 1: all; kt = 2: frames 0..T-2
#pragma unroll
            for (int co = 0; co < 3; ++co) {
                const float sm = sfl[0][co][ctr], fi = sfl[1][co][ctr], la = sfl[2][co][ctr];
                g_t[tid][0 * 3 + co] = sm - fi; g_t[tid][1 * 3 + co] = sm; g_t[tid][2 * 3 + co] = sm - la;
            }
        }
        if (g_stat != nullptr && valid) {
#pragma unroll
            for (int ci = 0; ci < 3; ++ci) {
                float a = 0.f;
#pragma unroll
                for (int co = 0; co < 3; ++co)
#pragma unroll
                    for (int k = 0; k < 9; ++k) {
                        const int off = ctr + (k / 3 - 1) * HAL_PITCH + (k % 3 - 1);
                        const int kh = 2 - k / 3, kw = 2 - k % 3;
                        const float sm = sfl[0][co][off];
                        a += HAL_W(co, ci, 1, kh, kw) * sm + HAL_W(co, ci, 0, kh, kw) * (sm - sfl[1][co][off]) +
                             HAL_W(co, ci, 2, kh, kw) * (sm - sfl[2][co][off]);
                    }
                atomicAdd(&g_stat[(si * 3 + ci) * HW + (int64_t)gy * W + gx], a);
            }
        }
        __syncthreads();                                   // g_t complete
        if (g_w != nullptr) {
            // static channels: C[r][j] += sum over this wave's 64 columns of A[r][col] * B[col][j]; A = static value at the column's
            // neighbour (ci, kh, kw), B = G_j of the column.  v_mfma_f32_32x32x2f32: lane l supplies A[row l % 32][k = l / 32] and
            // B[k = l / 32][column l % 32]
            const int r = lane & 31, kk = lane >> 5;
            const int ci = r / 9, kh = (r % 9) / 3, kw = r % 3;
#pragma unroll 4
            for (int stp = 0; stp < 32; ++stp) {
                const int col = wv * 64 + stp * 2 + kk;            // a thread index = a tile pixel
                const int cy = col / HAL_TW, cx = col % HAL_TW;
                const float a = (r < 27) ? st_t[ci][(cy + kh) * HAL_PITCH + cx + kw] : 0.f;
                const float b = (r < 9) ? g_t[col][r] : 0.f;
                accs = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, accs, 0, 0, 0);
            }
        }
        __syncthreads();                                   // tiles free for the next walk
    }
    if (g_w == nullptr || g_b == nullptr) return;
    // closing reduction: 81 + 3 per-thread sums and the 27 x 9 matrix of every wave -> atomics
    float* red = &go_w[0][0][0];                           // [4 waves][84 + 243] floats (the ring is free now)
#pragma unroll
    for (int k = 0; k < 81; ++k) {
        const float tot = wave_sum(accw[k]);
        if (lane == 0) red[wv * 327 + k] = tot;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float tot = wave_sum(accb[c]);
        if (lane == 0) red[wv * 327 + 81 + c] = tot;
    }
    {   // 32 x 32 accumulator layout: lane l holds column l % 32, rows 8 * (v / 4) + 4 * (l / 32) + v % 4 for v = 0..15
        const int j = lane & 31;
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int r = 8 * (v / 4) + 4 * (lane >> 5) + (v % 4);
            if (j < 9 && r < 27) red[wv * 327 + 84 + r * 9 + j] = accs[v];
        }
    }
    __syncthreads();
    for (int k = tid; k < 327; k += 256) {
        const float tot = red[k] + red[327 + k] + red[2 * 327 + k] + red[3 * 327 + k];
        if (k < 81) {
            const int co = k / 27;
            atomicAdd(&g_w[(co * 4 + 3) * 27 + (k % 27)], tot);              // [co][ci = 3][kt][kh][kw]
        } else if (k < 84) {
            atomicAdd(&g_b[k - 81], tot);
        } else {
            const int r = (k - 84) / 9, j = (k - 84) % 9;                    // r = ci * 9 + kh * 3 + kw, j = kt * 3 + co
            const int ci = r / 9, co = j % 3, kt = j / 3;
            atomicAdd(&g_w[((co * 4 + ci) * 3 + kt) * 9 + (r % 9)], tot);
        }
    }
}

extern "C" int vd_hallucinator_bwd(const float* g_out, const float* stat, const float* dyn, const int64_t* sidx,
                                   const int64_t* didx, const float* w, int n, int T, int H, int W, float* g_dyn,
                                   float* g_stat, float* g_w, float* g_b, void* stream) {
    const int64_t total = (int64_t)n * H * W;
    if (total <= 0 || T <= 0) return 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    // 1 (default): the fused kernel where the launch has >= 1024 tiles (50 clips 112 x 112: 2800; measured 0.301 vs 0.330 ms, the
    // upstream gradient read once instead of three times) -- below that its <= 512 persistent workgroups do not fill the chip and the
    // two-kernel form is the faster one (7 clips 64 x 64 x 8: 0.056 vs 0.046 ms); 2: always fused; 0: never (tools/hal_check.py).
    // Both forms are bound by vector-ALU and LDS issue (162 multiply-adds and ~110 LDS reads per pixel and frame), not by HBM:
    // 203 MB of algorithmic traffic in 0.3 ms
    static const int fused = getenv("VD_HAL_FUSED") ? atoi(getenv("VD_HAL_FUSED")) : 1;
    const int tiles_x = (W + HAL_TW - 1) / HAL_TW, tiles_y = (H + HAL_TH - 1) / HAL_TH;
    // Ordered mode (vd_set_deterministic / VD_DETERMINISTIC): both forms close with one fp32 atomic per workgroup onto the
    // same <= 327 parameter-gradient addresses, in whatever order the workgroups finish.  The ordered form is the two-kernel one with
    // ONE workgroup per parameter job: its threads walk the pixel columns in a fixed order, the wave and workgroup sums have a fixed
    // order, and each address takes a single add onto the caller's zero.  (g_dyn / g_stat take one add per element and clip: they
    // are order-free wherever no two clips share a memory row, which is how utils.Conv3DNet calls this.)  Slow at full size -- one
    // workgroup walks every column -- and meant for reproducing a run, not for timing one.
    const bool ordered = vd_get_deterministic() != 0;
    if (!ordered && fused && (g_w != nullptr) == (g_b != nullptr) && (fused >= 2 || (int64_t)n * tiles_x * tiles_y >= 1024)) {
        int64_t grid = (int64_t)n * tiles_x * tiles_y;
        if (grid > 512) grid = 512;
        hipLaunchKernelGGL(hal_bwd_fused_kernel, dim3((unsigned)grid), dim3(256), 0, st, g_out, stat, dyn, sidx, didx, w, n, T, H, W,
                           tiles_x, tiles_y, g_dyn, g_stat, g_w, g_b);
        return (int)hipGetLastError();
    }
    hipLaunchKernelGGL(hal_bwd_data_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, g_out, sidx, didx,
                       w, n, T, H, W, g_dyn, g_stat);
    int e = (int)hipGetLastError();
    if (e) return e;
    if (g_w != nullptr && g_b != nullptr) {
        int64_t chunks = (total + 255) / 256;
        // (256 blocks per job: more blocks cost more in the closing atomics -- every block adds onto the same <= 81 addresses --
        //  than they gain in parallelism: 0.17 ms at 256, 0.25 at 1024, 0.43 at 2560 for 50 clips 112x112x16)
        if (chunks > 256) chunks = 256;
        if (ordered) chunks = 1;
        hipLaunchKernelGGL(hal_bwd_param_kernel, dim3((unsigned)chunks, 6), dim3(256), 0, st, g_out, stat, dyn, sidx,
                           didx, n, T, H, W, g_w, g_b);
        e = (int)hipGetLastError();
    }
    return e;
}

// ------------------------------------------------------------------------------------------
// match_loss row reductions.  Short rows (len <= 64, e.g. the 7-wide rows of the 5-D Conv3d
// gradients): one lane-group per row, 64/grp rows per wave.  Long rows: a wave per row.
__host__ __device__ inline int64_t vd_match_blocks(int64_t rows, int len) {
    int64_t blocks = (len == 1) ? (rows + 1023) / 1024 : (len <= 8) ? (rows + 255) / 256 : (rows + 3) / 4;
    if (blocks > 1024) blocks = 1024;
    if (blocks < 1) blocks = 1;
    return blocks;
}

// forward: every block ends with 5 atomics onto the SAME 5 accumulators, which the L2 serialises (~8 ns each): with
// up to 1024 blocks per tensor the closing atomics were 120 of the kernel's 130 us; 96 long-running blocks per tensor
// keep the loads in flight (grid-stride) and cut them to a few us.
__host__ __device__ inline int64_t vd_match_blocks_fwd(int64_t rows, int len) {
    const int64_t b = vd_match_blocks(rows, len);
    return b > 96 ? 96 : b;          // (same-box, with one sum per block: 48 / 96 / 192 / 384 blocks -> 16.8 / 12.6 / 14.2 / 21.4 us per gradient list)
}

// Short rows (len <= 8: the 7-wide rows of the 5-D Conv3d gradients are 99.8 % of a ConvNet3D gradient list).  A thread per row
// reading its own 28 bytes made every load instruction touch 64 x 28 B for 256 B used (1.4 TB/s for the list); here a wave takes
// 64 consecutive rows = 64 * len consecutive floats with coalesced loads and hands every lane its row through LDS (row pitch
// len | 1 floats: conflict-free).  All waves run the same number of rounds (block barriers inside).
#define VD_MATCH_SHORT_PITCH 9
#define VD_MATCH_FWD_THREADS 512          // forward blocks: the closing atomics cap their number (vd_match_blocks_fwd), not their size
struct VdMatchStage { float r[8][64 * VD_MATCH_SHORT_PITCH]; float s[8][64 * VD_MATCH_SHORT_PITCH]; };      // up to 8 waves per block

__device__ __forceinline__ int64_t match_short_rounds(int64_t rows, int64_t nblk) {
    const int64_t per = nblk * (blockDim.x >> 6) * 64;
    return (rows + per - 1) / per;
}

__device__ __forceinline__ int64_t match_short_row0(int64_t it, int64_t nblk) {      // first row of this wave's chunk in round ``it``
    return ((it * nblk + blockIdx.x) * (blockDim.x >> 6) + (threadIdx.x >> 6)) * 64;
}

__device__ __forceinline__ int match_short_count(int64_t rows, int len, int64_t r0) {      // floats in the chunk
    const int64_t left = rows - r0;
    return (int)(left < 64 ? (left < 0 ? 0 : left) : 64) * len;
}

// the chunk's 64 * len consecutive floats of both tensors, coalesced, into registers (element j * 64 + lane in slot j)
__device__ __forceinline__ void match_short_load(const float* __restrict__ gr, const float* __restrict__ gs, int64_t rows, int len,
                                                 int64_t r0, float (&x)[8], float (&y)[8]) {
    const int lane = threadIdx.x & 63, n = match_short_count(rows, len, r0);
    const int64_t base = r0 * len;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int idx = j * 64 + lane;
        const bool in = j < len && idx < n;
        x[j] = in ? gr[base + idx] : 0.f;
        y[j] = in ? gs[base + idx] : 0.f;
    }
}

// registers -> LDS: afterwards lane l of wave w finds row r0 + l at st.r[w][l * (len | 1) + k].  Block barriers on both sides.
__device__ __forceinline__ void match_short_put(VdMatchStage& st, int len, int n, const float (&x)[8], const float (&y)[8]) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, ls = len | 1, magic = 65536 / len + 1;
    __syncthreads();                      // the previous round's reads are done
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int idx = j * 64 + lane;
        if (j < len && idx < n) {
            const int row = (idx * magic) >> 16, k = idx - row * len;      // idx / len, exact for idx < 512, len <= 8
            st.r[w][row * ls + k] = x[j];
            st.s[w][row * ls + k] = y[j];
        }
    }
    __syncthreads();
}

__device__ __forceinline__ void match_rows_fwd_body(const float* __restrict__ gr, const float* __restrict__ gs,
                                                    int64_t rows, int len, float* __restrict__ acc, const int64_t nblk, const bool flat,
                                                    const int need = 31) {
    __shared__ float red[16];
    float s_cos = 0.f, s_mse = 0.f, s_dot = 0.f, s_rr = 0.f, s_ss = 0.f;
    if (flat) {
        // flat sums ('mse' / 'cos' metrics): 16-byte loads, grid-stride
        const int64_t n4 = rows >> 2;
        const float4* r4 = reinterpret_cast<const float4*>(gr);
        const float4* s4 = reinterpret_cast<const float4*>(gs);
        const bool aligned = ((reinterpret_cast<uintptr_t>(gr) | reinterpret_cast<uintptr_t>(gs)) & 15) == 0;
        const int64_t tid0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nt = (int64_t)nblk * blockDim.x;
        int64_t done = 0;
        if (aligned) {
            for (int64_t i = tid0; i < n4; i += nt) {
                const float4 x = r4[i], y = s4[i];
                s_dot += x.x * y.x + x.y * y.y + x.z * y.z + x.w * y.w;
                s_rr += x.x * x.x + x.y * x.y + x.z * x.z + x.w * x.w;
                s_ss += y.x * y.x + y.y * y.y + y.z * y.z + y.w * y.w;
                s_mse += (y.x - x.x) * (y.x - x.x) + (y.y - x.y) * (y.y - x.y) + (y.z - x.z) * (y.z - x.z) + (y.w - x.w) * (y.w - x.w);
            }
            done = n4 << 2;
        }
        for (int64_t i = done + tid0; i < rows; i += nt) {
            const float x = gr[i], y = gs[i];
            s_dot += x * y; s_rr += x * x; s_ss += y * y; s_mse += (y - x) * (y - x);
        }
    } else if (len <= 8) {
        // one thread per row, rows staged through LDS; the next round's loads fly under this round's sums
        __shared__ VdMatchStage st;
        const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, ls = len | 1;
        const int64_t rounds = match_short_rounds(rows, nblk);
        float x[8], y[8];
        match_short_load(gr, gs, rows, len, match_short_row0(0, nblk), x, y);
        for (int64_t it = 0; it < rounds; ++it) {
            const int64_t r0 = match_short_row0(it, nblk);
            match_short_put(st, len, match_short_count(rows, len, r0), x, y);
            if (it + 1 < rounds) match_short_load(gr, gs, rows, len, match_short_row0(it + 1, nblk), x, y);
            if (r0 + lane < rows) {
                float d = 0.f, a = 0.f, b = 0.f, m = 0.f;
                for (int k = 0; k < len; ++k) {
                    const float u = st.r[w][lane * ls + k], v = st.s[w][lane * ls + k];
                    d += u * v; a += u * u; b += v * v; m += (v - u) * (v - u);
                }
                s_cos += 1.f - d / (sqrtf(a) * sqrtf(b) + 0.000001f);
                s_mse += m; s_dot += d; s_rr += a; s_ss += b;
            }
        }
    } else {
        // one wave per row
        const int lane = threadIdx.x & 63;
        const int64_t wid = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
        const int64_t nw = ((int64_t)nblk * blockDim.x) >> 6;
        for (int64_t r = wid; r < rows; r += nw) {
            float d = 0.f, a = 0.f, b = 0.f, m = 0.f;
            for (int k = lane; k < len; k += 64) {
                const float x = gr[r * len + k], y = gs[r * len + k];
                d += x * y; a += x * x; b += y * y; m += (y - x) * (y - x);
            }
            d = wave_sum(d); a = wave_sum(a); b = wave_sum(b); m = wave_sum(m);
            if (lane == 0) {
                s_cos += 1.f - d / (sqrtf(a) * sqrtf(b) + 0.000001f);
                s_mse += m; s_dot += d; s_rr += a; s_ss += b;
            }
        }
    }
    float v[5] = {s_cos, s_mse, s_dot, s_rr, s_ss};
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        // (same-address atomics cost ~11 ns each at the L2 and pile up at the end of the launch: 6.5 of 19 us for a ConvNet3D
        //  gradient list with all five sums; a caller that needs one sum says so -- VdMatchBatch.reserved)
        if (!((need >> k) & 1)) continue;
        const float tot = block_sum(v[k], red);
        if (threadIdx.x == 0) atomicAdd(&acc[k], tot);
    }
}

__global__ __launch_bounds__(VD_MATCH_FWD_THREADS) void match_rows_fwd_kernel(const float* __restrict__ gr, const float* __restrict__ gs,
                                                              int64_t rows, int len, float* __restrict__ acc) {
    match_rows_fwd_body(gr, gs, rows, len, acc, gridDim.x, false);      // [rows][len] is a ROW view for every len (vd_hip.h)
}

// all tensors of a gradient list in ONE launch: blockIdx.y = segment (a match_loss call used to be 8 launches of
// 5-35 us each, i.e. launch-bound at 2-3 % of HBM bandwidth)
__global__ __launch_bounds__(VD_MATCH_FWD_THREADS) void match_rows_fwd_multi_kernel(const VdMatchBatch b, float* __restrict__ acc) {
    const VdMatchSeg& sg = b.seg[blockIdx.y];
    const int64_t nblk = vd_match_blocks_fwd(sg.rows, sg.reserved ? 1 : (sg.len == 1 ? 2 : sg.len));
    if ((int64_t)blockIdx.x >= nblk) return;
    match_rows_fwd_body(sg.gr, sg.gs, sg.rows, sg.len, acc, nblk, sg.reserved != 0, (b.reserved & 31) ? (b.reserved & 31) : 31);
}

extern "C" int vd_match_rows_fwd_multi(const VdMatchBatch* b, float* acc, void* stream) {
    if (b == nullptr || acc == nullptr || b->nseg < 0 || b->nseg > VD_MATCH_MAX_SEG) return -1;
    int64_t gx = 0;
    for (int i = 0; i < b->nseg; ++i) {
        if (b->seg[i].rows <= 0 || b->seg[i].len <= 0 || !b->seg[i].gr || !b->seg[i].gs) return -1;
        const int64_t nb = vd_match_blocks_fwd(b->seg[i].rows, b->seg[i].reserved ? 1 : (b->seg[i].len == 1 ? 2 : b->seg[i].len));
        gx = gx > nb ? gx : nb;
    }
    if (b->nseg == 0) return 0;
    hipLaunchKernelGGL(match_rows_fwd_multi_kernel, dim3((unsigned)gx, (unsigned)b->nseg), dim3(VD_MATCH_FWD_THREADS), 0,
                       reinterpret_cast<hipStream_t>(stream), *b, acc);
    return (int)hipGetLastError();
}

extern "C" int vd_match_rows_fwd(const float* gr, const float* gs, int64_t rows, int len, float* acc, void* stream) {
    if (rows <= 0 || len <= 0) return 0;
    const int64_t blocks = vd_match_blocks(rows, len == 1 ? 2 : len);      // len == 1: one-element cosine rows, not a flat sum
    hipLaunchKernelGGL(match_rows_fwd_kernel, dim3((unsigned)blocks), dim3(VD_MATCH_FWD_THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                       gr, gs, rows, len, acc);
    return (int)hipGetLastError();
}

// d/d gs.  mode 0: per-row cosine distance; with n=|r|, m=|s|, den=n*m+eps:
//   d(1 - <r,s>/den)/ds = -r/den + <r,s> * n * s / (m * den^2)
// mode 1: 2*(s-r).  mode 2: the same cosine formula with the GLOBAL sums acc[2..4].
__device__ __forceinline__ void match_rows_bwd_body(const float* __restrict__ gr, const float* __restrict__ gs,
                                                    int64_t rows, int len, int mode, const float* __restrict__ acc,
                                                    const float* __restrict__ gout, float* __restrict__ g, const int64_t nblk) {
    const float go = gout[0];
    if (mode == 1) {
        const int64_t n = rows * len;
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)nblk * blockDim.x)
            g[i] = go * 2.f * (gs[i] - gr[i]);
        return;
    }
    if (mode == 2) {
        const float d = acc[2], nr = sqrtf(acc[3]), ns = sqrtf(acc[4]);
        const float den = nr * ns + 0.000001f;
        const float c1 = -1.f / den, c2 = (ns > 0.f) ? d * nr / (ns * den * den) : 0.f;
        const int64_t n = rows * len;
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)nblk * blockDim.x)
            g[i] = go * (c1 * gr[i] + c2 * gs[i]);
        return;
    }
    if (len <= 8) {
        // rows staged through LDS; the gradient rows go back the same way: coalesced stores (up to 1024 blocks: one or two rounds,
        // nothing to prefetch)
        __shared__ VdMatchStage st;
        const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, ls = len | 1, magic = 65536 / len + 1;
        const int64_t rounds = match_short_rounds(rows, nblk);
        for (int64_t it = 0; it < rounds; ++it) {
            const int64_t r0 = match_short_row0(it, nblk);
            const int n = match_short_count(rows, len, r0);
            __syncthreads();                      // the previous round's reads are done
            for (int j = 0; j < len; ++j) {
                const int idx = j * 64 + lane;
                if (idx < n) {
                    const int row = (idx * magic) >> 16, k = idx - row * len;
                    st.r[w][row * ls + k] = gr[r0 * len + idx];
                    st.s[w][row * ls + k] = gs[r0 * len + idx];
                }
            }
            __syncthreads();
            if (r0 + lane < rows) {
                float d = 0.f, a = 0.f, b = 0.f;
                for (int k = 0; k < len; ++k) {
                    const float u = st.r[w][lane * ls + k], v = st.s[w][lane * ls + k];
                    d += u * v; a += u * u; b += v * v;
                }
                const float nr = sqrtf(a), ns = sqrtf(b), den = nr * ns + 0.000001f;
                const float c1 = -1.f / den, c2 = (ns > 0.f) ? d * nr / (ns * den * den) : 0.f;
                for (int k = 0; k < len; ++k) st.r[w][lane * ls + k] = go * (c1 * st.r[w][lane * ls + k] + c2 * st.s[w][lane * ls + k]);
            }
            __syncthreads();
            for (int j = 0; j < len; ++j) {
                const int idx = j * 64 + lane;
                if (idx < n) {
                    const int row = (idx * magic) >> 16, k = idx - row * len;
                    g[r0 * len + idx] = st.r[w][row * ls + k];
                }
            }
        }
    } else {
        const int lane = threadIdx.x & 63;
        const int64_t wid = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
        const int64_t nw = ((int64_t)nblk * blockDim.x) >> 6;
        for (int64_t r = wid; r < rows; r += nw) {
            float d = 0.f, a = 0.f, b = 0.f;
            for (int k = lane; k < len; k += 64) {
                const float x = gr[r * len + k], y = gs[r * len + k];
                d += x * y; a += x * x; b += y * y;
            }
            d = wave_sum(d); a = wave_sum(a); b = wave_sum(b);
            const float nr = sqrtf(a), ns = sqrtf(b), den = nr * ns + 0.000001f;
            const float c1 = -1.f / den, c2 = (ns > 0.f) ? d * nr / (ns * den * den) : 0.f;
            for (int k = lane; k < len; k += 64) g[r * len + k] = go * (c1 * gr[r * len + k] + c2 * gs[r * len + k]);
        }
    }
}

__global__ __launch_bounds__(256) void match_rows_bwd_kernel(const float* __restrict__ gr, const float* __restrict__ gs,
                                                              int64_t rows, int len, int mode, const float* __restrict__ acc,
                                                              const float* __restrict__ gout, float* __restrict__ g) {
    match_rows_bwd_body(gr, gs, rows, len, mode, acc, gout, g, gridDim.x);
}

__global__ __launch_bounds__(256) void match_rows_bwd_multi_kernel(const VdMatchBatch b, int mode, const float* __restrict__ acc,
                                                                    const float* __restrict__ gout) {
    const VdMatchSeg& sg = b.seg[blockIdx.y];
    const int64_t nblk = vd_match_blocks(sg.rows * (mode == 0 ? 1 : sg.len), mode == 0 ? (sg.len == 1 ? 2 : sg.len) : 1);
    if ((int64_t)blockIdx.x >= nblk) return;
    match_rows_bwd_body(sg.gr, sg.gs, sg.rows, sg.len, mode, acc, gout, sg.g, nblk);
}

extern "C" int vd_match_rows_bwd_multi(const VdMatchBatch* b, int mode, const float* acc, const float* gout, void* stream) {
    if (b == nullptr || acc == nullptr || gout == nullptr || b->nseg < 0 || b->nseg > VD_MATCH_MAX_SEG || mode < 0 || mode > 2) return -1;
    int64_t gx = 0;
    for (int i = 0; i < b->nseg; ++i) {
        if (b->seg[i].rows <= 0 || b->seg[i].len <= 0 || !b->seg[i].gr || !b->seg[i].gs || !b->seg[i].g) return -1;
        const int64_t nb = vd_match_blocks(b->seg[i].rows * (mode == 0 ? 1 : b->seg[i].len), mode == 0 ? (b->seg[i].len == 1 ? 2 : b->seg[i].len) : 1);
        gx = gx > nb ? gx : nb;
    }
    if (b->nseg == 0) return 0;
    hipLaunchKernelGGL(match_rows_bwd_multi_kernel, dim3((unsigned)gx, (unsigned)b->nseg), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), *b, mode, acc, gout);
    return (int)hipGetLastError();
}

extern "C" int vd_match_rows_bwd(const float* gr, const float* gs, int64_t rows, int len, int mode, const float* acc,
                                 const float* gout, float* g_gs, void* stream) {
    if (rows <= 0 || len <= 0) return 0;
    if (mode < 0 || mode > 2) return -2;
    int64_t blocks = (mode != 0 || len <= 8) ? (rows * (mode != 0 ? len : 1) + 255) / 256 : (rows + 3) / 4;
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(match_rows_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       gr, gs, rows, len, mode, acc, gout, g_gs);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// Classifier head of ConvNet3D.forward in eval mode (networks.py:738-745): AvgPool3d(k, stride 1)
// -> [dropout = identity] -> 1x1x1 conv -> squeeze -> max over T.  One workgroup per clip.
__global__ __launch_bounds__(256) void head_fwd_kernel(const float* __restrict__ feats, const float* __restrict__ w,
                                                        const float* __restrict__ b, int C, int To, int Ho, int Wo,
                                                        int kt, int kh, int kw, int K, float* __restrict__ out) {
    extern __shared__ float pooled[];          // [Tp][C]
    const int clip = blockIdx.x;
    const int Tp = To - kt + 1;
    const float* f = feats + (int64_t)clip * C * To * Ho * Wo;
    const float inv = 1.f / (float)(kt * kh * kw);
    for (int i = threadIdx.x; i < Tp * C; i += blockDim.x) {
        const int c = i % C, t = i / C;
        float a = 0.f;
        for (int dt = 0; dt < kt; ++dt)
            for (int dh = 0; dh < kh; ++dh)
                for (int dw = 0; dw < kw; ++dw) a += f[((c * To + t + dt) * Ho + dh) * Wo + dw];
        pooled[t * C + c] = a * inv;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < K; k += blockDim.x) {
        float best = -3.402823466e38f;
        for (int t = 0; t < Tp; ++t) {
            float a = b[k];
            for (int c = 0; c < C; ++c) a += w[k * C + c] * pooled[t * C + c];
            best = fmaxf(best, a);
        }
        out[(int64_t)clip * K + k] = best;
    }
}

extern "C" int vd_head_fwd(const float* feats, const float* w, const float* b, int64_t nclips, int C, int To, int Ho,
                           int Wo, int kt, int kh, int kw, int K, float* out, void* stream) {
    if (nclips <= 0) return 0;
    if (Ho - kh + 1 != 1 || Wo - kw + 1 != 1 || To - kt + 1 < 1) return -2;   // forward() squeezes H and W
    const size_t lds = (size_t)(To - kt + 1) * C * sizeof(float);
    hipLaunchKernelGGL(head_fwd_kernel, dim3((unsigned)nclips), dim3(256), lds, reinterpret_cast<hipStream_t>(stream),
                       feats, w, b, C, To, Ho, Wo, kt, kh, kw, K, out);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// Weight-gradient operand preparation (see plan.plan_wgrad).
// One thread per (channel chunk cc, clip chunk cb, position): loads the 8 clips' slots (8 channels
// each), transposes the 8x8 block of 16-bit values in registers, stores 8 slots (8 clips each).
__global__ void clip_minor_cl_kernel(const uint4* __restrict__ src, int64_t src_plane, int planes, int64_t nclips, int CCh,
                                     int64_t npos, uint4* __restrict__ dst, int64_t dst_plane, int CCb) {
    const int64_t total = (int64_t)CCh * CCb * npos;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int64_t pos = i % npos;
    const int cb = (int)((i / npos) % CCb);
    const int cc = (int)(i / (npos * CCb));
    for (int pl = 0; pl < planes; ++pl) {
        uint16_t m[8][8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int64_t clip = (int64_t)cb * 8 + j;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (clip < nclips) v = src[pl * src_plane + (clip * CCh + cc) * npos + pos];
            m[j][0] = v.x & 0xffff; m[j][1] = v.x >> 16; m[j][2] = v.y & 0xffff; m[j][3] = v.y >> 16;
            m[j][4] = v.z & 0xffff; m[j][5] = v.z >> 16; m[j][6] = v.w & 0xffff; m[j][7] = v.w >> 16;
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            uint4 o;
            o.x = m[0][k] | ((uint32_t)m[1][k] << 16); o.y = m[2][k] | ((uint32_t)m[3][k] << 16);
            o.z = m[4][k] | ((uint32_t)m[5][k] << 16); o.w = m[6][k] | ((uint32_t)m[7][k] << 16);
            dst[pl * dst_plane + (((int64_t)(cc * 8 + k)) * CCb + cb) * npos + pos] = o;
        }
    }
}

extern "C" int vd_clip_minor_cl(const void* src, int64_t src_plane_slots, int planes, int64_t nclips, int C, int64_t npos,
                                void* dst, int64_t dst_plane_slots, void* stream) {
    if (C % 8 != 0 || planes < 1 || planes > 2) return -2;
    const int CCb = (int)((nclips + 7) / 8);
    const int64_t total = (int64_t)(C / 8) * CCb * npos;
    if (total <= 0) return 0;
    hipLaunchKernelGGL(clip_minor_cl_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), (const uint4*)src, src_plane_slots, planes, nclips, C / 8, npos,
                       (uint4*)dst, dst_plane_slots, CCb);
    return (int)hipGetLastError();
}

__global__ void clip_minor_pix_kernel(const float* __restrict__ x, int64_t nclips, int T, int HW, uint4* __restrict__ hi,
                                      uint4* __restrict__ lo, int prec, int CCb) {
    const int64_t npos = (int64_t)T * HW;
    const int64_t total = (int64_t)3 * CCb * npos;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int64_t pos = i % npos;
    const int cb = (int)((i / npos) % CCb);
    const int c = (int)(i / (npos * CCb));
    const int64_t t = pos / HW, hw = pos % HW;
    uint16_t h16[8], l16[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int64_t clip = (int64_t)cb * 8 + j;
        const float v = (clip < nclips) ? x[((clip * T + t) * 3 + c) * HW + hw] : 0.f;
        split16p(prec, v, h16[j], l16[j]);
    }
    uint4 vh, vl;
    vh.x = h16[0] | ((uint32_t)h16[1] << 16); vh.y = h16[2] | ((uint32_t)h16[3] << 16);
    vh.z = h16[4] | ((uint32_t)h16[5] << 16); vh.w = h16[6] | ((uint32_t)h16[7] << 16);
    hi[i] = vh;
    if (lo != nullptr) {
        vl.x = l16[0] | ((uint32_t)l16[1] << 16); vl.y = l16[2] | ((uint32_t)l16[3] << 16);
        vl.z = l16[4] | ((uint32_t)l16[5] << 16); vl.w = l16[6] | ((uint32_t)l16[7] << 16);
        lo[i] = vl;
    }
}

extern "C" int vd_clip_minor_pix(const float* x, int64_t nclips, int T, int H, int W, void* dst_hi, void* dst_lo, int prec,
                                 void* stream) {
    const int CCb = (int)((nclips + 7) / 8);
    const int64_t total = (int64_t)3 * CCb * T * H * W;
    if (total <= 0) return 0;
    hipLaunchKernelGGL(clip_minor_pix_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), x, nclips, T, H * W, (uint4*)dst_hi, (uint4*)dst_lo, prec, CCb);
    return (int)hipGetLastError();
}

// one thread per packed B slot: (plane, box, cb, s, nt, lane) -> 8 clips of dy[pos][n]
__global__ void pack_dy_kernel(const uint16_t* __restrict__ dy, int64_t dy_plane_elems, int planes, int64_t nclips, int N,
                               int T, int OH, int OW, int nt, int noh, int now, int S, int CCb, int NT, int nbh, int nbw,
                               uint4* __restrict__ dst, int64_t dst_plane_slots, int64_t per_plane) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= per_plane * planes) return;
    const int pl = (int)(i / per_plane);
    int64_t r = i - (int64_t)pl * per_plane;
    const int lane = (int)(r & 63); r >>= 6;
    const int ntile = (int)(r % NT); r /= NT;
    const int s = (int)(r % S); r /= S;
    const int cb = (int)(r % CCb); r /= CCb;
    const int box = (int)r;
    const int bw = box % nbw, bh = (box / nbw) % nbh, bt = box / (nbw * nbh);
    const int pidx = 2 * s + (lane >> 5);
    const int dow = pidx % now, doh = (pidx / now) % noh, dt = pidx / (now * noh);
    const int t = bt * nt + dt, oh = bh * noh + doh, ow = bw * now + dow;
    const int n = ntile * 32 + (lane & 31);
    uint16_t v[8];
    const bool inside = (t < T) && (oh < OH) && (ow < OW);
    const int64_t npos = (int64_t)T * OH * OW;
    const int64_t pos = ((int64_t)t * OH + oh) * OW + ow;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int64_t clip = (int64_t)cb * 8 + j;
        v[j] = (inside && clip < nclips) ? dy[pl * dy_plane_elems + ((clip * (N >> 3) + (n >> 3)) * npos + pos) * 8 + (n & 7)] : (uint16_t)0;
    }
    uint4 o;
    o.x = v[0] | ((uint32_t)v[1] << 16); o.y = v[2] | ((uint32_t)v[3] << 16);
    o.z = v[4] | ((uint32_t)v[5] << 16); o.w = v[6] | ((uint32_t)v[7] << 16);
    dst[pl * dst_plane_slots + (i - (int64_t)pl * per_plane)] = o;
}

extern "C" int vd_pack_dy(const void* dy, int64_t dy_plane_slots, int planes, int64_t nclips, int N, int T, int OH, int OW,
                          int nt, int noh, int now, void* dst, int64_t dst_plane_elems, void* stream) {
    if (N % 32 != 0 || planes < 1 || planes > 2 || ((nt * noh * now) & 1)) return -2;
    const int S = nt * noh * now / 2, CCb = (int)((nclips + 7) / 8), NT = N / 32;
    const int nbt = (T + nt - 1) / nt, nbh = (OH + noh - 1) / noh, nbw = (OW + now - 1) / now;
    const int64_t per_plane = (int64_t)nbt * nbh * nbw * CCb * S * NT * 64;
    if (per_plane <= 0) return 0;
    const int64_t total = per_plane * planes;
    hipLaunchKernelGGL(pack_dy_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       (const uint16_t*)dy, dy_plane_slots * 8, planes, nclips, N, T, OH, OW, nt, noh, now, S, CCb, NT, nbh, nbw,
                       (uint4*)dst, dst_plane_elems / 8, per_plane);
    return (int)hipGetLastError();
}

// vd_unpool_relu_bwd + vd_pack_dy in one pass, for a layer whose dense dy nobody else reads (the first layer when no pixel
// gradient is asked for): one thread per packed B slot (box, cb, s, nt, lane) computes its 8 clips of dy[pos][n] straight
// from the pooled gradient and the arg-max bytes.  Same arithmetic, so the packed operand is bitwise the one the two
// kernels produce -- without writing and re-reading the dense slots (2 x 642 MB for 50 clips 112x112x16 in the hi+lo formats).
__global__ void unpool_pack_kernel(const float* __restrict__ g, const uint8_t* __restrict__ amax, int64_t nclips, int N,
                                   int To, int Ho, int Wo, int pool_t, int T, int OH, int OW, int g_layout,
                                   int nt, int noh, int now, int S, int CCb, int NT, int nbh, int nbw,
                                   uint4* __restrict__ hi, uint4* __restrict__ lo, int prec, const float* __restrict__ scale,
                                   int64_t per_plane) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= per_plane) return;
    const float sc = (scale != nullptr) ? scale[0] : 1.f;
    int64_t r = i;
    const int lane = (int)(r & 63); r >>= 6;
    const int ntile = (int)(r % NT); r /= NT;
    const int s = (int)(r % S); r /= S;
    const int cb = (int)(r % CCb); r /= CCb;
    const int box = (int)r;
    const int bw = box % nbw, bh = (box / nbw) % nbh, bt = box / (nbw * nbh);
    const int pidx = 2 * s + (lane >> 5);
    const int dow = pidx % now, doh = (pidx / now) % noh, dt = pidx / (now * noh);
    const int t = bt * nt + dt, oh = bh * noh + doh, ow = bw * now + dow;
    const int n = ntile * 32 + (lane & 31);
    const int pt = t / pool_t, pr = oh >> 1, pc = ow >> 1;
    const bool inside = (t < T) && (oh < OH) && (ow < OW) && (pt < To) && (pr < Ho) && (pc < Wo);
    const int j = (pool_t == 2 ? ((t & 1) << 2) : 0) | ((oh & 1) << 1) | (ow & 1);
    const int64_t npos = (int64_t)To * Ho * Wo;
    const int64_t pos = ((int64_t)pt * Ho + pr) * Wo + pc;
    const int CC = N >> 3, cc = n >> 3, e = n & 7;
    uint16_t h16[8], l16[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int64_t clip = (int64_t)cb * 8 + k;
        float v = 0.f;
        if (inside && clip < nclips) {
            int64_t gi, ai;
            if (g_layout == 0) { gi = (clip * N + n) * npos + pos; ai = gi; }
            else { gi = (clip * npos + pos) * N + n; ai = ((clip * CC + cc) * npos + pos) * 8 + e; }
            if (amax[ai] == (uint8_t)j) v = g[gi] * sc;
        }
        split16p(prec, v, h16[k], l16[k]);
    }
    uint4 vh, vl;
    vh.x = h16[0] | ((uint32_t)h16[1] << 16); vh.y = h16[2] | ((uint32_t)h16[3] << 16);
    vh.z = h16[4] | ((uint32_t)h16[5] << 16); vh.w = h16[6] | ((uint32_t)h16[7] << 16);
    hi[i] = vh;
    if (lo != nullptr) {
        vl.x = l16[0] | ((uint32_t)l16[1] << 16); vl.y = l16[2] | ((uint32_t)l16[3] << 16);
        vl.z = l16[4] | ((uint32_t)l16[5] << 16); vl.w = l16[6] | ((uint32_t)l16[7] << 16);
        lo[i] = vl;
    }
}

// The same for blocks with even height and width: one thread per 2x2 spatial pool window (box, cb, dt, doh/2, dow/2, nt, n%32)
// reads the 8 clips' pooled values and arg-max bytes ONCE and writes the window's four slots (4x fewer load instructions;
// the four stores of a wave's 32 channels are 512 contiguous bytes each).
__global__ void unpool_pack_win_kernel(const float* __restrict__ g, const uint8_t* __restrict__ amax, int64_t nclips, int N,
                                       int To, int Ho, int Wo, int pool_t, int T, int OH, int OW, int g_layout,
                                       int nt, int noh, int now, int S, int CCb, int NT, int nbh, int nbw,
                                       uint4* __restrict__ hi, uint4* __restrict__ lo, int prec, const float* __restrict__ scale,
                                       int64_t nthreads) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nthreads) return;
    const float sc = (scale != nullptr) ? scale[0] : 1.f;
    const int hw = now >> 1, hh = noh >> 1;
    int64_t r = i;
    const int l32 = (int)(r & 31); r >>= 5;
    const int ntile = (int)(r % NT); r /= NT;
    const int wc = (int)(r % hw); r /= hw;
    const int wr = (int)(r % hh); r /= hh;
    const int dt = (int)(r % nt); r /= nt;
    const int cb = (int)(r % CCb); r /= CCb;
    const int box = (int)r;
    const int bw = box % nbw, bh = (box / nbw) % nbh, bt = box / (nbw * nbh);
    const int t = bt * nt + dt, oh0 = bh * noh + 2 * wr, ow0 = bw * now + 2 * wc;
    const int n = ntile * 32 + l32;
    const int pt = t / pool_t, pr = oh0 >> 1, pc = ow0 >> 1;
    const bool live = (t < T) && (pt < To) && (pr < Ho) && (pc < Wo);
    const int jt = (pool_t == 2) ? ((t & 1) << 2) : 0;
    const int64_t npos = (int64_t)To * Ho * Wo;
    const int64_t pos = ((int64_t)pt * Ho + pr) * Wo + pc;
    const int CC = N >> 3, cc = n >> 3, e = n & 7;
    float gv[8];
    int code[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int64_t clip = (int64_t)cb * 8 + k;
        gv[k] = 0.f; code[k] = -1;
        if (live && clip < nclips) {
            int64_t gi, ai;
            if (g_layout == 0) { gi = (clip * N + n) * npos + pos; ai = gi; }
            else { gi = (clip * npos + pos) * N + n; ai = ((clip * CC + cc) * npos + pos) * 8 + e; }
            code[k] = (int)amax[ai];
            gv[k] = g[gi] * sc;
        }
    }
    const int64_t box_base = ((int64_t)box * CCb + cb) * S;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int dr = q >> 1, dc = q & 1;
        const int pidx = (dt * noh + 2 * wr + dr) * now + 2 * wc + dc;
        const bool inside = (oh0 + dr < OH) && (ow0 + dc < OW);
        const int j = jt | (dr << 1) | dc;
        uint16_t h16[8], l16[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) split16p(prec, (inside && code[k] == j) ? gv[k] : 0.f, h16[k], l16[k]);
        const int64_t o = ((box_base + (pidx >> 1)) * NT + ntile) * 64 + (pidx & 1) * 32 + l32;
        uint4 vh, vl;
        vh.x = h16[0] | ((uint32_t)h16[1] << 16); vh.y = h16[2] | ((uint32_t)h16[3] << 16);
        vh.z = h16[4] | ((uint32_t)h16[5] << 16); vh.w = h16[6] | ((uint32_t)h16[7] << 16);
        hi[o] = vh;
        if (lo != nullptr) {
            vl.x = l16[0] | ((uint32_t)l16[1] << 16); vl.y = l16[2] | ((uint32_t)l16[3] << 16);
            vl.z = l16[4] | ((uint32_t)l16[5] << 16); vl.w = l16[6] | ((uint32_t)l16[7] << 16);
            lo[o] = vl;
        }
    }
}

extern "C" int vd_unpool_relu_bwd_packed(const float* g, const uint8_t* argmax, int64_t nclips, int C, int To, int Ho, int Wo,
                                         int pool_t, int T, int OH, int OW, int g_layout, int nt, int noh, int now,
                                         void* dst_hi, void* dst_lo, int prec, const float* scale, void* stream) {
    if (C % 32 != 0 || (pool_t != 1 && pool_t != 2) || ((nt * noh * now) & 1) || nt < 1 || noh < 1 || now < 1) return -2;
    const int S = nt * noh * now / 2, CCb = (int)((nclips + 7) / 8), NT = C / 32;
    const int nbt = (T + nt - 1) / nt, nbh = (OH + noh - 1) / noh, nbw = (OW + now - 1) / now;
    const int64_t per_plane = (int64_t)nbt * nbh * nbw * CCb * S * NT * 64;
    if (per_plane <= 0) return 0;
    if (!g || !argmax || !dst_hi) return -1;
    if ((noh & 1) == 0 && (now & 1) == 0) {
        const int64_t nthreads = per_plane / 4;          // four slots per thread
        hipLaunchKernelGGL(unpool_pack_win_kernel, dim3((unsigned)((nthreads + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                           g, argmax, nclips, C, To, Ho, Wo, pool_t, T, OH, OW, g_layout, nt, noh, now, S, CCb, NT, nbh, nbw,
                           (uint4*)dst_hi, (uint4*)dst_lo, prec, scale, nthreads);
        return (int)hipGetLastError();
    }
    hipLaunchKernelGGL(unpool_pack_kernel, dim3((unsigned)((per_plane + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       g, argmax, nclips, C, To, Ho, Wo, pool_t, T, OH, OW, g_layout, nt, noh, now, S, CCb, NT, nbh, nbw,
                       (uint4*)dst_hi, (uint4*)dst_lo, prec, scale, per_plane);
    return (int)hipGetLastError();
}

// Conv3d bias gradient: one workgroup per 8-channel chunk; threads stride (clip, position).
__global__ __launch_bounds__(256) void bias_grad_kernel(const uint4* __restrict__ dy, int64_t plane_slots, int planes,
                                                         int64_t nclips, int CCh, int64_t npos, int prec,
                                                         const float* __restrict__ scale_inv, float* __restrict__ db) {
    // grid (N/8, clips, position blocks): every workgroup reduces a contiguous run of slots of one
    // (clip, channel chunk) and adds its 8 partial sums with fp32 atomics.
    __shared__ float red[16];
    const int cc = blockIdx.x;
    const int64_t clip = blockIdx.y;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const bool bf = (prec == VD_PREC_BF16 || prec == VD_PREC_BF16X3);
    for (int pl = 0; pl < planes; ++pl) {
        const uint4* base = dy + pl * plane_slots + (clip * CCh + cc) * npos;
        for (int64_t pos = (int64_t)blockIdx.z * blockDim.x + threadIdx.x; pos < npos; pos += (int64_t)gridDim.z * blockDim.x) {
            const uint4 v = base[pos];
            const uint32_t wds[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const uint16_t hbits = (uint16_t)(wds[k >> 1] >> ((k & 1) * 16));
                acc[k] += bf ? __uint_as_float((uint32_t)hbits << 16) : (float)__builtin_bit_cast(_Float16, hbits);
            }
        }
    }
    const float sc = scale_inv ? scale_inv[0] : 1.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float tot = block_sum(acc[k], red);
        if (threadIdx.x == 0) atomicAdd(&db[cc * 8 + k], tot * sc);
    }
}

extern "C" int vd_bias_grad(const void* dy, int64_t dy_plane_slots, int planes, int64_t nclips, int N, int64_t npos, int prec,
                            const float* scale_inv, float* db, void* stream) {
    if (N % 8 != 0 || nclips > 65535) return -2;
    if (nclips <= 0) return 0;
    int zb = (int)((npos + 256 * 8 - 1) / (256 * 8));
    if (zb > 64) zb = 64;
    hipLaunchKernelGGL(bias_grad_kernel, dim3(N / 8, (unsigned)nclips, zb), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       (const uint4*)dy, dy_plane_slots, planes, nclips, N / 8, npos, prec, scale_inv, db);
    return (int)hipGetLastError();
}

// Bias gradient straight from the POOLED gradient: the dense dy has one non-zero per pool window -- the pooled
// value, if the window was alive -- so db[n] = sum over clips and pooled positions of g where bit 7 of the arg-max
// byte is clear.  Reads 4-8x fewer bytes than summing the dense dy slots (vd_bias_grad).
__global__ __launch_bounds__(256) void bias_grad_pooled_kernel(const float* __restrict__ g, const uint8_t* __restrict__ amax,
                                                                int C, int64_t npos, int g_layout, int pos_per_block,
                                                                float* __restrict__ db, int partial) {
    __shared__ float red[256];
    const int64_t clip = blockIdx.x;
    const int n = threadIdx.x % C, pl = threadIdx.x / C, npl = 256 / C;
    const int64_t p0 = (int64_t)blockIdx.y * pos_per_block;
    const int64_t p1 = (p0 + pos_per_block < npos) ? p0 + pos_per_block : npos;
    const int CC = C >> 3;
    float acc = 0.f;
    for (int64_t pos = p0 + pl; pos < p1; pos += npl) {
        int64_t gi, ai;
        if (g_layout == 0) { gi = (clip * C + n) * npos + pos; ai = gi; }
        else { gi = (clip * npos + pos) * C + n; ai = ((clip * CC + (n >> 3)) * npos + pos) * 8 + (n & 7); }
        if (!(amax[ai] & 0x80)) acc += g[gi];
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    if (pl == 0) {
        for (int k = 1; k < npl; ++k) acc += red[k * C + n];
        if (partial) db[((int64_t)clip * gridDim.y + blockIdx.y) * C + n] = acc;     // ordered mode: one slot per workgroup, folded below
        else atomicAdd(&db[n], acc);
    }
}

// Ordered mode (vd_*_ordered, DESIGN 8b "deterministic training step"): the workgroups' partial sums, one row of C floats per
// (clip, position block), are folded in index order by ONE thread per channel -- a fixed summation order, so the result is
// bitwise reproducible where the atomic form's last bits depend on the order the workgroups retire in.
__global__ __launch_bounds__(1024) void fold_rows_kernel(const float* __restrict__ part, int64_t nrows, int C, float* __restrict__ out) {
    // 32 row lanes x 32 channels per workgroup: lane l adds rows l, l + 32, ... in index order, then ONE thread per channel adds
    // the 32 lane sums in lane order -- the same association in every run (a single thread walking 1250 rows took 0.2 ms)
    __shared__ float lanes[32][33];
    const int n = blockIdx.x * 32 + (threadIdx.x & 31), l = threadIdx.x >> 5;
    float acc = 0.f;
    if (n < C)
        for (int64_t r = l; r < nrows; r += 32) acc += part[r * C + n];
    lanes[l][threadIdx.x & 31] = acc;
    __syncthreads();
    if (l == 0 && n < C) {
        float tot = 0.f;
#pragma unroll
        for (int k = 0; k < 32; ++k) tot += lanes[k][threadIdx.x & 31];
        out[n] += tot;
    }
}

extern "C" int vd_bias_grad_pooled(const float* g, const uint8_t* argmax, int64_t nclips, int C, int64_t npos, int g_layout,
                                   float* db, void* stream) {
    if (C <= 0 || C > 256 || 256 % C != 0 || C % 8 != 0 || nclips > 0x7fffffff) return -2;
    if (nclips <= 0 || npos <= 0) return 0;
    const int ppb = 256;
    const unsigned gy = (unsigned)((npos + ppb - 1) / ppb);
    hipLaunchKernelGGL(bias_grad_pooled_kernel, dim3((unsigned)nclips, gy), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), g,
                       argmax, C, npos, g_layout, ppb, db, 0);
    return (int)hipGetLastError();
}

extern "C" int64_t vd_bias_grad_pooled_scratch_floats(int64_t nclips, int C, int64_t npos) {
    if (nclips <= 0 || npos <= 0 || C <= 0) return 0;
    return nclips * ((npos + 255) / 256) * C;
}

// vd_bias_grad_pooled with a FIXED summation order: partial sums per (clip, block of 256 positions) into `scratch`
// (vd_bias_grad_pooled_scratch_floats floats, caller-owned), then folded in index order and added to db.
extern "C" int vd_bias_grad_pooled_ordered(const float* g, const uint8_t* argmax, int64_t nclips, int C, int64_t npos, int g_layout,
                                           float* scratch, float* db, void* stream) {
    if (C <= 0 || C > 256 || 256 % C != 0 || C % 8 != 0 || nclips > 0x7fffffff) return -2;
    if (nclips <= 0 || npos <= 0) return 0;
    if (scratch == nullptr || db == nullptr) return -1;
    const int ppb = 256;
    const unsigned gy = (unsigned)((npos + ppb - 1) / ppb);
    hipLaunchKernelGGL(bias_grad_pooled_kernel, dim3((unsigned)nclips, gy), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), g,
                       argmax, C, npos, g_layout, ppb, scratch, 1);
    hipLaunchKernelGGL(fold_rows_kernel, dim3((unsigned)((C + 31) / 32)), dim3(1024), 0, reinterpret_cast<hipStream_t>(stream), scratch,
                       nclips * (int64_t)gy, C, db);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// Training half of the classifier head + loss + optimiser (evaluate_synset / epoch('train'),
// reference utils.py:765-792, 852): one workgroup per clip, everything per clip fits LDS.
//   pooled[t'][c] = mean over the (kt,kh,kw) window of feats;  dropped = pooled * mask (mask already
//   holds 0 or 1/(1-p));  z[t'][k] = b[k] + sum_c w[k][c] * dropped[t'][c];  logits[k] = max_t' z.
__global__ __launch_bounds__(256) void head_train_fwd_kernel(const float* __restrict__ feats, const float* __restrict__ mask,
                                                              const float* __restrict__ w, const float* __restrict__ b,
                                                              int C, int To, int Ho, int Wo, int kt, int kh, int kw, int K,
                                                              float* __restrict__ dropped_out, float* __restrict__ logits,
                                                              int32_t* __restrict__ amax_t) {
    extern __shared__ float pooled[];          // [Tp][C]
    const int clip = blockIdx.x;
    const int Tp = To - kt + 1;
    const float* f = feats + (int64_t)clip * C * To * Ho * Wo;
    const float inv = 1.f / (float)(kt * kh * kw);
    for (int i = threadIdx.x; i < Tp * C; i += blockDim.x) {
        const int c = i % C, t = i / C;
        float a = 0.f;
        for (int dt = 0; dt < kt; ++dt)
            for (int dh = 0; dh < kh; ++dh)
                for (int dw = 0; dw < kw; ++dw) a += f[((c * To + t + dt) * Ho + dh) * Wo + dw];
        a *= inv;
        if (mask != nullptr) a *= mask[((int64_t)clip * C + c) * Tp + t];     // mask layout (B, C, Tp) like the pooled tensor
        pooled[t * C + c] = a;
        dropped_out[((int64_t)clip * Tp + t) * C + c] = a;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < K; k += blockDim.x) {
        float best = -3.402823466e38f;
        int bt = 0;
        for (int t = 0; t < Tp; ++t) {
            float a = b[k];
            for (int c = 0; c < C; ++c) a += w[k * C + c] * pooled[t * C + c];
            if (a > best) { best = a; bt = t; }
        }
        logits[(int64_t)clip * K + k] = best;
        amax_t[(int64_t)clip * K + k] = bt;
    }
}

extern "C" int vd_head_train_fwd(const float* feats, const float* mask, const float* w, const float* b, int64_t nclips, int C,
                                 int To, int Ho, int Wo, int kt, int kh, int kw, int K, float* dropped, float* logits,
                                 int32_t* amax_t, void* stream) {
    if (nclips <= 0) return 0;
    if (Ho - kh + 1 != 1 || Wo - kw + 1 != 1 || To - kt + 1 < 1) return -2;
    const size_t lds = (size_t)(To - kt + 1) * C * sizeof(float);
    hipLaunchKernelGGL(head_train_fwd_kernel, dim3((unsigned)nclips), dim3(256), lds, reinterpret_cast<hipStream_t>(stream),
                       feats, mask, w, b, C, To, Ho, Wo, kt, kh, kw, K, dropped, logits, amax_t);
    return (int)hipGetLastError();
}

// Mean cross-entropy over the batch and its gradient w.r.t. the logits: one workgroup per clip.
__global__ __launch_bounds__(64) void ce_loss_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels, int B,
                                                      int K, float* __restrict__ loss_per_clip, float* __restrict__ dlogits) {
    const int clip = blockIdx.x, lane = threadIdx.x;
    const float* z = logits + (int64_t)clip * K;
    float m = -3.402823466e38f;
    for (int k = lane; k < K; k += 64) m = fmaxf(m, z[k]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    // The softmax in fp64, rounded once (round 6).  The fast intrinsics this kernel used (__expf / __logf: hardware exp2 / log2 with an
    // fp32 argument scaling) leave ~4e-7 on log-sum-exp -- one common relative factor on all K probabilities of a clip, so they no
    // longer sum to one -- where torch's fp32 log_softmax (what F.cross_entropy of distill_baseline.py:249 runs) is exact to 6e-8;
    // over the ten unrolled student steps of MTT that was the 3 - 14x by which the HIP gradients stood further from the exact
    // ones than fp32 arithmetic (tools/mtt_dissect.py).  K <= a few hundred values per clip: the cost is nothing.
    double sum = 0.0;
    for (int k = lane; k < K; k += 64) sum += exp((double)z[k] - (double)m);
    sum = wave_sum_d(sum);
    const int64_t yl = labels[clip];
    const double lse = (double)m + log(sum);
    if (yl < 0 || yl >= K) {
        // a label outside [0, K): torch raises; without a host sync the loud failure is a NaN loss and gradient
        const float nan = __uint_as_float(0x7fc00000u);
        if (lane == 0) loss_per_clip[clip] = nan;
        for (int k = lane; k < K; k += 64) dlogits[(int64_t)clip * K + k] = nan;
        return;
    }
    const int y = (int)yl;
    if (lane == 0) loss_per_clip[clip] = (float)(lse - (double)z[y]);
    const double invB = 1.0 / (double)B;
    for (int k = lane; k < K; k += 64)
        dlogits[(int64_t)clip * K + k] = (float)((exp((double)z[k] - lse) - (k == y ? 1.0 : 0.0)) * invB);
}

extern "C" int vd_ce_loss(const float* logits, const int64_t* labels, int B, int K, float* loss_per_clip, float* dlogits,
                          void* stream) {
    if (B <= 0) return 0;
    hipLaunchKernelGGL(ce_loss_kernel, dim3(B), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), logits, labels, B, K,
                       loss_per_clip, dlogits);
    return (int)hipGetLastError();
}

// Backward of the head: dlogits (B,K) routed to the arg-max frame; gradients of the 1x1x1 conv
// (atomics into g_w [K][C], g_b [K]) and of the features (B,C,To,Ho,Wo) through dropout and avg-pool.
__global__ __launch_bounds__(256) void head_train_bwd_kernel(const float* __restrict__ dlogits, const int32_t* __restrict__ amax_t,
                                                              const float* __restrict__ dropped, const float* __restrict__ mask,
                                                              const float* __restrict__ w, int C, int To, int Ho, int Wo, int kt,
                                                              int kh, int kw, int K, float* __restrict__ g_w,
                                                              float* __restrict__ g_b, float* __restrict__ g_feats) {
    extern __shared__ float dp[];              // [Tp][C] gradient w.r.t. the dropped/pooled tensor
    const int clip = blockIdx.x;
    const int Tp = To - kt + 1;
    const float* dl = dlogits + (int64_t)clip * K;
    const int32_t* am = amax_t + (int64_t)clip * K;
    for (int i = threadIdx.x; i < Tp * C; i += blockDim.x) {
        const int c = i % C, t = i / C;
        float a = 0.f;
        for (int k = 0; k < K; ++k) if (am[k] == t) a += dl[k] * w[k * C + c];
        if (mask != nullptr) a *= mask[((int64_t)clip * C + c) * Tp + t];
        dp[t * C + c] = a;
    }
    if (g_w != nullptr) {               // (NULL in the ordered mode: head_param_grad_ordered_kernel computes both)
        for (int i = threadIdx.x; i < K * C; i += blockDim.x) {
            const int c = i % C, k = i / C;
            atomicAdd(&g_w[i], dl[k] * dropped[((int64_t)clip * Tp + am[k]) * C + c]);
        }
        for (int k = threadIdx.x; k < K; k += blockDim.x) atomicAdd(&g_b[k], dl[k]);
    }
    __syncthreads();
    const float inv = 1.f / (float)(kt * kh * kw);
    float* gf = g_feats + (int64_t)clip * C * To * Ho * Wo;
    for (int i = threadIdx.x; i < C * To * Ho * Wo; i += blockDim.x) {
        const int x = i % Wo, y = (i / Wo) % Ho, t = (i / (Wo * Ho)) % To, c = i / (Wo * Ho * To);
        // windows (stride 1) containing (t,y,x): t' in [t-kt+1, t], and the single h'/w' window covers all y,x
        float a = 0.f;
        for (int tp = t - kt + 1; tp <= t; ++tp) if (tp >= 0 && tp < Tp) a += dp[tp * C + c];
        (void)x; (void)y;
        gf[i] = a * inv;
    }
}

// Ordered mode of the logit conv's parameter gradients: a gather instead of a scatter -- one thread per (class k, channel c)
// walks the clips in index order,  g_w[k][c] += sum_clip dl[clip][k] * dropped[clip][amax_t[clip][k]][c];  threads with c == C
// do the bias,  g_b[k] += sum_clip dl[clip][k].  No atomics, fixed order: bitwise reproducible.
__global__ __launch_bounds__(256) void head_param_grad_ordered_kernel(const float* __restrict__ dlogits, const int32_t* __restrict__ amax_t,
                                                                       const float* __restrict__ dropped, int64_t nclips, int C, int Tp,
                                                                       int K, float* __restrict__ g_w, float* __restrict__ g_b) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)K * (C + 1)) return;
    const int k = (int)(i / (C + 1)), c = (int)(i % (C + 1));
    float acc = 0.f;
    if (c == C) {
        for (int64_t clip = 0; clip < nclips; ++clip) acc += dlogits[clip * K + k];
        g_b[k] += acc;
    } else {
        for (int64_t clip = 0; clip < nclips; ++clip)
            acc += dlogits[clip * K + k] * dropped[(clip * Tp + amax_t[clip * K + k]) * C + c];
        g_w[(int64_t)k * C + c] += acc;
    }
}

// vd_head_train_bwd with the parameter gradients summed over the clips in a fixed order (no atomics); same arguments.
extern "C" int vd_head_train_bwd_ordered(const float* dlogits, const int32_t* amax_t, const float* dropped, const float* mask,
                                         const float* w, int64_t nclips, int C, int To, int Ho, int Wo, int kt, int kh, int kw, int K,
                                         float* g_w, float* g_b, float* g_feats, void* stream) {
    if (nclips <= 0) return 0;
    if (Ho - kh + 1 != 1 || Wo - kw + 1 != 1 || To - kt + 1 < 1) return -2;
    if (g_w == nullptr || g_b == nullptr) return -1;
    const int Tp = To - kt + 1;
    const size_t lds = (size_t)Tp * C * sizeof(float);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(head_train_bwd_kernel, dim3((unsigned)nclips), dim3(256), lds, st, dlogits, amax_t, dropped, mask, w, C, To, Ho,
                       Wo, kt, kh, kw, K, (float*)nullptr, (float*)nullptr, g_feats);
    const int64_t n = (int64_t)K * (C + 1);
    hipLaunchKernelGGL(head_param_grad_ordered_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, dlogits, amax_t, dropped,
                       nclips, C, Tp, K, g_w, g_b);
    return (int)hipGetLastError();
}

extern "C" int vd_head_train_bwd(const float* dlogits, const int32_t* amax_t, const float* dropped, const float* mask,
                                 const float* w, int64_t nclips, int C, int To, int Ho, int Wo, int kt, int kh, int kw, int K,
                                 float* g_w, float* g_b, float* g_feats, void* stream) {
    if (nclips <= 0) return 0;
    if (Ho - kh + 1 != 1 || Wo - kw + 1 != 1 || To - kt + 1 < 1) return -2;
    const size_t lds = (size_t)(To - kt + 1) * C * sizeof(float);
    hipLaunchKernelGGL(head_train_bwd_kernel, dim3((unsigned)nclips), dim3(256), lds, reinterpret_cast<hipStream_t>(stream),
                       dlogits, amax_t, dropped, mask, w, C, To, Ho, Wo, kt, kh, kw, K, g_w, g_b, g_feats);
    return (int)hipGetLastError();
}

// Re-split 16-bit operand slots from one hi/lo format to another (f16 pairs <-> bf16 pairs): the
// gradient-matching engine takes its pooling decisions from an f16x3 forward (rounding error like
// fp32's) and runs the adjoint sweeps on bf16 pairs (fp32's exponent range).
__global__ void resplit_kernel(const uint16_t* __restrict__ shi, const uint16_t* __restrict__ slo, int64_t n, int sprec,
                               uint16_t* __restrict__ dhi, uint16_t* __restrict__ dlo, int dprec) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const bool sbf = (sprec == VD_PREC_BF16 || sprec == VD_PREC_BF16X3);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        float v = sbf ? __uint_as_float((uint32_t)shi[i] << 16) : (float)__builtin_bit_cast(_Float16, shi[i]);
        if (slo != nullptr) v += sbf ? __uint_as_float((uint32_t)slo[i] << 16) : (float)__builtin_bit_cast(_Float16, slo[i]);
        uint16_t hi, lo;
        split16p(dprec, v, hi, lo);
        dhi[i] = hi;
        if (dlo != nullptr) dlo[i] = lo;
    }
}

extern "C" int vd_resplit_slots(const void* src_hi, const void* src_lo, int64_t n_elems, int src_prec, void* dst_hi, void* dst_lo,
                                int dst_prec, void* stream) {
    if (n_elems <= 0) return 0;
    int64_t blocks = (n_elems + 255) / 256;
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL(resplit_kernel, dim3((unsigned)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       (const uint16_t*)src_hi, (const uint16_t*)src_lo, n_elems, src_prec, (uint16_t*)dst_hi, (uint16_t*)dst_lo,
                       dst_prec);
    return (int)hipGetLastError();
}

// fp32 -> (scaled) 16-bit operand elements, same order: the fp32 tangents a select = 2 program wrote become the source slots
// of the next level once their range is known (vd_absmax_scale).  16 bytes in, 8 (+ 8) bytes out per thread and round.
__global__ void split_scaled_kernel(const float4* __restrict__ src, int64_t n4, const float* __restrict__ scale,
                                    uint2* __restrict__ dhi, uint2* __restrict__ dlo, int prec) {
    const float sc = (scale != nullptr) ? scale[0] : 1.f;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        const float4 v = src[i];
        uint16_t h[4], l[4];
        split16p(prec, v.x * sc, h[0], l[0]); split16p(prec, v.y * sc, h[1], l[1]);
        split16p(prec, v.z * sc, h[2], l[2]); split16p(prec, v.w * sc, h[3], l[3]);
        dhi[i] = make_uint2(h[0] | ((uint32_t)h[1] << 16), h[2] | ((uint32_t)h[3] << 16));
        if (dlo != nullptr) dlo[i] = make_uint2(l[0] | ((uint32_t)l[1] << 16), l[2] | ((uint32_t)l[3] << 16));
    }
}

extern "C" int vd_split_scaled(const float* src, int64_t n_elems, const float* scale, void* dst_hi, void* dst_lo, int prec, void* stream) {
    if (n_elems <= 0) return 0;
    if (src == nullptr || dst_hi == nullptr || (n_elems & 3) != 0 || prec < 0 || prec > 3) return -2;
    if (((reinterpret_cast<uintptr_t>(src) & 15) | (reinterpret_cast<uintptr_t>(dst_hi) & 7) | (reinterpret_cast<uintptr_t>(dst_lo) & 7)) != 0) return -2;
    const int64_t n4 = n_elems >> 2;
    int64_t blocks = (n4 + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(split_scaled_kernel, dim3((unsigned)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       (const float4*)src, n4, scale, (uint2*)dst_hi, (uint2*)dst_lo, prec);
    return (int)hipGetLastError();
}

__global__ void scale_combine_kernel(const float* __restrict__ a, const float* __restrict__ b, int mode, float* __restrict__ out) {
    const float x = a[0], y = (b != nullptr) ? b[0] : 1.f;
    float s = x * y;
    if (mode == 1) {      // common scale of two tensors: the smaller one -- but an all-zero tensor (absmax word 0) constrains nothing
        const bool a_empty = (a[2] == 0.f), b_empty = (b == nullptr) || (b[2] == 0.f);
        s = a_empty ? (b_empty ? 1.f : y) : (b_empty ? x : fminf(x, y));
    }
    out[0] = s;
    out[1] = 1.f / s;
}

extern "C" int vd_scale_combine(const float* a, const float* b, int mode, float* out, void* stream) {
    if (a == nullptr || out == nullptr || (mode != 0 && mode != 1)) return -2;
    hipLaunchKernelGGL(scale_combine_kernel, dim3(1), dim3(1), 0, reinterpret_cast<hipStream_t>(stream), a, b, mode, out);
    return (int)hipGetLastError();
}

// Second-order pass through the head (gradient matching, d match_loss / d pixels): given the
// adjoints of the head's parameter gradients (v_w [K][C], v_b [K]) and of the feature gradient
// (gbar_feats, (B,C,To,Ho,Wo)), produce the adjoint of the features.  With p = softmax(logits),
// dlog = (p - onehot)/B, t*_k the arg-max frame of class k:
//   dlogbar[k]  = sum_c w[k][c] * m*avgpool(gbar_feats)[t*_k][c] + sum_c v_w[k][c] * dropped[t*_k][c] + v_b[k]
//   logitbar[k] = p[k] * (dlogbar[k] - <p, dlogbar>) / B                       (Hessian of the mean CE)
//   dropbar[t][c] = sum_{k: t*_k = t} (w[k][c] * logitbar[k] + v_w[k][c] * dlog[k])
//   abar_feats = avgpool^T (m * dropbar)
__global__ __launch_bounds__(256) void head_second_order_kernel(
    const float* __restrict__ logits, const float* __restrict__ dlogits, const int32_t* __restrict__ amax_t,
    const float* __restrict__ dropped, const float* __restrict__ mask, const float* __restrict__ w,
    const float* __restrict__ v_w, const float* __restrict__ v_b, const float* __restrict__ gbar_feats, int B, int C, int To,
    int Ho, int Wo, int kt, int kh, int kw, int K, float* __restrict__ abar_feats, float* __restrict__ wbar,
    float* __restrict__ bbar, float* __restrict__ dlogbar_out) {
    extern __shared__ float sm[];
    const int Tp = To - kt + 1;
    float* u = sm;                   // [Tp][C]  m * avgpool(gbar_feats), later m * dropbar
    float* dlb = sm + Tp * C;        // [K] dlogbar, then logitbar
    float* pk = dlb + K;             // [K] softmax
    __shared__ float red[16];
    const int clip = blockIdx.x;
    const float inv = 1.f / (float)(kt * kh * kw);
    const float* gb = gbar_feats + (int64_t)clip * C * To * Ho * Wo;
    for (int i = threadIdx.x; i < Tp * C; i += blockDim.x) {
        const int c = i % C, t = i / C;
        float a = 0.f;
        for (int dt = 0; dt < kt; ++dt)
            for (int dh = 0; dh < kh; ++dh)
                for (int dw = 0; dw < kw; ++dw) a += gb[((c * To + t + dt) * Ho + dh) * Wo + dw];
        a *= inv;
        if (mask != nullptr) a *= mask[((int64_t)clip * C + c) * Tp + t];
        u[i] = a;
    }
    // logits == nullptr: no loss Hessian (the caller differentiates its own loss; autograd path of ConvNet3D.forward):
    // dlogbar is handed out through dlogbar_out and logitbar = 0.
    const bool hess = (logits != nullptr);
    const float* z = hess ? logits + (int64_t)clip * K : nullptr;
    float m = -3.402823466e38f;
    double ssum = 1.0;              // (softmax and the Hessian's <p, dlogbar> in fp64: see ce_loss_kernel)
    if (hess) {
        for (int k = 0; k < K; ++k) m = fmaxf(m, z[k]);
        ssum = 0.0;
        for (int k = 0; k < K; ++k) ssum += exp((double)z[k] - (double)m);
    }
    __syncthreads();
    const int32_t* am = amax_t + (int64_t)clip * K;
    const float* dl = dlogits + (int64_t)clip * K;
    double part = 0.0;
    for (int k = threadIdx.x; k < K; k += blockDim.x) {
        const int t = am[k];
        const float* dr = dropped + ((int64_t)clip * Tp + t) * C;
        float a = v_b[k];
        for (int c = 0; c < C; ++c) a += w[k * C + c] * u[t * C + c] + v_w[k * C + c] * dr[c];
        const double pd = hess ? exp((double)z[k] - (double)m) / ssum : 0.0;
        dlb[k] = a;
        pk[k] = (float)pd;
        part += pd * (double)a;
        if (dlogbar_out != nullptr) dlogbar_out[(int64_t)clip * K + k] = a;
    }
    __shared__ double dot_s;
    __shared__ double red_d[16];
    part = wave_sum_d(part);
    if ((threadIdx.x & 63) == 0) red_d[threadIdx.x >> 6] = part;
    __syncthreads();
    if (threadIdx.x == 0) {
        double tsum = 0.0;
        for (int i = 0; i < (int)((blockDim.x + 63) >> 6); ++i) tsum += red_d[i];
        dot_s = tsum;
    }
    __syncthreads();
    const double dot = dot_s;
    for (int k = threadIdx.x; k < K; k += blockDim.x)
        dlb[k] = hess ? (float)((double)pk[k] * ((double)dlb[k] - dot) / (double)B) : 0.f;
    __syncthreads();
    if (wbar != nullptr) {
        // adjoint of the logit conv's own parameters (Hessian-vector product for MTT):
        //   wbar[k][c] += dlog[k] * (m*avgpool(gbar))[t*_k][c] + logitbar[k] * dropped[t*_k][c];  bbar[k] += logitbar[k]
        for (int i = threadIdx.x; i < K * C; i += blockDim.x) {
            const int c = i % C, k = i / C;
            const int t = am[k];
            atomicAdd(&wbar[i], dl[k] * u[t * C + c] + dlb[k] * dropped[((int64_t)clip * Tp + t) * C + c]);
        }
        for (int k = threadIdx.x; k < K; k += blockDim.x) atomicAdd(&bbar[k], dlb[k]);
        __syncthreads();
    }
    for (int i = threadIdx.x; i < Tp * C; i += blockDim.x) {
        const int c = i % C, t = i / C;
        float a = 0.f;
        for (int k = 0; k < K; ++k)
            if (am[k] == t) a += w[k * C + c] * dlb[k] + v_w[k * C + c] * dl[k];
        if (mask != nullptr) a *= mask[((int64_t)clip * C + c) * Tp + t];
        u[i] = a;
    }
    __syncthreads();
    float* out = abar_feats + (int64_t)clip * C * To * Ho * Wo;
    for (int i = threadIdx.x; i < C * To * Ho * Wo; i += blockDim.x) {
        const int t = (i / (Wo * Ho)) % To, c = i / (Wo * Ho * To);
        float a = 0.f;
        for (int tp = t - kt + 1; tp <= t; ++tp) if (tp >= 0 && tp < Tp) a += u[tp * C + c];
        out[i] = a * inv;
    }
}

extern "C" int vd_head_second_order(const float* logits, const float* dlogits, const int32_t* amax_t, const float* dropped,
                                    const float* mask, const float* w, const float* v_w, const float* v_b,
                                    const float* gbar_feats, int64_t nclips, int C, int To, int Ho, int Wo, int kt, int kh, int kw,
                                    int K, float* abar_feats, float* wbar, float* bbar, float* dlogbar_out, void* stream) {
    if (nclips <= 0) return 0;
    if (Ho - kh + 1 != 1 || Wo - kw + 1 != 1 || To - kt + 1 < 1) return -2;
    const size_t lds = ((size_t)(To - kt + 1) * C + 2 * (size_t)K) * sizeof(float);
    hipLaunchKernelGGL(head_second_order_kernel, dim3((unsigned)nclips), dim3(256), lds, reinterpret_cast<hipStream_t>(stream),
                       logits, dlogits, amax_t, dropped, mask, w, v_w, v_b, gbar_feats, (int)nclips, C, To, Ho, Wo, kt, kh, kw, K,
                       abar_feats, wbar, bbar, dlogbar_out);
    return (int)hipGetLastError();
}

// torch.optim.SGD(momentum, weight_decay): g' = g + wd*p; buf = first ? g' : mu*buf + g'; p -= lr*buf.
__global__ void sgd_wd_kernel(float* __restrict__ x, float* __restrict__ buf, const float* __restrict__ g, int64_t n, float lr,
                              float mu, float wd, int first) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        // every operation rounded on its own (no fused multiply-add), as in sgd_momentum_kernel
#pragma clang fp contract(off)
        const float p = x[i];
        const float decay = wd * p;
        const float gv = g[i] + decay;
        const float prev = buf[i] * mu;
        const float bnew = first ? gv : prev + gv;
        buf[i] = bnew;
        const float step = lr * bnew;
        x[i] = p - step;
    }
}

extern "C" int vd_sgd_momentum_wd(float* x, float* buf, const float* g, int64_t n, float lr, float momentum, float wd,
                                  int first, void* stream) {
    if (n <= 0) return 0;
    int64_t blocks = (n + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(sgd_wd_kernel, dim3((unsigned)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), x, buf, g, n,
                       lr, momentum, wd, first);
    return (int)hipGetLastError();
}

// Batch-global standardisation of epoch() (utils.py:770): out = (x - mean(x)) / std(x), unbiased std.
// Sum and sum of squares are accumulated in fp64 from the first add on (a float's square is exact in fp64), so that the
// one-pass variance (sum x^2 - n mean^2) / (n - 1) keeps ~1e-10 even at |mean| / std = 1000, where fp32 partial sums lost
// 2.5e-2 of the output to the cancellation.  Per element that is two conversions and two fp64 adds in the first kernel and two
// conversions, an fp64 subtract and multiply in the second, against 4 + 8 bytes of HBM traffic.
__device__ __forceinline__ double block_sum_d(double v, double* red) {      // result valid in thread 0; fixed association
    v = wave_sum_d(v);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[w] = v;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0) {
        const int nw = (blockDim.x + 63) >> 6;
        for (int i = 0; i < nw; ++i) t += red[i];
    }
    return t;
}

__device__ __forceinline__ void sum_sumsq_thread(const float* __restrict__ x, int64_t n, double& s, double& q) {
    s = 0.0; q = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const double v = (double)x[i];
        s += v; q += v * v;
    }
}

// out = (x - mean) / std with the subtraction in fp64 and ONE rounding to fp32 (a float mean of 1000 is itself off by up to 3e-5)
__device__ __forceinline__ void standardize_apply(const float* __restrict__ x, int64_t n, double sum, double sumsq, float* __restrict__ out) {
    const double mean = sum / (double)n;
    const double var = (sumsq - (double)n * mean * mean) / (double)(n - 1);
    const double inv = 1.0 / sqrt(var);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        out[i] = (float)(((double)x[i] - mean) * inv);
}

__global__ void sum_sumsq_kernel(const float* __restrict__ x, int64_t n, double* __restrict__ acc) {
    __shared__ double red[16];
    double s, q;
    sum_sumsq_thread(x, n, s, q);
    const double ts = block_sum_d(s, red);
    const double tq = block_sum_d(q, red);
    if (threadIdx.x == 0) { atomicAdd(&acc[0], ts); atomicAdd(&acc[1], tq); }
}

__global__ void standardize_kernel(const float* __restrict__ x, int64_t n, const double* __restrict__ acc, float* __restrict__ out) {
    standardize_apply(x, n, acc[0], acc[1], out);
}

// Ordered mode: every block writes its two partial sums to its own slot; every block of the second kernel folds the slots in
// the same fixed order (lane-strided, then a fixed shuffle tree), so mean and std do not depend on the order blocks retire in.
__global__ void sum_sumsq_partial_kernel(const float* __restrict__ x, int64_t n, double* __restrict__ part) {
    __shared__ double red[16];
    double s, q;
    sum_sumsq_thread(x, n, s, q);
    const double ts = block_sum_d(s, red);
    const double tq = block_sum_d(q, red);
    if (threadIdx.x == 0) { part[2 * blockIdx.x] = ts; part[2 * blockIdx.x + 1] = tq; }
}

__global__ void standardize_ordered_kernel(const float* __restrict__ x, int64_t n, const double* __restrict__ part, int nparts,
                                           float* __restrict__ out) {
    __shared__ double tot[2];
    if (threadIdx.x < 64) {
        double s = 0.0, q = 0.0;
        for (int b = threadIdx.x; b < nparts; b += 64) { s += part[2 * b]; q += part[2 * b + 1]; }
        for (int off = 32; off > 0; off >>= 1) { s += __shfl_down(s, off, 64); q += __shfl_down(q, off, 64); }
        if (threadIdx.x == 0) { tot[0] = s; tot[1] = q; }
    }
    __syncthreads();
    standardize_apply(x, n, tot[0], tot[1], out);
}

// vd_standardize with a fixed summation order; `scratch` holds VD_STANDARDIZE_ORDERED_SCRATCH (4096) doubles, caller-owned.
extern "C" int vd_standardize_ordered(const float* x, int64_t n, double* scratch, float* out, void* stream) {
    if (n < 2) return -2;
    if (x == nullptr || scratch == nullptr || out == nullptr) return -1;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    int64_t blocks = (n + 256 * 16 - 1) / (256 * 16);
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(sum_sumsq_partial_kernel, dim3((unsigned)blocks), dim3(256), 0, st, x, n, scratch);
    hipLaunchKernelGGL(standardize_ordered_kernel, dim3((unsigned)blocks), dim3(256), 0, st, x, n, scratch, (int)blocks, out);
    return (int)hipGetLastError();
}

extern "C" int vd_standardize(const float* x, int64_t n, double* scratch2, float* out, void* stream) {
    if (n < 2) return -2;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipError_t e = hipMemsetAsync(scratch2, 0, 2 * sizeof(double), st);
    if (e != hipSuccess) return (int)e;
    int64_t blocks = (n + 256 * 16 - 1) / (256 * 16);
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(sum_sumsq_kernel, dim3((unsigned)blocks), dim3(256), 0, st, x, n, scratch2);
    hipLaunchKernelGGL(standardize_kernel, dim3((unsigned)blocks), dim3(256), 0, st, x, n, scratch2, out);
    return (int)hipGetLastError();
}

// MFMA-saturating microbenchmark ("a measured MFMA-saturating microbenchmark beside the spec
// figure").  Every wave issues `iters` x 8 MFMA groups from registers, no memory traffic in the loop.  The operands
// are pseudo-random and a different register pair feeds each group (the chip sheds clock with the energy per MFMA, so
// constant or trivial operands over-state what a real kernel can reach; MI355X_MICROARCH.md, DVFS give-back).
//   shape 0: v_mfma_f32_32x32x16_f16, 8 independent accumulators;  shape 1: v_mfma_f32_16x16x32_f16, the same
//   output tiles as 4 x (16x16) each, two instructions per 32x32x16 equivalent (same FLOP per group).
// FLOP = blocks * 4 waves * iters * 8 * 32768 either way.
typedef _Float16 vd_f16x8 __attribute__((ext_vector_type(8)));
typedef float vd_f32x16 __attribute__((ext_vector_type(16)));
typedef float vd_f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ vd_f16x8 peak_operand(uint32_t seed) {
    vd_f16x8 v;
    for (int i = 0; i < 8; ++i) {
        seed = seed * 1664525u + 1013904223u;
        v[i] = (_Float16)(((float)(seed >> 8) * (1.0f / 16777216.0f) - 0.5f) * 0.25f);
    }
    return v;
}

template <int SHAPE>
__global__ __launch_bounds__(256) void mfma_peak_kernel(int iters, float* __restrict__ out) {
    vd_f16x8 a[8], b[8];
    for (int t = 0; t < 8; ++t) {
        a[t] = peak_operand((uint32_t)(threadIdx.x * 131 + t * 7 + blockIdx.x));
        b[t] = peak_operand((uint32_t)(threadIdx.x * 17 + t * 29 + 5));
    }
    float s = 0.f;
    if constexpr (SHAPE == 0) {
        vd_f32x16 c[8] = {};
        for (int i = 0; i < iters; ++i) {
#pragma unroll
            for (int t = 0; t < 8; ++t) c[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[t], b[t], c[t], 0, 0, 0);
        }
        for (int t = 0; t < 8; ++t)
            for (int i = 0; i < 16; ++i) s += c[t][i];
    } else {
        vd_f32x4 c[16] = {};
        for (int i = 0; i < iters; ++i) {
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                c[2 * t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[t], b[t], c[2 * t], 0, 0, 0);
                c[2 * t + 1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[(t + 1) & 7], b[t], c[2 * t + 1], 0, 0, 0);
            }
        }
        for (int t = 0; t < 16; ++t)
            for (int i = 0; i < 4; ++i) s += c[t][i];
    }
    out[(int64_t)blockIdx.x * blockDim.x + threadIdx.x] = s;
}

extern "C" int vd_mfma_peak(int blocks, int iters, int shape, float* out, void* stream) {
    if (blocks <= 0 || iters <= 0 || out == nullptr || shape < 0 || shape > 1) return -1;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (shape == 0) hipLaunchKernelGGL(mfma_peak_kernel<0>, dim3((unsigned)blocks), dim3(256), 0, st, iters, out);
    else hipLaunchKernelGGL(mfma_peak_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, st, iters, out);
    return (int)hipGetLastError();
}

extern "C" int vd_abi_version(void) { return VD_ABI_VERSION; }

// ------------------------------------------------------------------------------------------------------------------------
// Decoded frames -> clips: HWC uint8 -> CHW fp32, (v / 255 - mean[c]) / std[c]  (torchvision ToTensor + Normalize as the
// reference's datasets apply them per frame, utils.py:171-173; here once per preload, on the device).  HBM-bound: 3 bytes
// read and 12 written per pixel.  Every operation is a correctly rounded fp32 one, so the result equals the host
// transform's bit for bit.
// ------------------------------------------------------------------------------------------------------------------------
// (FrameNorm / frame_norm1: frame_norm.h, shared with vd_clips_sample)

__global__ void frames_normalize_quad_kernel(const uint32_t* __restrict__ src, float* __restrict__ dst, int64_t nframes,
                                             int64_t quads_per_frame, FrameNorm nm) {
    const int64_t total = nframes * quads_per_frame;
    const int64_t hw = quads_per_frame * 4;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t f = i / quads_per_frame, q = i - f * quads_per_frame;
        const uint32_t* s = src + i * 3;                       // 4 pixels = 12 bytes
        const uint32_t a = s[0], b = s[1], c = s[2];           // r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
        float4 r, g, bl;
        r.x = frame_norm1(a & 255u, nm.mean[0], nm.std[0]);
        g.x = frame_norm1((a >> 8) & 255u, nm.mean[1], nm.std[1]);
        bl.x = frame_norm1((a >> 16) & 255u, nm.mean[2], nm.std[2]);
        r.y = frame_norm1(a >> 24, nm.mean[0], nm.std[0]);
        g.y = frame_norm1(b & 255u, nm.mean[1], nm.std[1]);
        bl.y = frame_norm1((b >> 8) & 255u, nm.mean[2], nm.std[2]);
        r.z = frame_norm1((b >> 16) & 255u, nm.mean[0], nm.std[0]);
        g.z = frame_norm1(b >> 24, nm.mean[1], nm.std[1]);
        bl.z = frame_norm1(c & 255u, nm.mean[2], nm.std[2]);
        r.w = frame_norm1((c >> 8) & 255u, nm.mean[0], nm.std[0]);
        g.w = frame_norm1((c >> 16) & 255u, nm.mean[1], nm.std[1]);
        bl.w = frame_norm1(c >> 24, nm.mean[2], nm.std[2]);
        float* d = dst + f * 3 * hw + q * 4;
        *reinterpret_cast<float4*>(d) = r;
        *reinterpret_cast<float4*>(d + hw) = g;
        *reinterpret_cast<float4*>(d + 2 * hw) = bl;
    }
}

__global__ void frames_normalize_scalar_kernel(const uint8_t* __restrict__ src, float* __restrict__ dst, int64_t nframes, int64_t hw,
                                               FrameNorm nm) {
    const int64_t total = nframes * hw;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t f = i / hw, p = i - f * hw;
        const uint8_t* s = src + i * 3;
        float* d = dst + f * 3 * hw + p;
        d[0] = frame_norm1(s[0], nm.mean[0], nm.std[0]);
        d[hw] = frame_norm1(s[1], nm.mean[1], nm.std[1]);
        d[2 * hw] = frame_norm1(s[2], nm.mean[2], nm.std[2]);
    }
}

extern "C" int vd_frames_normalize(const void* src_u8, float* dst, int64_t nframes, int height, int width, const float* mean3,
                                   const float* std3, void* stream) {
    if (nframes < 0 || height < 0 || width < 0 || !mean3 || !std3) return -1;
    const int64_t hw = (int64_t)height * width;
    if (nframes == 0 || hw == 0) return 0;
    if (!src_u8 || !dst) return -1;
    FrameNorm nm;
    for (int c = 0; c < 3; ++c) {
        nm.mean[c] = mean3[c]; nm.std[c] = std3[c];
        if (!(std3[c] != 0.f)) return -1;
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const bool vec = (hw % 4 == 0) && (reinterpret_cast<uintptr_t>(src_u8) % 4 == 0) && (reinterpret_cast<uintptr_t>(dst) % 16 == 0);
    const int64_t items = vec ? nframes * (hw / 4) : nframes * hw;
    int64_t blocks = (items + 255) / 256;
    if (blocks > 16384) blocks = 16384;
    if (vec)
        hipLaunchKernelGGL(frames_normalize_quad_kernel, dim3((unsigned)blocks), dim3(256), 0, st,
                           reinterpret_cast<const uint32_t*>(src_u8), dst, nframes, hw / 4, nm);
    else
        hipLaunchKernelGGL(frames_normalize_scalar_kernel, dim3((unsigned)blocks), dim3(256), 0, st,
                           reinterpret_cast<const uint8_t*>(src_u8), dst, nframes, hw, nm);
    return (int)hipGetLastError();
}

// Weight-gradient programs accumulate into scratch copies laid out [replica][cin*147 rows][cout cols] (cout minor, so the 32
// lanes of an atomic instruction fall into one 128-byte line instead of 32 lines 441..18816 floats apart) and spread
// their boxes over the copies.  This folds them back: out[col][row] += sum_r rep[r][row][col]  (out = dW, (cout, cin, 3, 7, 7)).
__global__ void replica_sum_kernel(const float* __restrict__ rep, int replicas, int rows, int cols, float* __restrict__ out) {
    __shared__ float tile[32][33];
    const int r0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
    const int64_t plane = (int64_t)rows * cols;
    for (int dy = threadIdx.y; dy < 32; dy += blockDim.y) {
        const int row = r0 + dy, col = c0 + threadIdx.x;
        float sum = 0.f;
        if (row < rows && col < cols)
            for (int r = 0; r < replicas; ++r) sum += rep[r * plane + (int64_t)row * cols + col];
        tile[dy][threadIdx.x] = sum;
    }
    __syncthreads();
    for (int dy = threadIdx.y; dy < 32; dy += blockDim.y) {
        const int col = c0 + dy, row = r0 + threadIdx.x;
        if (row < rows && col < cols) out[(int64_t)col * rows + row] += tile[threadIdx.x][dy];
    }
}

// Many copies (the ordered mode gives every box of positions its own: 896 for the first level at 112x112x16): first fold
// groups of VD_REPLICA_GROUP consecutive copies IN PLACE into the group's first copy -- one thread per (group, element), copies
// added in index order --, then fold the group heads with the kernel above (stride = group).  Fixed association, no atomics:
// bitwise reproducible; 100 MB of copies stream through ~3000 workgroups instead of 28.
#define VD_REPLICA_GROUP 32
__global__ __launch_bounds__(256) void replica_group_sum_kernel(float* __restrict__ rep, int replicas, int64_t plane) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= plane) return;
    const int r0 = blockIdx.y * VD_REPLICA_GROUP;
    const int r1 = r0 + VD_REPLICA_GROUP < replicas ? r0 + VD_REPLICA_GROUP : replicas;
    float sum = 0.f;
    for (int r = r0; r < r1; ++r) sum += rep[(int64_t)r * plane + i];
    rep[(int64_t)r0 * plane + i] = sum;
}

__global__ void replica_sum_strided_kernel(const float* __restrict__ rep, int replicas, int stride, int rows, int cols, float* __restrict__ out) {
    __shared__ float tile[32][33];
    const int r0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
    const int64_t plane = (int64_t)rows * cols;
    for (int dy = threadIdx.y; dy < 32; dy += blockDim.y) {
        const int row = r0 + dy, col = c0 + threadIdx.x;
        float sum = 0.f;
        if (row < rows && col < cols)
            for (int r = 0; r < replicas; r += stride) sum += rep[r * plane + (int64_t)row * cols + col];
        tile[dy][threadIdx.x] = sum;
    }
    __syncthreads();
    for (int dy = threadIdx.y; dy < 32; dy += blockDim.y) {
        const int col = c0 + dy, row = r0 + threadIdx.x;
        if (row < rows && col < cols) out[(int64_t)col * rows + row] += tile[threadIdx.x][dy];
    }
}

extern "C" int vd_replica_sum(float* rep, int replicas, int rows, int cols, float* out, void* stream) {
    if (replicas < 0 || rows < 0 || cols < 0) return -1;
    if (replicas == 0 || rows == 0 || cols == 0) return 0;
    if (!rep || !out) return -1;
    if (replicas > 2 * VD_REPLICA_GROUP) {
        const int64_t plane = (int64_t)rows * cols;
        const int groups = (replicas + VD_REPLICA_GROUP - 1) / VD_REPLICA_GROUP;
        hipLaunchKernelGGL(replica_group_sum_kernel, dim3((unsigned)((plane + 255) / 256), (unsigned)groups), dim3(256), 0,
                           reinterpret_cast<hipStream_t>(stream), rep, replicas, plane);
        hipLaunchKernelGGL(replica_sum_strided_kernel, dim3((unsigned)((rows + 31) / 32), (unsigned)((cols + 31) / 32)), dim3(32, 8), 0,
                           reinterpret_cast<hipStream_t>(stream), rep, replicas, VD_REPLICA_GROUP, rows, cols, out);
        return (int)hipGetLastError();
    }
    hipLaunchKernelGGL(replica_sum_kernel, dim3((unsigned)((rows + 31) / 32), (unsigned)((cols + 31) / 32)), dim3(32, 8), 0,
                       reinterpret_cast<hipStream_t>(stream), rep, replicas, rows, cols, out);
    return (int)hipGetLastError();
}
