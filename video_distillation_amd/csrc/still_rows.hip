// Still clips straight into the first level's operand rows (distill.StillDMTrainer's real side).
//
// A batch of still clips is images[index[i]] repeated over T frames.  The first conv level reads its input as padded 16-bit pixel
// rows [clip][t*3+c][h][pix_row_pitch(W)] (vd_pix2rows: 3 zero pixels in front, zeros behind).  Building them with what there was
// takes vds_still_expand (fp32 clips written) and vd_pix2rows (those read back, the rows written); the T frames of a still clip
// hold the same rows, so here a lane
//   - owns one 16-byte chunk (8 pixels) of one padded row of one image plane,
//   - builds it ONCE: three aligned float4 loads cover x[8j-4 .. 8j+7] when W % 4 == 0 and the base is 16-byte aligned, eight
//     guarded scalar loads otherwise; one split16p per pixel (split16.h: the conversion vd_pix2rows makes),
//   - and stores it at the T frame positions of the clip (and of the low plane where there is one).
// Consecutive lanes take consecutive chunks of an image (chunk q = (c*H + h)*cpr + j), so each of the T store streams of a
// workgroup is contiguous.  grid x = 256-chunk pieces of an image, grid y strides over the clips: `index[i]` is workgroup-
// uniform.  Offsets are 64-bit (3400 clips of 16x3x112x112 are 4.4e9 bytes of rows).  No LDS, no atomics, plain vector stores.
// The bytes are those of vd_pix2rows(vds_still_expand(...)), both planes (tests/test_gpu_still_dm.py).
// `index` is not checked on the device: hip.still_rows refuses a row outside the images before it is uploaded.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vd_hip.h"
#include "split16.h"

namespace {

template <bool VEC>
__global__ __launch_bounds__(256) void still_rows_kernel(const float* __restrict__ images, const int64_t* __restrict__ index,
                                                         int64_t n, int T, int H, int W, int cpr, uint4* __restrict__ hi,
                                                         uint4* __restrict__ lo, int prec) {
    const int per_frame = 3 * H * cpr;                      // chunks of one frame of a clip == of one image
    const int q = (int)(blockIdx.x * 256 + threadIdx.x);
    if (q >= per_frame) return;
    const int r = q / cpr, j = q - r * cpr;                 // r = c*H + h: row of the image
    const int w0 = 8 * j - 3;
    for (int64_t i = blockIdx.y; i < n; i += gridDim.y) {
        const int64_t row = index ? index[i] : i;
        const float* xr = images + (row * 3 * H + r) * W;
        uint16_t h16[8], l16[8];
        if (VEC) {
            float f[12];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int wq = 8 * j - 4 + 4 * k;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (wq >= 0 && wq < W) v = *reinterpret_cast<const float4*>(xr + wq);
                f[4 * k] = v.x; f[4 * k + 1] = v.y; f[4 * k + 2] = v.z; f[4 * k + 3] = v.w;
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
        const int64_t o = i * T * per_frame + q;
        uint4* dh = hi + o;
#pragma unroll 4
        for (int t = 0; t < T; ++t) dh[(int64_t)t * per_frame] = vh;
        if (lo != nullptr) {
            vl.x = l16[0] | ((uint32_t)l16[1] << 16); vl.y = l16[2] | ((uint32_t)l16[3] << 16);
            vl.z = l16[4] | ((uint32_t)l16[5] << 16); vl.w = l16[6] | ((uint32_t)l16[7] << 16);
            uint4* dl = lo + o;
#pragma unroll 4
            for (int t = 0; t < T; ++t) dl[(int64_t)t * per_frame] = vl;
        }
    }
}

}  // namespace

extern "C" int vdsr_still_rows(const float* images, const int64_t* index, int64_t n, int T, int H, int W, void* out_hi, void* out_lo,
                               int prec, void* stream) {
    if (T <= 0 || H <= 0 || W <= 0 || n < 0 || prec < VD_PREC_BF16 || prec > VD_PREC_F16X3) return -1;
    if (n == 0) return 0;
    if (!images || !out_hi) return -1;
    const int cpr = ((W + 8) + 7) / 8;          // 16-byte chunks per padded row (pix_row_pitch(W) / 8)
    const int64_t per_frame = (int64_t)3 * H * cpr;
    if (per_frame > INT32_MAX) return -1;
    const dim3 grid((unsigned)((per_frame + 255) / 256), (unsigned)(n < 65535 ? n : 65535));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    uint4* hi = reinterpret_cast<uint4*>(out_hi);
    uint4* lo = reinterpret_cast<uint4*>(out_lo);
    if (W % 4 == 0 && reinterpret_cast<uintptr_t>(images) % 16 == 0) {
        hipLaunchKernelGGL(still_rows_kernel<true>, grid, dim3(256), 0, st, images, index, n, T, H, W, cpr, hi, lo, prec);
    } else {
        hipLaunchKernelGGL(still_rows_kernel<false>, grid, dim3(256), 0, st, images, index, n, T, H, W, cpr, hi, lo, prec);
    }
    return (int)hipGetLastError();
}
