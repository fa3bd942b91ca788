// Clips drawn per read out of a device-resident store of whole videos (dataset.ResidentVideos / ResidentClipLoader).
//
// Reference: the `__getitem__` of the frame-folder datasets (distill_utils/dataset.py:146-568) opens 16 JPEGs per read, flips
// them, resizes / crops and normalises on one host thread; its test loader draws a new start frame and a new flip on every
// read, so nothing of that can be frozen by a preload.  Here every frame of every video is decoded once into
// frames (F, Hs, Ws, 3) uint8 in HBM (resized, unflipped, uncropped), the draws of a batch are made on the host into three small
// tables, and one launch gathers + mirrors + crops + normalises:
//   dst[b][t][c][y][x] = norm(frames[row[b*T+t]][i + y][sx][c]),   sx = flip[b] ? Ws - 1 - (j + x) : j + x,
// (i, j) = crop_yx[(b*T+t)*2 ..] or (0, 0).  PIL's flip and its bilinear resize commute, so reading the stored frame mirrored
// is the host's flip -> resize -> crop.  HBM-bound: 3 bytes read and 12 written per pixel, plus one table row per frame.
//   clips_sample_quad_kernel   : no crop, Ws % 4 == 0, aligned bases: a lane reads three dwords (four pixels) and writes three
//                                float4; a flipped frame reads the mirrored quad of the same row and reverses it in registers.
//                                A lane keeps its quad and walks over frames, so the table entries are workgroup-uniform.
//   clips_sample_scalar_kernel : everything else (crops, odd widths, unaligned views), one pixel per lane.
// A row outside the store (or a crop outside the frame) is skipped by the kernels; the Python layer refuses such tables before
// they are uploaded.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vd_hip.h"
#include "frame_norm.h"

namespace {

// grid: x = 256-quad chunks of a frame, y strides over the frames -- the frame (its table row, its clip's flip) is uniform over a
// workgroup, so the tables are read with scalar loads and no lane divides a 64-bit index
__global__ __launch_bounds__(256) void clips_sample_quad_kernel(const uint32_t* __restrict__ frames, int64_t store_frames,
                                                                const int64_t* __restrict__ frame_row,
                                                                const uint8_t* __restrict__ flip, int nframes, int T,
                                                                int quads_per_row, int quads_per_frame,
                                                                float* __restrict__ dst, FrameNorm nm) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= quads_per_frame) return;
    const int y = q / quads_per_row, xq = q - y * quads_per_row;
    const int mq = y * quads_per_row + (quads_per_row - 1 - xq);                // the mirrored quad of the same row
    const int64_t hw = (int64_t)quads_per_frame * 4;
    for (int f = blockIdx.y; f < nframes; f += gridDim.y) {
        const int64_t row = frame_row[f];
        if (row < 0 || row >= store_frames) continue;
        const bool fl = flip[f / T] != 0;
        const uint32_t* s = frames + (row * quads_per_frame + (fl ? mq : q)) * 3;      // 4 pixels = 12 bytes
        const uint32_t a = s[0], b = s[1], c = s[2];                            // r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
        uint32_t p0 = a & 0xffffffu, p1 = (a >> 24) | ((b & 0xffffu) << 8), p2 = (b >> 16) | ((c & 0xffu) << 16), p3 = c >> 8;
        if (fl) {                                                               // (b g r packed per pixel; reverse the quad)
            uint32_t t0 = p0, t1 = p1;
            p0 = p3; p1 = p2; p2 = t1; p3 = t0;
        }
        float4 r, g, bl;
        r.x = frame_norm1(p0 & 255u, nm.mean[0], nm.std[0]);
        g.x = frame_norm1((p0 >> 8) & 255u, nm.mean[1], nm.std[1]);
        bl.x = frame_norm1(p0 >> 16, nm.mean[2], nm.std[2]);
        r.y = frame_norm1(p1 & 255u, nm.mean[0], nm.std[0]);
        g.y = frame_norm1((p1 >> 8) & 255u, nm.mean[1], nm.std[1]);
        bl.y = frame_norm1(p1 >> 16, nm.mean[2], nm.std[2]);
        r.z = frame_norm1(p2 & 255u, nm.mean[0], nm.std[0]);
        g.z = frame_norm1((p2 >> 8) & 255u, nm.mean[1], nm.std[1]);
        bl.z = frame_norm1(p2 >> 16, nm.mean[2], nm.std[2]);
        r.w = frame_norm1(p3 & 255u, nm.mean[0], nm.std[0]);
        g.w = frame_norm1((p3 >> 8) & 255u, nm.mean[1], nm.std[1]);
        bl.w = frame_norm1(p3 >> 16, nm.mean[2], nm.std[2]);
        float* d = dst + (int64_t)f * 3 * hw + (int64_t)q * 4;
        *reinterpret_cast<float4*>(d) = r;
        *reinterpret_cast<float4*>(d + hw) = g;
        *reinterpret_cast<float4*>(d + 2 * hw) = bl;
    }
}

__global__ __launch_bounds__(256) void clips_sample_scalar_kernel(const uint8_t* __restrict__ frames, int64_t store_frames,
                                                                  int src_h, int src_w, const int64_t* __restrict__ frame_row,
                                                                  const int32_t* __restrict__ crop_yx,
                                                                  const uint8_t* __restrict__ flip, int64_t nframes, int T,
                                                                  int out_h, int out_w, float* __restrict__ dst, FrameNorm nm) {
    const int64_t hw = (int64_t)out_h * out_w;
    const int64_t total = nframes * hw;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t f = i / hw;
        const int p = (int)(i - f * hw);
        const int64_t row = frame_row[f];
        if (row < 0 || row >= store_frames) continue;
        const int cy = crop_yx ? crop_yx[2 * f] : 0, cx = crop_yx ? crop_yx[2 * f + 1] : 0;
        if (cy < 0 || cx < 0 || cy > src_h - out_h || cx > src_w - out_w) continue;
        const int y = p / out_w, x = p - y * out_w;
        const int sx = flip[f / T] ? src_w - 1 - (cx + x) : cx + x;
        const uint8_t* s = frames + ((row * src_h + (cy + y)) * src_w + sx) * 3;
        float* d = dst + f * 3 * hw + p;
        d[0] = frame_norm1(s[0], nm.mean[0], nm.std[0]);
        d[hw] = frame_norm1(s[1], nm.mean[1], nm.std[1]);
        d[2 * hw] = frame_norm1(s[2], nm.mean[2], nm.std[2]);
    }
}

}  // namespace

extern "C" int vd_clips_sample(const void* frames_u8, int64_t store_frames, int src_h, int src_w, const int64_t* frame_row,
                               const int32_t* crop_yx, const uint8_t* flip, int64_t nclips, int T, int out_h, int out_w,
                               float* dst, const float* mean3, const float* std3, void* stream) {
    if (store_frames < 0 || src_h < 0 || src_w < 0 || nclips < 0 || T < 0 || out_h < 0 || out_w < 0 || !mean3 || !std3) return -1;
    if (out_h > src_h || out_w > src_w) return -1;
    if (!crop_yx && (out_h != src_h || out_w != src_w)) return -1;
    FrameNorm nm;
    for (int c = 0; c < 3; ++c) {
        nm.mean[c] = mean3[c]; nm.std[c] = std3[c];
        if (!(std3[c] != 0.f)) return -1;
    }
    const int64_t nframes = nclips * T;
    const int64_t hw = (int64_t)out_h * out_w;
    if (nframes == 0 || hw == 0) return 0;
    if (!frames_u8 || !frame_row || !flip || !dst) return -1;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const bool vec = !crop_yx && (out_w % 4 == 0) && (reinterpret_cast<uintptr_t>(frames_u8) % 4 == 0) &&
                     (reinterpret_cast<uintptr_t>(dst) % 16 == 0) && nframes <= INT32_MAX && hw / 4 <= INT32_MAX - 256;
    if (vec) {
        const int64_t gx = (hw / 4 + 255) / 256;                 // chunks of a frame; x * y capped as the scalar grid is
        int64_t gy = gx >= 16384 ? 1 : 16384 / gx;
        if (gy > nframes) gy = nframes;
        if (gy > 65535) gy = 65535;
        hipLaunchKernelGGL(clips_sample_quad_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, st,
                           reinterpret_cast<const uint32_t*>(frames_u8), store_frames, frame_row, flip, (int)nframes, T, out_w / 4,
                           (int)(hw / 4), dst, nm);
        return (int)hipGetLastError();
    }
    int64_t blocks = (nframes * hw + 255) / 256;
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL(clips_sample_scalar_kernel, dim3((unsigned)blocks), dim3(256), 0, st,
                       reinterpret_cast<const uint8_t*>(frames_u8), store_frames, src_h, src_w, frame_row, crop_yx, flip, nframes, T,
                       out_h, out_w, dst, nm);
    return (int)hipGetLastError();
}
