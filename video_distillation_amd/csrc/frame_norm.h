// The per-value arithmetic of the frame kernels (vd_frames_normalize in aux_kernels.hip, vd_clips_sample in clips_sample.hip):
// uint8 -> fp32, (v / 255 - mean[c]) / std[c], every operation a correctly rounded fp32 one, so the result equals torchvision's
// ToTensor + Normalize (dataset.FrameTransform.normalise) bit for bit.  One definition, so that the kernels cannot drift apart.
#ifndef VD_FRAME_NORM_H
#define VD_FRAME_NORM_H

#include <hip/hip_runtime.h>

struct FrameNorm { float mean[3]; float std[3]; };

__device__ __forceinline__ float frame_norm1(unsigned v, float mean, float sd) {
    return __fdiv_rn(__fsub_rn(__fdiv_rn((float)v, 255.0f), mean), sd);
}

#endif /* VD_FRAME_NORM_H */
