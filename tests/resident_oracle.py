"""Numpy restatement of vd_clips_sample (include/vd_hip.h): gather, mirror, crop, normalise.  Every fp32 operation of numpy is
correctly rounded, as the kernel's are, so the comparison is bit for bit."""
import numpy as np


def normalise(u8, mean, std):
    """(..., 3) uint8 -> (..., 3) fp32: (v / 255 - mean[c]) / std[c] in fp32, operation by operation."""
    x = u8.astype(np.float32) / np.float32(255)
    x = x - np.asarray(mean, dtype=np.float32)
    return x / np.asarray(std, dtype=np.float32)


def clips_sample(frames, frame_row, flip, crop_yx, frames_per_clip, out_hw, mean, std):
    """frames (F, Hs, Ws, 3) uint8, frame_row (b*T), flip (b), crop_yx (b*T, 2) or None -> (b, T, 3, H, W) fp32."""
    frames = np.asarray(frames)
    rows = np.asarray(frame_row).reshape(-1)
    flip = np.asarray(flip).reshape(-1)
    t = int(frames_per_clip)
    oh, ow = out_hw
    ws = frames.shape[2]
    out = np.empty((flip.size, t, 3, oh, ow), dtype=np.float32)
    for b in range(flip.size):
        for k in range(t):
            f = b * t + k
            i, j = (0, 0) if crop_yx is None else (int(v) for v in np.asarray(crop_yx).reshape(-1, 2)[f])
            src = frames[rows[f]]
            xs = np.arange(j, j + ow)
            if flip[b]:
                xs = ws - 1 - xs
            px = src[i:i + oh][:, xs]                                   # (oh, ow, 3)
            out[b, k] = np.moveaxis(normalise(px, mean, std), -1, 0)
    return out
