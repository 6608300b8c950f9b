"""Restatement of the predictor's finish on the host (torch-CPU and numpy only; nothing from oracle/): arg-max objectness with the
FIRST maximum -> F.interpolate bilinear, align_corners=False -> crop (scale > 0) or resize (scale == 0) -> > 0.5 ->
mask_generator.rle_encode.  Shared by tests/test_predictor_cpu.py, tests/test_hip_predict.py and tests/test_hip_predictor.py."""
import numpy as np
import torch
import torch.nn.functional as F

from selfmask_amd.mask_generator import rle_encode

THRESHOLD = 0.5  # evaluator.MASK_THRESHOLD


def first_argmax(objectness) -> int:
    o = np.asarray(objectness, np.float32).reshape(-1)
    return int(np.flatnonzero(o == o.max())[0])


def upsampled(mask: torch.Tensor, size, scale: float) -> torch.Tensor:
    """(mh, mw) float32 -> (H, W) float32: scale > 0: F.interpolate(scale_factor=scale)[:H, :W], zero outside the up-sampled plane;
    scale == 0: F.interpolate(size=(H, W))"""
    H, W = size
    m = mask.detach().cpu().float()[None, None]
    if scale > 0:
        up = F.interpolate(m, scale_factor=float(scale), mode="bilinear", align_corners=False)[0, 0]
        out = torch.zeros((H, W), dtype=torch.float32)
        h, w = min(H, up.shape[0]), min(W, up.shape[1])
        out[:h, :w] = up[:h, :w]
        return out
    return F.interpolate(m, size=(H, W), mode="bilinear", align_corners=False)[0, 0]


def finish_one(masks: torch.Tensor, objectness, size, scale: float) -> dict:
    """masks (nq, mh, mw), objectness (nq,) of ONE image -> {"best", "value" (H, W) float32, "binary", "soft" uint8, "rle"}"""
    best = first_argmax(objectness)
    v = upsampled(masks[best], size, scale).numpy()
    binary = (v > np.float32(THRESHOLD)).astype(np.uint8)
    soft = (np.clip(v, 0, 1) * 255).astype(np.uint8)  # app.py:283 / :297: clip, then a truncating cast
    return {"best": best, "value": v, "binary": binary, "soft": soft, "rle": rle_encode(binary)}


def finish(masks: torch.Tensor, objectness: torch.Tensor, sizes, scale: float):
    masks, objectness = masks.detach().cpu().float(), objectness.detach().cpu().float()
    return [finish_one(masks[b], objectness[b].numpy(), sizes[b], scale) for b in range(len(sizes))]
