"""Plain references for the per-kernel parity tests of the forward's glue kernels (test_hip_forward_kernels.py).

Everything here runs on the CPU in numpy / torch-fp64 and is itself witnessed by test_kernel_refs_cpu.py, so what the GPU
tests expect can be checked on a machine without a GPU.
"""
import numpy as np
import torch
import torch.nn.functional as F

EMBED = 384
# f16 rounds with unit roundoff 2^-11: |x - hi| <= 2^-11 |x| and lo carries that remainder to another 2^-11, so
# |unsplit(split(x)) - x| <= 2^-22 |x| while lo stays a normal f16; 2^-21 is the issue's figure for the format (2x slack)
F16X2_REL = 2.0 ** -21


# ---- F16X2 --------------------------------------------------------------------------------------------------------------
def split_bits(x) -> np.ndarray:
    """The definition of the F16X2 format, in numpy: per group of 8, hi = f16(x) (round to nearest even) then
    lo = f16((x - hi) * 2^11), both evaluated in fp32.  (..., K) fp32 -> (..., K/8, 2, 8) uint16."""
    xn = np.ascontiguousarray(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x, dtype=np.float32)
    assert xn.shape[-1] % 8 == 0
    hi = xn.astype(np.float16)
    lo = ((xn - hi.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
    g = xn.shape[:-1] + (xn.shape[-1] // 8, 8)
    return np.stack([hi.reshape(g), lo.reshape(g)], axis=-2).view(np.uint16)


def container_bits(t: torch.Tensor) -> np.ndarray:
    """The bits of a tensor that HOLDS F16X2 data (fp32 container, 4 B per element): (..., K) -> (..., K/8, 2, 8) uint16."""
    c = t.detach().cpu().contiguous()
    return c.view(torch.float16).reshape(*c.shape[:-1], c.shape[-1] // 8, 2, 8).numpy().view(np.uint16)


def unsplit(t: torch.Tensor) -> torch.Tensor:
    """fp64 values an F16X2 container stands for: hi + lo / 2048."""
    c = t.detach().cpu().contiguous()
    h = c.view(torch.float16).reshape(*c.shape[:-1], c.shape[-1] // 8, 2, 8).double()
    return (h[..., 0, :] + h[..., 1, :] / 2048.0).reshape(c.shape)


# ---- row maps and LayerNorm ---------------------------------------------------------------------------------------------
def map_rows(rows: int, m) -> torch.Tensor:
    """sm_row_map: logical row r -> (r / group) * stride + offset + r % group; group 0 = identity."""
    r = torch.arange(rows, dtype=torch.int64)
    group, stride, offset = m
    return r if group == 0 else (r // group) * stride + offset + r % group


def layernorm_ref(x, gamma, beta, eps: float) -> torch.Tensor:
    return F.layer_norm(x.double(), (x.shape[-1],), gamma.double(), beta.double(), eps)


def partial_sum_f32(parts: torch.Tensor, bias: torch.Tensor, residual: torch.Tensor) -> torch.Tensor:
    """The fused split-K reduction in the documented order, every step rounded to fp32: slices in order, then the bias, then the
    residual.  parts (S, rows, C), bias (C), residual (rows, C), all fp32 on the CPU."""
    assert parts.dtype == bias.dtype == residual.dtype == torch.float32
    v = parts[0].clone()
    for s in range(1, parts.shape[0]):
        v = v + parts[s]
    return (v + bias[None, :]) + residual


# ---- bilinear, align_corners=False, as ATen evaluates F.interpolate(scale_factor=sf) for a float input -------------------------
def bilinear_taps(size: int, sf: int, fused: bool = True):
    """Taps of one axis: (i0, i1, w1) for the sf * size outputs.  The scale 1 / sf is rounded to fp32 and the source coordinate
    max(inv * (o + 0.5) - 0.5, 0) is an fp32 value, i1 = min(i0 + 1, size - 1); w1 = coordinate - i0 (exact in fp32) is returned
    in fp64.  ATen writes the coordinate as `scale * (dst + 0.5) - 0.5`; the compilers of torch's CPU build and of the HIP
    library both contract it into ONE fused multiply-add, so that is the rule here: product and difference are exact in fp64
    (24 x 13 significant bits) and rounded to fp32 once.  `fused=False` rounds the product first - up to an ulp of the
    coordinate (1e-6 in the weights at column 48) away from torch for a scale that is not a power of two; the CPU tests show both."""
    inv = np.float32(1.0 / sf)
    o = np.arange(sf * size, dtype=np.float32) + np.float32(0.5)
    if fused:
        src = (np.float64(inv) * o.astype(np.float64) - 0.5).astype(np.float32)
    else:
        src = inv * o - np.float32(0.5)
    assert src.dtype == np.float32
    src = np.maximum(src, np.float32(0.0))
    i0 = src.astype(np.int64)
    i1 = np.minimum(i0 + 1, size - 1)
    w1 = (src - i0.astype(np.float32)).astype(np.float64)
    return torch.from_numpy(i0), torch.from_numpy(i1), torch.from_numpy(w1)


def bilinear_ref(x: torch.Tensor, sf: int) -> torch.Tensor:
    """x (..., gh, gw) -> (..., sf gh, sf gw) fp64: the fp32 taps above, blended in fp64."""
    gh, gw = x.shape[-2:]
    y0, y1, wy = bilinear_taps(gh, sf)
    x0, x1, wx = bilinear_taps(gw, sf)
    xd = x.double()
    rows = xd[..., :, x0] * (1 - wx) + xd[..., :, x1] * wx  # along x on the gh source rows, then along y
    return rows[..., y0, :] * (1 - wy)[:, None] + rows[..., y1, :] * wy[:, None]


def tokens_to_planes(tok: torch.Tensor, gh: int, gw: int) -> torch.Tensor:
    """channels-last tokens (B, gh*gw, C) -> (B, C, gh, gw)"""
    return tok.permute(0, 2, 1).reshape(tok.shape[0], tok.shape[2], gh, gw)


def planes_to_tokens(p: torch.Tensor) -> torch.Tensor:
    """(B, C, h, w) -> (B, h*w, C)"""
    return p.permute(0, 2, 3, 1).reshape(p.shape[0], p.shape[2] * p.shape[3], p.shape[1])
