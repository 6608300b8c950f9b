"""Per-operator Python entry points over the C ABI (torch tensors in, torch tensors out, current HIP stream).

PyTorch is plumbing here: device memory + streams.  Every function launches hand-written gfx950 kernels from
libselfmask_hip.so and raises if handed a CPU tensor (there is no fallback path).
"""
import ctypes
from typing import Optional, Tuple

import torch

from . import _native as N
from .runs import ObjectOptions, PendingRuns, batch_segments_to_rles, segments_to_rles  # noqa: F401  (part of this module's surface)
from .voting import knn  # noqa: F401  (sm_knn_f32: the neighbour lists of 384-d / 2048-d points)


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _dev(*ts):
    for t in ts:
        if t is not None and (not t.is_cuda or t.dtype != torch.float32):
            raise RuntimeError("selfmask_amd ops need float32 tensors on a HIP device (no CPU fallback)")


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def gemm(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, epilogue: int = N.EPI_BIAS,
         residual: Optional[torch.Tensor] = None,
         tile: Optional[Tuple[int, int]] = None, out: Optional[torch.Tensor] = None,
         out2: Optional[torch.Tensor] = None, a_alt: Optional[torch.Tensor] = None, alt_from_n: int = 0,
         split_k: int = 1) -> torch.Tensor:
    """C = epilogue(A W^T + bias).  a: (M,K) or (batch,M,K); w: (N,K) or (batch,N,K) (torch Linear layout)."""
    _dev(a, w, bias, residual)
    lib = N.load()
    a3 = a if a.dim() == 3 else a.unsqueeze(0)
    w3 = w if w.dim() == 3 else w.unsqueeze(0)
    assert a3.stride(-1) == 1 and w3.stride(-1) == 1
    batch = max(a3.shape[0], w3.shape[0])
    M, K = a3.shape[1], a3.shape[2]
    Nn = w3.shape[1]
    c = out if out is not None else torch.empty((max(batch, split_k), M, Nn), device=a.device, dtype=torch.float32)
    c3 = c if c.dim() == 3 else c.unsqueeze(0)
    g = N.GemmArgs()
    g.A, g.W, g.bias, g.C = a3.data_ptr(), w3.data_ptr(), _ptr(bias), c3.data_ptr()
    g.strideA = a3.stride(0) if a3.shape[0] > 1 else 0
    g.strideW = w3.stride(0) if w3.shape[0] > 1 else 0
    g.strideC = c3.stride(0)
    g.M, g.N, g.K = M, Nn, K
    g.lda, g.ldw, g.ldc = a3.stride(1), w3.stride(1), c3.stride(1)
    g.batch, g.epilogue = batch, epilogue
    if split_k > 1:  # slice s of the K range lands in c[s] (raw partial products; the caller sums the slices)
        assert batch == 1 and c3.shape[0] >= split_k
        g.split_k = split_k
    if a_alt is not None:
        g.A_alt, g.alt_from_n = a_alt.data_ptr(), alt_from_n
    if residual is not None:
        r3 = residual if residual.dim() == 3 else residual.unsqueeze(0)
        g.R, g.ldr = r3.data_ptr(), r3.stride(1)
        g.strideR = r3.stride(0) if r3.shape[0] > 1 else 0
    if epilogue == N.EPI_SIGMOID2:
        c2 = out2 if out2 is not None else torch.empty_like(c)
        g.C2 = c2.data_ptr()
    if tile is None:
        N.check(lib.sm_gemm_f32(g, _stream()), "sm_gemm_f32")
    else:
        N.check(lib.sm_gemm_f32_tile(g, tile[0], tile[1], _stream()), "sm_gemm_f32_tile")
    res = c if a.dim() == 3 or w.dim() == 3 or out is not None or split_k > 1 else c[0]
    if epilogue == N.EPI_SIGMOID2:
        return res, (c2 if c2.dim() == res.dim() else c2[0])
    return res


def split_f16x2(x: torch.Tensor) -> torch.Tensor:
    """fp32 (..., K) -> F16X2 (same shape / dtype container: 4 B per element, hi/lo f16 halves per group of 8)."""
    _dev(x)
    x2 = x.reshape(-1, x.shape[-1])
    assert x2.stride(1) == 1
    out = torch.empty((x2.shape[0], x2.shape[1]), device=x.device, dtype=torch.float32)
    N.check(N.load().sm_split_f16x2(x2.data_ptr(), x2.stride(0), out.data_ptr(), out.stride(0), x2.shape[0], x2.shape[1],
                                    _stream()), "sm_split_f16x2")
    return out.view(x.shape)


def unsplit_f16x2(t: torch.Tensor) -> torch.Tensor:
    """F16X2 (..., K) -> the fp32 values it stands for (hi + lo / 2048); inverse of split_f16x2 up to the format's 22 bits."""
    k = t.shape[-1]
    h = t.contiguous().view(torch.float16).reshape(*t.shape[:-1], k // 8, 2, 8).float()
    return (h[..., 0, :] + h[..., 1, :] / 2048.0).reshape(t.shape)


def gemm_f16x2(a_split: torch.Tensor, w_split: torch.Tensor, bias=None, epilogue: int = N.EPI_BIAS, residual=None,
               tile=(128, 128), out=None, out_f16x2: bool = False, split_k: int = 1, ln=None):
    """C = epilogue(A W^T + bias) with A, W in F16X2 format (see split_f16x2).  2-D operands, or 3-D (batch, rows, K)
    for a batched launch (no split_k then).  Test / tuning entry: the forward drives the kernel from C."""
    _dev(a_split, w_split, bias, residual)
    batched = a_split.dim() == 3
    assert not (batched and split_k > 1)
    a3 = a_split if batched else a_split.unsqueeze(0)
    w3 = w_split if batched else w_split.unsqueeze(0)
    nb, M, K = a3.shape
    Nn = w3.shape[1]
    c = out if out is not None else torch.empty((max(nb, split_k), M, Nn), device=a_split.device, dtype=torch.float32)
    c3 = c if c.dim() == 3 else c.unsqueeze(0)
    g = N.GemmArgs()
    g.A, g.W, g.bias, g.C = a3.data_ptr(), w3.data_ptr(), _ptr(bias), c3.data_ptr()
    g.strideA, g.strideW, g.strideC = a3.stride(0), w3.stride(0), c3.stride(0)
    g.M, g.N, g.K = M, Nn, K
    g.lda, g.ldw, g.ldc = a3.stride(1), w3.stride(1), c3.stride(1)
    g.batch, g.epilogue, g.split_k = nb, epilogue, split_k if split_k > 1 else 0
    if residual is not None:
        r3 = residual if residual.dim() == 3 else residual.unsqueeze(0)
        g.R, g.ldr, g.strideR = r3.data_ptr(), r3.stride(1), r3.stride(0)
    xn = None
    if ln is not None:  # (gamma, beta, eps): C = R + A W^T + bias and C2 = LayerNorm(C) in F16X2 (64x384 tile, N = 384)
        gamma, beta, eps = ln
        xn = torch.empty_like(c3)
        g.epilogue, g.C2, g.ln_gamma, g.ln_beta, g.ln_eps = N.EPI_RESIDUAL_LN, xn.data_ptr(), gamma.data_ptr(), beta.data_ptr(), eps
    N.check(N.load().sm_gemm_f16x2_tile(g, 1 if out_f16x2 else 0, tile[0], tile[1], _stream()), "sm_gemm_f16x2_tile")
    res = c if (out is not None or split_k > 1 or batched) else c[0]
    return (res, xn if batched else xn[0]) if ln is not None else res


def w16_scale_exponent(w: torch.Tensor) -> int:
    """s such that max|w| * 2^s lies in [2^13, 2^14): the per-tensor scaling of the W16 weight format."""
    import math
    m = float(w.detach().abs().max())
    if not math.isfinite(m):
        raise ValueError("weight tensor holds non-finite values")
    if m == 0.0:
        return 0
    return 13 - math.floor(math.log2(m))


def split_w16(w: torch.Tensor):
    """fp32 weight (rows, K) -> (W16 tensor, w_scale = 2^-s): scaled hi / UNSCALED lo halves (gemm_w16.hip)."""
    _dev(w)
    w2 = w.reshape(w.shape[0], -1).contiguous()
    s = w16_scale_exponent(w2)
    out = torch.empty_like(w2)
    N.check(N.load().sm_split_w16(w2.data_ptr(), w2.stride(0), out.data_ptr(), out.stride(0), w2.shape[0], w2.shape[1],
                                  float(2.0 ** s), _stream()), "sm_split_w16")
    return out, float(2.0 ** -s)


def gemm_w16(a_split: torch.Tensor, w16: torch.Tensor, w_scale: float, bias=None, epilogue: int = N.EPI_BIAS, residual=None,
             variant: Optional[int] = None, out=None, out_f16x2: bool = False, split_k: int = 1, a_alt=None, alt_from_n: int = 0,
             patch_n: int = 0, xs_out=None, stats_out=None, ln_stats=None, ln_c=None, ln_eps: float = 0.0):
    """C = epilogue(A W^T + bias), A in F16X2, W in W16 (split_w16); single-accumulator kernel.  variant None = the
    library's pick for the shape.  Test / tuning entry: the forward drives the kernel from C."""
    _dev(a_split, w16, bias, residual, a_alt)
    M, K = a_split.shape
    Nn = w16.shape[0]
    c = out if out is not None else torch.empty((max(1, split_k), M, Nn), device=a_split.device, dtype=torch.float32)
    c3 = c if c.dim() == 3 else c.unsqueeze(0)
    g = N.GemmArgs()
    g.A, g.W, g.bias, g.C = a_split.data_ptr(), w16.data_ptr(), _ptr(bias), c3.data_ptr()
    g.strideC = c3.stride(0)
    g.M, g.N, g.K = M, Nn, K
    g.lda, g.ldw, g.ldc = a_split.stride(0), w16.stride(0), c3.stride(1)
    g.batch, g.epilogue, g.split_k, g.w_scale = 1, epilogue, split_k if split_k > 1 else 0, w_scale
    if a_alt is not None:
        g.A_alt, g.alt_from_n = a_alt.data_ptr(), alt_from_n
    if residual is not None:
        g.R, g.ldr = residual.data_ptr(), residual.stride(0)
    if epilogue == N.EPI_PATCH:
        g.patch_n = patch_n
    # LayerNorm folded into the GEMMs around it: producer outputs (F16X2 copy + row statistics) / consumer inputs (see the header)
    g.C2, g.ln_stats_out, g.ln_stats, g.ln_c, g.ln_eps = _ptr(xs_out), _ptr(stats_out), _ptr(ln_stats), _ptr(ln_c), ln_eps
    lib = N.load()
    if variant is None:
        N.check(lib.sm_gemm_w16(g, 1 if out_f16x2 else 0, _stream()), "sm_gemm_w16")
    else:
        N.check(lib.sm_gemm_w16_tile(g, 1 if out_f16x2 else 0, variant, _stream()), "sm_gemm_w16_tile")
    return c if (out is not None or split_k > 1) else c[0]


def layernorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float,
              add: Optional[torch.Tensor] = None, in_map=(0, 0, 0), out_map=(0, 0, 0), rows: Optional[int] = None,
              out_rows: Optional[int] = None):
    """y = LayerNorm(x) (+ optional y2 = y + add[r % len(add)]); optional grouped row remaps (see the header)."""
    _dev(x, gamma, beta, add)
    x2 = x.reshape(-1, x.shape[-1])
    assert x2.stride(1) == 1 and x2.shape[1] == N.EMBED
    rows = x2.shape[0] if rows is None else rows
    y = torch.empty((rows if out_rows is None else out_rows, N.EMBED), device=x.device, dtype=torch.float32)
    a = N.LnArgs()
    a.x, a.ldx, a.gamma, a.beta, a.y, a.ldy = x2.data_ptr(), x2.stride(0), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), N.EMBED
    a.in_map, a.out_map = N.RowMap(*in_map), N.RowMap(*out_map)
    a.rows, a.eps = rows, eps
    y2 = None
    if add is not None:
        add = add.contiguous()
        y2 = torch.empty((rows, N.EMBED), device=x.device, dtype=torch.float32)
        a.y2, a.ldy2, a.add, a.add_rows = y2.data_ptr(), N.EMBED, add.data_ptr(), add.shape[0]
    N.check(N.load().sm_layernorm_rows_f32(a, _stream()), "sm_layernorm_rows_f32")
    if in_map == (0, 0, 0) and out_map == (0, 0, 0):
        y = y.view(x.shape)
    return (y, y2) if add is not None else y


def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, scale: float = 0.125, split: bool = False) -> torch.Tensor:
    """q (B,Nq,H,64), k/v (B,Nk,H,64) views (last two dims contiguous) -> (B,Nq,H*64).
    split=True: the operands are first converted to F16X2 rows and sm_attention_f16x2 (f16 matrix cores) runs."""
    _dev(q, k, v)
    B, nq, H, dh = q.shape
    nk = k.shape[1]
    if split:  # F16X2 images of the (B, N, H*64) rows; the (B,N,H,64) view keeps float-unit strides
        q, k, v = (split_f16x2(t.reshape(t.shape[0], t.shape[1], H * dh).contiguous()).view(t.shape[0], t.shape[1], H, dh)
                   for t in (q, k, v))
    assert dh == 64 and q.stride(3) == 1 and q.stride(2) == 64 and k.stride(2) == 64 and v.stride(2) == 64
    o = torch.empty((B, nq, H * dh), device=q.device, dtype=torch.float32)
    a = N.AttnArgs()
    a.Q, a.K, a.V, a.O = q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr()
    a.sQb, a.sQr, a.sKb, a.sKr, a.sVb, a.sVr = q.stride(0), q.stride(1), k.stride(0), k.stride(1), v.stride(0), v.stride(1)
    a.sOb, a.sOr = o.stride(0), o.stride(1)
    a.batch, a.heads, a.n_q, a.n_k, a.scale = B, H, nq, nk, scale
    if split:
        N.check(N.load().sm_attention_f16x2(a, _stream()), "sm_attention_f16x2")
    else:
        N.check(N.load().sm_attention_f32(a, _stream()), "sm_attention_f32")
    return o


def attention_probs(q: torch.Tensor, k: torch.Tensor, scale: float = 0.125, q0: int = 0, nq: Optional[int] = None,
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The post-softmax attention matrix itself (vision_transformer.py:122-123): q (B,Nq,H,64), k (B,Nk,H,64) fp32 views (last two
    dims contiguous), converted to F16X2 rows here -> softmax(scale * q k^T) for the query rows [q0, q0 + nq) as (B,H,nq,Nk) fp32
    (sm_attention_probs_f16x2).  ``out``: a (B,H,nq,Nk) view to write into - contiguous per image, any stride between images."""
    _dev(q, k, out)
    B, n_q, H, dh = q.shape
    nk = k.shape[1]
    nq = n_q - q0 if nq is None else nq
    q, k = (split_f16x2(t.reshape(t.shape[0], t.shape[1], H * dh).contiguous()).view(t.shape[0], t.shape[1], H, dh) for t in (q, k))
    assert dh == 64 and q.stride(3) == 1 and q.stride(2) == 64 and k.stride(2) == 64
    p = out if out is not None else torch.empty((B, H, max(nq, 0), nk), device=q.device, dtype=torch.float32)
    assert tuple(p.shape) == (B, H, nq, nk) and (p.numel() == 0 or p[0].is_contiguous())
    a = N.AttnProbsArgs()
    a.Q, a.K, a.P = q.data_ptr(), k.data_ptr(), p.data_ptr()
    a.sQb, a.sQr, a.sKb, a.sKr, a.sPb = q.stride(0), q.stride(1), k.stride(0), k.stride(1), p.stride(0) if B > 1 else 0
    a.batch, a.heads, a.n_q, a.n_k, a.q0, a.nq, a.scale = B, H, n_q, nk, q0, nq, scale
    N.check(N.load().sm_attention_probs_f16x2(a, _stream()), "sm_attention_probs_f16x2")
    return p


def fold_layernorm(weight: torch.Tensor, bias: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor):
    """LayerNorm(gamma, beta) folded into the Linear(weight, bias) it feeds -> (W16 tensor of weight * gamma, its 2^-s, folded
    bias b + W beta, row sums c of the gain-scaled weight as rounded to W16): LN(x) W^T + b = r (x W'^T - mu c) + b'."""
    w16, ws = split_w16((weight * gamma[None, :]).contiguous())
    rows, K = weight.shape
    h = w16.view(torch.float16).reshape(rows, K // 8, 2, 8).double()
    c = ((h[:, :, 0, :] + h[:, :, 1, :]).reshape(rows, K).sum(1) * ws).float().contiguous()
    # (an elementwise product + row sum, not `@`: weight packing stays off the vendor BLAS - one-time per checkpoint, not timed)
    b2 = (bias.double() + (weight.double() * beta.double()[None, :]).sum(1)).float().contiguous()
    return w16, ws, b2, c


def qkv_attention(xn: torch.Tensor, w_qkv: torch.Tensor, b_qkv: torch.Tensor, B: int, scale: float = 0.125,
                  out_f16x2: bool = False, ln=None, xs: Optional[torch.Tensor] = None,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Fused qkv Linear + softmax attention of an encoder block (sm_qkv_attention_w16): xn (B*N, 384) fp32 LayerNorm output
    (converted to F16X2 here), w_qkv (1152, 384) / b_qkv (1152) fp32 -> (B*N, 384) merged-head attention output.
    ``xs``: the input already in F16X2 (then ``xn`` is not read and may be None) - a (B*N, 384) view whose row stride becomes
    ldx, e.g. a column slice of a wider buffer that starts at a multiple of 8 columns.  ``out``: a (B*N, 384) view to write
    into; its row stride becomes ldo.  The library checks strides and alignment."""
    _dev(xn, w_qkv, b_qkv, xs, out)
    if xs is None:
        xs = split_f16x2(xn.contiguous())
    M = xs.shape[0]
    assert M % B == 0 and xs.dim() == 2 and xs.shape[1] == N.EMBED and xs.stride(1) == 1
    o = out if out is not None else torch.empty((M, N.EMBED), device=xs.device, dtype=torch.float32)
    assert tuple(o.shape) == (M, N.EMBED) and o.stride(1) == 1
    a = N.QkvAttnArgs()
    if ln is not None:  # (gamma, beta, eps, stats): xn is then the RAW stream whose LayerNorm is folded into the projection
        gamma, beta, eps, stats = ln
        w16, ws, b2, cvec = fold_layernorm(w_qkv, b_qkv, gamma, beta)
        a.ln_stats, a.ln_c, a.ln_eps = stats.data_ptr(), cvec.data_ptr(), eps
        b_qkv = b2
    else:
        w16, ws = split_w16(w_qkv)
    a.Xn, a.Wqkv, a.bias, a.O = xs.data_ptr(), w16.data_ptr(), b_qkv.data_ptr(), o.data_ptr()
    a.ldx, a.ldo, a.B, a.N, a.w_scale, a.scale, a.out_f16x2 = xs.stride(0), o.stride(0), B, M // B, ws, scale, 1 if out_f16x2 else 0
    N.check(N.load().sm_qkv_attention_w16(a, _stream()), "sm_qkv_attention_w16")
    return o


def im2col_patches(img: torch.Tensor, patch: int) -> torch.Tensor:
    _dev(img)
    img = img.contiguous()
    B, _, H, W = img.shape
    gh, gw = -(-H // patch), -(-W // patch)
    cols = torch.empty((B * gh * gw, 3 * patch * patch), device=img.device, dtype=torch.float32)
    N.check(N.load().sm_im2col_patches_f32(img.data_ptr(), cols.data_ptr(), B, H, W, patch, _stream()), "sm_im2col")
    return cols


def pos_embed_bicubic(pos: torch.Tensor, gh: int, gw: int) -> torch.Tensor:
    _dev(pos)
    pos = pos.reshape(-1, N.EMBED).contiguous()
    g0 = int(round((pos.shape[0] - 1) ** 0.5))
    out = torch.empty((1 + gh * gw, N.EMBED), device=pos.device, dtype=torch.float32)
    N.check(N.load().sm_pos_embed_bicubic_f32(pos.data_ptr(), g0, out.data_ptr(), gh, gw, _stream()), "sm_pos_bicubic")
    return out


def upsample2x_tokens(tok: torch.Tensor, gh: int, gw: int) -> torch.Tensor:
    """tok (B, gh*gw, 384) -> (B, 4*gh*gw, 384), channels-last bilinear x2."""
    _dev(tok)
    assert tok.stride(2) == 1 and tok.stride(1) == N.EMBED
    B = tok.shape[0]
    up = torch.empty((B, 4 * gh * gw, N.EMBED), device=tok.device, dtype=torch.float32)
    N.check(N.load().sm_upsample2x_tokens_f32(tok.data_ptr(), tok.stride(0), up.data_ptr(), B, gh, gw, _stream()),
            "sm_upsample2x")
    return up


def rowdot_sigmoid(h: torch.Tensor, w: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    _dev(h, w, b)
    h2 = h.reshape(-1, N.EMBED).contiguous()
    out = torch.empty((h2.shape[0],), device=h.device, dtype=torch.float32)
    N.check(N.load().sm_rowdot_sigmoid_f32(h2.data_ptr(), w.data_ptr(), b.data_ptr(), out.data_ptr(), h2.shape[0],
                                           _stream()), "sm_rowdot_sigmoid")
    return out


_THRESHOLDS = {}


def f_max_thresholds(device) -> torch.Tensor:
    """The 255 strict thresholds of metrics/f_measure.py:65 as the float32 values torch.arange produces (constant)."""
    t = _THRESHOLDS.get(device)
    if t is None:
        t = torch.arange(0, 1, 1 / 255).to(device)
        assert t.numel() == 255 and t.dtype == torch.float32
        _THRESHOLDS[device] = t
    return t


class GtBatch:
    """Ground-truth masks of one batch packed for sm_evaluate_masks_f32: one uint8 buffer + a device descriptor
    array.  Build it once per batch (the evaluator's data loader side), reuse it across calls."""

    def __init__(self, gts, device):
        for g in gts:
            if g.dtype != torch.uint8 or g.dim() != 2:
                raise RuntimeError("ground-truth masks must be 2-D uint8 tensors")
        flat = [g.reshape(-1) for g in gts]
        self._build([tuple(g.shape) for g in gts], None, (flat[0] if len(gts) == 1 else torch.cat(flat)).to(device),
                    lambda table: torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(device))

    def _build(self, shapes, offsets, gt_all, images) -> "GtBatch":
        """The one builder: image b's (H, W) bytes at ``gt_all[offsets[b]:]`` (``offsets`` None: the planes lie end to end).  Fills the
        host sm_eval_image table (sm_sod_metrics_u8 checks it and sizes its grids from it), ``max_pixels`` and ``extent`` once;
        ``images`` is that table on the device, or the caller's way to bring the host table there."""
        self.shapes = [(int(h), int(w)) for h, w in shapes]
        self.B = len(self.shapes)
        if offsets is None:
            offsets = [sum(h * w for h, w in self.shapes[:b]) for b in range(self.B)]
        self.offsets = [int(o) for o in offsets]
        self.host = (N.EvalImage * self.B)()
        for e, (h, w), off in zip(self.host, self.shapes, self.offsets):
            e.gt_off, e.H, e.W = off, h, w
        self.max_pixels = max(h * w for h, w in self.shapes)
        self.extent = max(off + h * w for (h, w), off in zip(self.shapes, self.offsets))
        self.gt_all = gt_all
        self.images = images(self.host) if callable(images) else images
        return self

    @classmethod
    def from_packed(cls, packed, device) -> "GtBatch":
        """GtBatch from pipeline.pack_gts' page-locked buffers: two asynchronous H2D copies on the current stream."""
        from .pipeline import _POOL
        flat, descr, shapes = packed
        gb = cls.__new__(cls)._build(shapes, None, flat.to(device, non_blocking=True), descr.to(device, non_blocking=True))
        _POOL.release_after((flat, descr), torch.cuda.current_stream(device))
        return gb

    @classmethod
    def from_device(cls, flat: torch.Tensor, shapes, offsets) -> "GtBatch":
        """GtBatch over ground truth that is on the device already (``png_decode.decode_png_batch(mode="gt")``): image b's (H, W) bytes
        at ``flat[offsets[b]:]``; only the descriptors travel, through a page-locked buffer on the current stream."""
        from .pipeline import upload_tables
        if flat.dtype != torch.uint8 or flat.dim() != 1 or flat.device.type != "cuda":
            raise RuntimeError("GtBatch.from_device: a 1-D uint8 tensor on a HIP device")
        if len(shapes) == 0 or len(offsets) != len(shapes):
            raise ValueError("GtBatch.from_device: one offset per image, at least one image")
        for b, ((h, w), off) in enumerate(zip(shapes, offsets)):
            if off < 0 or off + h * w > flat.numel():
                raise ValueError(f"GtBatch.from_device: image {b} ({h} x {w} at {off}) lies outside the buffer of {flat.numel()} bytes")
        return cls.__new__(cls)._build(shapes, offsets, flat, lambda table: upload_tables([table], flat.device)[0][0])


def _last_layer(mask_pred_last: torch.Tensor):
    """-> B, nq, mh, mw of the last layer's masks as the kernels read them: dense per image, any batch stride
    (``out["mask_pred"][:, -1]``)"""
    B, nq, mh, mw = mask_pred_last.shape
    assert mask_pred_last.stride(3) == 1 and mask_pred_last.stride(2) == mw and mask_pred_last.stride(1) == mh * mw
    return B, nq, mh, mw


def _sel_col(which: str) -> int:
    """the column of evaluate_masks' rows that holds the picked ("pick") or the upper-bound ("ub") query's index"""
    if which not in ("pick", "ub"):
        raise ValueError(f'which={which!r}: "pick" or "ub"')
    return 14 if which == "pick" else 15


def _fits_upsampled(shapes, mh: int, mw: int, scale: float, what: str) -> None:
    """scale-factor mode crops the up-sampled mask to (H_b, W_b): no image may be larger than it"""
    if scale > 0:
        for (h, w) in shapes:
            assert h <= int(mh * scale) and w <= int(mw * scale), f"{what} larger than the up-sampled mask"


def evaluate_masks(mask_pred_last: torch.Tensor, objectness_last: torch.Tensor, gts, scale: float = 0.0,
                   return_ious: bool = False, extra: bool = False):
    """Evaluator post-processing + 14 metrics per image on the device (sm_evaluate_masks_f32).

    mask_pred_last (B, nq, mh, mw) probabilities (any batch stride, e.g. ``out["mask_pred"][:, -1]``),
    objectness_last (B, nq), gts: list of B uint8 {0,1} tensors (H_b, W_b) or a prepacked GtBatch.
    scale > 0: reference mode (F.interpolate(scale_factor=scale)[..., :H, :W]); 0: resize to each GT's size.
    Returns rows (B, 16) float32 [7 metrics of the picked mask, 7 of the upper bound, q*, ub] (+ ious (B, nq)).
    ``extra=True`` appends ``extra`` (B, 2, 4) float64 to the result: e_adp, e_mean, e_max, wfm (sod_metrics) of the picked and of
    the upper-bound query's 8-bit plane (upsample_selected_u8), as the same call up-sampled them."""
    _dev(mask_pred_last, objectness_last)
    B, nq, mh, mw = _last_layer(mask_pred_last)
    assert objectness_last.stride(1) == 1
    dev = mask_pred_last.device
    gb = gts if isinstance(gts, GtBatch) else GtBatch(gts, dev)
    assert gb.B == B
    _fits_upsampled(gb.shapes, mh, mw, scale, "GT")
    rows = torch.empty((B, 16), device=dev, dtype=torch.float32)
    ious = torch.empty((B, nq), device=dev, dtype=torch.float32) if return_ious else None
    lib = N.load()
    wsb = lib.sm_evaluate_workspace_bytes(B, nq, mh, mw, gb.max_pixels)
    if wsb == 0:
        raise ValueError("unsupported evaluate_masks shape")
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    a = N.EvalArgs()
    a.mask_pred, a.mask_stride_b = mask_pred_last.data_ptr(), mask_pred_last.stride(0)
    a.objectness, a.obj_stride_b = objectness_last.data_ptr(), objectness_last.stride(0)
    a.gt, a.images, a.thresholds = gb.gt_all.data_ptr(), gb.images.data_ptr(), f_max_thresholds(dev).data_ptr()
    a.rows, a.ious, a.workspace, a.workspace_bytes = rows.data_ptr(), _ptr(ious), ws.data_ptr(), wsb
    a.B, a.nq, a.mh, a.mw, a.scale = B, nq, mh, mw, float(scale)
    a.max_pixels = gb.max_pixels
    N.check(lib.sm_evaluate_masks_f32(a, _stream()), "sm_evaluate_masks_f32")
    if extra:
        ex = torch.stack([sod_metrics(upsample_selected_u8(mask_pred_last, rows, gb, scale, which), gb) for which in ("pick", "ub")],
                         dim=1)
        return (rows, ious, ex) if return_ious else (rows, ex)
    return (rows, ious) if return_ious else rows


def upsample_selected(mask_pred_last: torch.Tensor, rows: torch.Tensor, size, which: str = "pick") -> torch.Tensor:
    """(B, nq, mh, mw) probabilities + the (B, 16) rows of evaluate_masks -> (B, OH, OW) float64: the picked ("pick") or
    upper-bound ("ub") query's mask up-sampled bilinearly to ``size`` - the bilateral solver's target."""
    _dev(mask_pred_last, rows)
    B, nq, mh, mw = _last_layer(mask_pred_last)
    assert rows.shape == (B, 16) and rows.is_contiguous()
    out = torch.empty((B, size[0], size[1]), dtype=torch.float64, device=mask_pred_last.device)
    N.check(N.load().sm_upsample_selected_f64(mask_pred_last.data_ptr(), mask_pred_last.stride(0), rows.data_ptr(), _sel_col(which),
                                              out.data_ptr(), B, mh, mw, size[0], size[1], _stream()), "sm_upsample_selected_f64")
    return out


def mask_u8_to_f32(m: torch.Tensor) -> torch.Tensor:
    if not m.is_cuda or m.dtype != torch.uint8:
        raise RuntimeError("mask_u8_to_f32 takes a uint8 tensor on a HIP device")
    m = m.contiguous()
    out = torch.empty(m.shape, dtype=torch.float32, device=m.device)
    N.check(N.load().sm_mask_u8_to_f32(m.data_ptr(), out.data_ptr(), m.numel(), _stream()), "sm_mask_u8_to_f32")
    return out


def upsample_selected_native(mask_pred_last: torch.Tensor, rows: torch.Tensor, batch, scale: float, which: str = "pick") -> torch.Tensor:
    """Native resolution: image b's picked ("pick") or upper-bound ("ub") mask as the evaluator's reference mode up-samples it,
    F.interpolate(scale_factor=scale)[..., :H_b, :W_b], as float64 packed at ``batch.px_off`` (a bilateral_solver.MixedBatch) -
    the value evaluate_masks(..., scale=scale) scored for that image, and the target of the mixed-size bilateral solve."""
    _dev(mask_pred_last, rows)
    B, nq, mh, mw = _last_layer(mask_pred_last)
    assert rows.shape == (B, 16) and rows.is_contiguous() and batch.B == B and scale > 0
    _fits_upsampled(batch.shapes, mh, mw, scale, "image")
    out = torch.empty(batch.n_pixels, dtype=torch.float64, device=mask_pred_last.device)
    N.check(N.load().sm_upsample_selected_native_f64(mask_pred_last.data_ptr(), mask_pred_last.stride(0), rows.data_ptr(), _sel_col(which),
                                                     batch.dev.data_ptr(), out.data_ptr(), B, mh, mw, float(scale), batch.max_pixels,
                                                     _stream()), "sm_upsample_selected_native_f64")
    return out


def mask_planes_u8_to_f32(binary: torch.Tensor, batch) -> torch.Tensor:
    """Packed 0/1 planes of a MixedBatch -> (B, 1, Hmax, Wmax) float32, every image in the top-left corner of its zeroed plane: a
    one-query mask_pred that evaluate_masks(..., scale=1.0) crops back to (H_b, W_b)."""
    if not binary.is_cuda or binary.dtype != torch.uint8 or binary.numel() != batch.n_pixels:
        raise RuntimeError("mask_planes_u8_to_f32 takes the packed uint8 planes of the batch on a HIP device")
    Hm, Wm = max(h for h, _ in batch.shapes), max(w for _, w in batch.shapes)
    out = torch.zeros((batch.B, 1, Hm, Wm), dtype=torch.float32, device=binary.device)
    N.check(N.load().sm_mask_planes_u8_to_f32(binary.data_ptr(), batch.dev.data_ptr(), out.data_ptr(), batch.B, Hm, Wm,
                                              batch.max_pixels, _stream()), "sm_mask_planes_u8_to_f32")
    return out


def upsample_selected_u8(mask_pred_last: torch.Tensor, rows: torch.Tensor, gts: "GtBatch", scale: float = 0.0,
                         which: str = "pick") -> torch.Tensor:
    """The 8-bit plane E-measure and weighted F are defined on (sm_upsample_selected_u8): image b's picked ("pick") or upper-bound
    ("ub") query up-sampled as evaluate_masks(..., scale=scale) scored it, clipped to [0, 1], times 255, truncated - the
    predictor's ``soft`` bytes.  Returns a flat uint8 buffer with image b's (H_b, W_b) plane at ``gts.offsets[b]``, where the ground
    truth lies in ``gts.gt_all``."""
    _dev(mask_pred_last, rows)
    B, nq, mh, mw = _last_layer(mask_pred_last)
    assert rows.shape == (B, 16) and rows.is_contiguous() and gts.B == B
    _fits_upsampled(gts.shapes, mh, mw, scale, "GT")
    out = torch.empty(gts.extent, dtype=torch.uint8, device=mask_pred_last.device)
    N.check(N.load().sm_upsample_selected_u8(mask_pred_last.data_ptr(), mask_pred_last.stride(0), rows.data_ptr(), _sel_col(which),
                                             gts.images.data_ptr(), out.data_ptr(), B, mh, mw, float(scale), gts.max_pixels, _stream()),
            "sm_upsample_selected_u8")
    return out


def sod_metrics(pred_u8, gts, return_hist: bool = False):
    """E-measure and weighted F-measure per image on the device (sm_sod_metrics_u8; ``sod_metrics.py`` defines the values).

    ``pred_u8``: a list of B (H_b, W_b) uint8 device tensors (then ``gts`` may be a list of uint8 tensors of the same sizes or a
    GtBatch), or one flat uint8 buffer with image b's plane at ``gts.offsets[b]`` (``gts`` a GtBatch; what upsample_selected_u8
    returns).  Returns (B, 4) float64 on the device: e_adp, e_mean, e_max, wfm; with ``return_hist`` also the (B, 2, 256) int32
    histograms of the planes over foreground and background."""
    if isinstance(pred_u8, (list, tuple)):
        if not pred_u8:
            raise ValueError("an empty batch")
        dev = pred_u8[0].device
        gb = gts if isinstance(gts, GtBatch) else GtBatch(gts, dev)
        for p in pred_u8:
            if not p.is_cuda or p.dtype != torch.uint8 or p.dim() != 2:
                raise RuntimeError("sod_metrics takes 2-D uint8 planes on a HIP device (no CPU fallback)")
        if [tuple(p.shape) for p in pred_u8] != [tuple(s) for s in gb.shapes]:
            raise ValueError("prediction and ground-truth sizes differ")
        if all(o == sum(h * w for h, w in gb.shapes[:b]) for b, o in enumerate(gb.offsets)):
            flat = pred_u8[0].reshape(-1) if gb.B == 1 else torch.cat([p.reshape(-1) for p in pred_u8])
        else:
            flat = torch.empty(gb.extent, dtype=torch.uint8, device=dev)
            for p, o in zip(pred_u8, gb.offsets):
                flat[o:o + p.numel()] = p.reshape(-1)
    else:
        if not isinstance(gts, GtBatch):
            raise ValueError("a packed prediction buffer goes with a GtBatch")
        flat, gb = pred_u8, gts
        if not flat.is_cuda or flat.dtype != torch.uint8 or flat.dim() != 1 or not flat.is_contiguous():
            raise RuntimeError("sod_metrics takes a flat uint8 buffer on a HIP device (no CPU fallback)")
    dev = flat.device
    if flat.numel() < gb.extent or gb.gt_all.numel() < gb.extent or gb.gt_all.device != dev:
        raise ValueError("the prediction buffer (or the ground truth) is shorter than the batch's planes, or on another device")
    B, max_pixels = gb.B, gb.max_pixels
    lib = N.load()
    wsb = lib.sm_sod_metrics_workspace_bytes(B, max_pixels)
    if wsb == 0:
        raise ValueError("unsupported sod_metrics shape (1 <= H W <= 2^22 per image)")
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    out = torch.empty((B, 4), dtype=torch.float64, device=dev)
    hist = torch.empty((B, 2, 256), dtype=torch.int32, device=dev) if return_hist else None
    N.check(lib.sm_sod_metrics_u8(flat.data_ptr(), gb.gt_all.data_ptr(), gb.images.data_ptr(), ctypes.addressof(gb.host), B, max_pixels,
                                  out.data_ptr(), _ptr(hist), ws.data_ptr(), wsb, _stream()), "sm_sod_metrics_u8")
    return (out, hist) if return_hist else out


class PackedImages:
    """Descriptor table (sm_bilateral_image per image) of a batch whose images differ in size, for the predictor's finish: built on
    the host, uploaded with ONE asynchronous copy from page-locked memory on the current stream.  Per-pixel buffers are packed:
    image b's H*W values at ``px_off[b]``.  ``bilateral_solver.MixedBatch`` is this table plus the solver's workspace layout."""

    def __init__(self, shapes, device, img_offsets=None):
        from .pipeline import upload_tables
        B = len(shapes)
        if B == 0:
            raise ValueError("an empty batch")
        self.shapes = [(int(h), int(w)) for h, w in shapes]
        self.host = (N.BilateralImage * B)()
        io, po, self.px_off = 0, 0, []
        for b, (h, w) in enumerate(self.shapes):
            if h < 1 or w < 1:
                raise ValueError(f"image {b} is empty ({h} x {w})")
            e = self.host[b]
            e.img_off = int(img_offsets[b]) if img_offsets is not None else io
            e.px_off, e.H, e.W = po, h, w
            self.px_off.append(po)
            io += h * w * 3
            po += h * w
        self.B, self.n_pixels, self.max_pixels = B, po, max(h * w for h, w in self.shapes)
        self.img_bytes = max(self.host[b].img_off + h * w * 3 for b, (h, w) in enumerate(self.shapes))
        self._prepare()  # a subclass completes the host table (the solver's workspace offsets) before it is uploaded
        (self.dev,), _ = upload_tables([self.host], device)

    def _prepare(self) -> None:
        pass


class PendingPredictions:
    """The finish of one batch (``predict_masks``), queued on the current stream: ``result()`` waits for THAT batch's copies only.
    The inputs are kept for it - on overflow of ``cap`` the runs are found once more with room for the longest code - so the
    caller must not let the stream overwrite them (a replayed graph's static outputs) before asking."""

    def __init__(self, mask_pred_last, objectness_last, table, scale, rle, binary, soft, cap, objects=None, soft_png=False):
        import ctypes
        B, nq, mh, mw = mask_pred_last.shape
        dev = mask_pred_last.device
        self.table, self.cap, self._rle = table, int(cap), rle
        self.best = best = torch.empty(B, dtype=torch.int32, device=dev)
        self.binary = torch.empty(table.n_pixels, dtype=torch.uint8, device=dev) if binary else None
        self.soft = torch.empty(table.n_pixels, dtype=torch.uint8, device=dev) if soft or soft_png else None
        planes = (_ptr(self.binary), _ptr(self.soft))

        def launch(starts, info, cap, ws, first):  # the planes are written the first time only
            a = N.PredictArgs()
            a.masks, a.mask_stride_b = mask_pred_last.data_ptr(), mask_pred_last.stride(0)
            a.objectness, a.obj_stride_b = objectness_last.data_ptr(), objectness_last.stride(0)
            a.images, a.best = table.dev.data_ptr(), best.data_ptr()
            a.starts, a.info, a.cap = _ptr(starts), _ptr(info), cap
            a.binary, a.soft = planes if first else (None, None)
            a.workspace, a.workspace_bytes = _ptr(ws), 0 if ws is None else ws.numel()
            a.B, a.nq, a.mh, a.mw, a.max_pixels, a.scale = B, nq, mh, mw, table.max_pixels, float(scale)
            N.check(N.load().sm_predict_masks_f32(a, ctypes.addressof(table.host), torch.cuda.current_stream(dev).cuda_stream),
                    "sm_predict_masks_f32")

        self._runs = None
        if rle or objects is not None:  # the objects are found on the runs
            self._runs = PendingRuns(launch, table.shapes, self.cap, table.max_pixels, dev,
                                     objects and (table, objects, (mask_pred_last, best, float(scale))))
        else:
            launch(None, None, 0, None, True)
        # best and the planes in one page-locked buffer each
        self._host = {}
        for name, t in (("best", best), ("binary", self.binary), ("soft", self.soft if soft else None)):
            if t is not None:
                self._host[name] = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
                self._host[name].copy_(t, non_blocking=True)
        self._done = torch.cuda.Event()
        self._done.record(torch.cuda.current_stream(dev))
        # the soft maps as PNG files, encoded where they lie: their raw pixels stay on the device
        self._png = png_encode_async(packed=(self.soft, table.px_off, [(h, w, 1) for h, w in table.shapes])) if soft_png else None

    # the reader's device buffers and pending objects under the names they have on this class (None without runs)
    _starts = property(lambda self: getattr(self._runs, "_starts", None))
    _info = property(lambda self: getattr(self._runs, "_info", None))
    _objects = property(lambda self: getattr(self._runs, "_objects", None))

    def result(self) -> dict:
        """-> {"best": [query index], "rle": [COCO uncompressed RLE dict], "binary" / "soft": [(H_b, W_b) uint8 array], "soft_png":
        [the soft map as a PNG file, bytes], "objects": [the dict of ``_PendingObjects.result``]} (the keys asked for)"""
        self._done.synchronize()
        out = {"best": self._host["best"].tolist()}
        if self._runs is not None:
            rles, objects = self._runs.result(self._rle)
            out.update({k: v for k, v in (("rle", rles), ("objects", objects)) if v is not None})
        for name in ("binary", "soft"):
            if name in self._host:
                flat = self._host[name].numpy()
                out[name] = [flat[o:o + hh * ww].reshape(hh, ww) for o, (hh, ww) in zip(self.table.px_off, self.table.shapes)]
        if self._png is not None:
            out["soft_png"] = self._png.result()
        return out


def predict_masks(mask_pred_last: torch.Tensor, objectness_last: torch.Tensor, table, scale: float = 0.0, rle: bool = True,
                  binary: bool = False, soft: bool = False, cap: int = 8192, objects=None, soft_png: bool = False) -> PendingPredictions:
    """The predictor's fused finish (sm_predict_masks_f32), without waiting: mask_pred_last (B, nq, mh, mw) probabilities (any batch
    stride), objectness_last (B, nq), ``table`` a PackedImages / MixedBatch with the output size of every image.  The arg-max query's
    mask, up-sampled as ``evaluate_masks`` up-samples it (``scale`` as there), thresholded at 0.5: ``rle`` its COCO run-length code,
    ``binary`` / ``soft`` packed uint8 planes (0/1; clip(v, 0, 1) * 255 truncated).  ``.best`` (B,) int32 stays on the device.
    ``objects`` (an ``ObjectOptions`` or a dict of its keys): sm_mask_objects is queued right behind the runs and ``result()`` gains
    "objects" - per image the mask's connected components with box, area, centroid, score = the mean of the soft values, first raster
    pixel and, on request, an RLE each; ``None``: nothing more is launched.  ``soft_png``: the soft planes are encoded as 8-bit grey
    PNG files on the device (``png_encode_async`` on the packed planes) and ``result()`` gains "soft_png": one ``bytes`` per image."""
    _dev(mask_pred_last, objectness_last)
    B, nq, mh, mw = _last_layer(mask_pred_last)
    assert objectness_last.shape == (B, nq) and objectness_last.stride(1) == 1 and table.B == B
    return PendingPredictions(mask_pred_last, objectness_last, table, scale, rle, binary, soft, max(1, min(int(cap), table.max_pixels)),
                              ObjectOptions.of(objects), soft_png)


class PendingPackedRuns(PendingRuns):
    """``rle_runs_packed_async``'s reader: ``result()`` -> one dict per image, or (those, the objects per image) when asked for them"""

    def result(self):
        rles, objects = super().result()
        return rles if objects is None else (rles, objects)


def rle_runs_packed_async(planes: torch.Tensor, table, cap: int = 8192, objects=None) -> PendingPackedRuns:
    """Packed 0/1 uint8 planes (image b's H_b x W_b bytes at ``table.px_off[b]`` - the mixed bilateral solver's binary output) ->
    their run-length codes, without waiting (``.result()``): ``voting.rle_runs_async`` for images of different sizes.  With
    ``objects`` (as ``predict_masks``) ``result()`` is (codes, objects per image); a plane has no soft values, so ``score`` is None."""
    import ctypes
    if not planes.is_cuda or planes.dtype != torch.uint8 or not planes.is_contiguous() or planes.numel() < table.n_pixels:
        raise RuntimeError("rle_runs_packed_async takes the packed uint8 planes of the batch on a HIP device (no CPU fallback)")

    def launch(starts, info, cap, ws, first):
        N.check(N.load().sm_rle_runs_packed_u8(planes.data_ptr(), table.dev.data_ptr(), ctypes.addressof(table.host), table.B,
                                               starts.data_ptr(), cap, info.data_ptr(), ws.data_ptr(), ws.numel(),
                                               torch.cuda.current_stream(planes.device).cuda_stream), "sm_rle_runs_packed_u8")

    opts = ObjectOptions.of(objects)
    return PendingPackedRuns(launch, table.shapes, max(1, min(int(cap), table.max_pixels)), table.max_pixels, planes.device,
                             opts and (table, opts, None))


# ---- the serving response's images: resized 8-bit mask + heat map (csrc/present.hip) ---------------------------------------------------
_PRESENT_TABLES = {}   # (device, mh, mw, ((H, W, img_off), ...)) -> _PresentTables, the most recent _TABLES_MAX kept
_TABLES_MAX = 64
_PRESENT_LUT = {}


def _recent(cache: dict, key, make):
    """``cache[key]``, made on first use, as the most recently used of the _TABLES_MAX entries the cache keeps"""
    t = cache.pop(key, None)
    if t is None:
        t = make()
    cache[key] = t  # most recently used last
    while len(cache) > _TABLES_MAX:
        cache.pop(next(iter(cache)))
    return t


class _PresentTables:
    """Descriptor and tap tables of one batch of sizes, on the host and on the device (uploaded once through the pinned pool; ``ready``
    orders another stream's first use behind that upload).  Image b's pixels start at ``px_off[b]``, a multiple of 4."""

    def __init__(self, mh, mw, items, device):
        from .pipeline import upload_tables
        from .resample import CoefTable
        B = len(items)
        self.host = (N.PresentImage * B)()
        table, po, self.px_off = CoefTable("lanczos"), 0, []
        for b, (h, w, img_off) in enumerate(items):
            if h < 1 or w < 1 or h * w > N.PRESENT_MAX_PIXELS:
                raise ValueError(f"image {b} is {h} x {w} (1 .. {N.PRESENT_MAX_PIXELS} pixels)")
            d = self.host[b]
            d.img_off, d.px_off, d.H, d.W = img_off, po, h, w
            self.px_off.append(po)
            po += (h * w + 3) & ~3
            # a pass between equal lengths is skipped: ks = 0
            d.coef_x, d.ksx = table.add(mw, w) if w != mw else (0, 0)
            d.coef_y, d.ksy = table.add(mh, h) if h != mh else (0, 0)
        self.B, self.n_pixels, self.max_w = B, po, max(w for _, w, _ in items)
        self.shapes = [(h, w) for h, w, _ in items]
        (self.coef, self.dev), self.ready = upload_tables([table.array(), self.host], device)


def _present_tables(mh, mw, items, device) -> _PresentTables:
    return _recent(_PRESENT_TABLES, (device, mh, mw, tuple(items)), lambda: _PresentTables(mh, mw, items, device))


def _present_lut(device) -> torch.Tensor:
    t = _PRESENT_LUT.get(device)
    if t is None:
        from .present import JET_RGBA
        t = _PRESENT_LUT[device] = torch.from_numpy(JET_RGBA.copy()).to(device)
    return t


class PendingPresent:
    """``present_masks_async``'s launches and (``host=True``) their one device-to-host copy, queued on the current stream;
    ``result()`` waits for that copy alone and hands out per image ``(mask (H, W) uint8 | None, heat map (H, W, 4) uint8 | None)`` -
    numpy views of one page-locked buffer, or views of the device buffer."""

    def __init__(self, tables, dev_buf, host_buf, heat_at, want_mask, want_heat, keep):
        self.tables, self.dev_buf, self.host_buf, self.heat_at = tables, dev_buf, host_buf, heat_at
        self.want_mask, self.want_heat = want_mask, want_heat
        self._keep = keep  # inputs of the queued kernels
        self.done = None
        if host_buf is not None:
            self.done = torch.cuda.Event()
            self.done.record(torch.cuda.current_stream(dev_buf.device))

    def result(self):
        if self.done is not None:
            self.done.synchronize()
            self._keep = None
        buf = self.host_buf.numpy() if self.host_buf is not None else self.dev_buf
        out = []
        for (h, w), po in zip(self.tables.shapes, self.tables.px_off):
            m = buf[po:po + h * w].reshape(h, w) if self.want_mask else None
            a = self.heat_at + 4 * po
            out.append((m, buf[a:a + 4 * h * w].reshape(h, w, 4) if self.want_heat else None))
        return out


def present_masks_async(masks: torch.Tensor, images, packed=None, want_mask: bool = True, want_heat: bool = True, host: bool = True,
                        alpha: float = 0.5, brightness: float = 1.1, lut: Optional[torch.Tensor] = None) -> PendingPresent:
    """The response's two images for B selected masks: ``masks`` (B, mh, mw) float32 in [0, 1] on the device; ``images`` a list of
    (H, W, 3) uint8 arrays (packed and uploaded here through the pinned pool), or - ``packed=(pixel buffer on the device, byte offset of
    every image in it)``, what the input pipeline uploaded already - anything that carries their (H, W).  Image b's mask is resized to
    its (H, W) as Pillow's LANCZOS does; the heat map is ``lut`` (256 x 4 uint8 on the device; default: jet) of it, blended with the
    upload and brightened.  ``host``: one device-to-host copy of both outputs into page-locked memory.  Sizes seen before reuse their
    descriptor and tap tables on the device."""
    import numpy as np
    from .pipeline import _POOL, packed_pixel_offsets
    if not masks.is_cuda or masks.dtype != torch.float32 or masks.dim() != 3 or masks[0].numel() and not masks[0].is_contiguous():
        raise RuntimeError("present_masks needs a (B, mh, mw) float32 tensor on a HIP device whose masks are contiguous (no CPU fallback)")
    if not (want_mask or want_heat):
        raise ValueError("present_masks: neither the mask nor the heat map asked for")
    device, (B, mh, mw) = masks.device, masks.shape
    shapes = [tuple(int(v) for v in (im.shape[:2] if hasattr(im, "shape") else im[:2])) for im in images]
    if len(shapes) != B:
        raise ValueError(f"{B} masks for {len(shapes)} images")
    st = torch.cuda.current_stream(device)
    keep = [masks]
    if packed is not None:
        pixels, offs = packed
        if not pixels.is_cuda or pixels.dtype != torch.uint8:
            raise RuntimeError("present_masks: packed pixels are a uint8 buffer on the HIP device")
    elif want_heat:
        offs = packed_pixel_offsets(shapes)
        staging = _POOL.get(offs[-1] + shapes[-1][0] * shapes[-1][1] * 3, torch.uint8)
        sv = staging.numpy()
        for im, (h, w), o in zip(images, shapes, offs):
            assert im.dtype == np.uint8 and im.shape == (h, w, 3), "uploads must be (H, W, 3) uint8"
            sv[o:o + h * w * 3] = im.reshape(-1)
        pixels = staging.to(device, non_blocking=True)
        _POOL.release_after((staging,), st)
    else:
        pixels, offs = None, [0] * B
    for (h, w), o in zip(shapes, offs):
        if want_heat and (o < 0 or o + h * w * 3 > pixels.numel()):
            raise ValueError("present_masks: an image lies outside the pixel buffer")
    t = _present_tables(mh, mw, tuple((h, w, int(o)) for (h, w), o in zip(shapes, offs)), device)
    st.wait_event(t.ready)
    heat_at = (t.n_pixels + 15) & ~15 if want_mask else 0
    dev_buf = torch.empty(heat_at + (4 * t.n_pixels if want_heat else 0), dtype=torch.uint8, device=device)
    lib = N.load()
    ws_bytes = lib.sm_present_workspace_bytes(B, mh, t.max_w)
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=device)
    lut = _present_lut(device) if lut is None else lut
    N.check(lib.sm_present_masks_u8(masks.data_ptr(), masks.stride(0), mh, mw, _ptr(pixels), t.host, t.dev.data_ptr(), t.coef.data_ptr(),
                                    lut.data_ptr(), alpha, brightness, dev_buf.data_ptr() if want_mask else None,
                                    dev_buf[heat_at:].data_ptr() if want_heat else None, ws.data_ptr(), ws_bytes, B, st.cuda_stream),
            "sm_present_masks_u8")
    host_buf = None
    if host:
        host_buf = torch.empty(dev_buf.numel(), dtype=torch.uint8, pin_memory=True)
        host_buf.copy_(dev_buf, non_blocking=True)
    return PendingPresent(t, dev_buf, host_buf, heat_at, want_mask, want_heat, keep + [pixels, ws, lut])


def present_masks(masks: torch.Tensor, images, **kw):
    """``present_masks_async(...).result()``: per image ``(mask (H, W) uint8, heat map (H, W, 4) uint8)``."""
    return present_masks_async(masks, images, **kw).result()


# ---- PNG files of images that are on the device (csrc/png.hip; the format: selfmask_amd/png.py) ---------------------------------------
_PNG_TABLES = {}   # (device, ((H, W, C, pix_off), ...), filter_mode) -> _PngTables, the most recent _TABLES_MAX kept


class _PngTables:
    """Descriptor table of one batch of shapes on the host and on the device (uploaded once through the pinned pool; ``ready`` orders
    another stream's first use behind that upload).  Image b's file goes to ``out_off[b]`` (a multiple of 16) with ``cap[b]`` =
    ``sm_png_bound`` bytes of room."""

    def __init__(self, items, filter_mode, device):
        from .pipeline import upload_tables
        lib = N.load()
        B = len(items)
        self.host = (N.PngImage * B)()
        self.out_off, self.cap, oo = [], [], 0
        for b, (h, w, c, pix_off) in enumerate(items):
            cap = lib.sm_png_bound(h, w, c)
            if not cap:
                raise ValueError(f"png_encode: image {b} is {h} x {w} x {c} (1, 3 or 4 channels, at most 2^24 pixels)")
            d = self.host[b]
            d.pix_off, d.out_off, d.out_cap, d.H, d.W, d.channels, d.filter_mode = pix_off, oo, cap, h, w, c, filter_mode
            self.out_off.append(oo)
            self.cap.append(cap)
            oo += (cap + 15) & ~15
        self.B, self.out_bytes = B, oo
        self.ws_bytes = lib.sm_png_workspace_bytes(self.host, B)
        (self.dev,), self.ready = upload_tables([self.host], device)


def _png_tables(items, filter_mode, device) -> _PngTables:
    return _recent(_PNG_TABLES, (device, tuple(items), filter_mode), lambda: _PngTables(items, filter_mode, device))


class PendingPng:
    """``png_encode_async``'s launches and the copy of the files' sizes, queued on the current stream.  ``result()`` waits for the sizes,
    copies exactly the used bytes of every file into page-locked memory on the same stream and hands out one ``bytes`` per image."""

    def __init__(self, tables, out, sizes, stream, keep):
        self.tables, self.out, self.stream, self._keep = tables, out, stream, keep
        self.sizes_host = torch.empty(tables.B, dtype=torch.int64, pin_memory=True)
        self.sizes_host.copy_(sizes, non_blocking=True)
        self.done = torch.cuda.Event()
        self.done.record(stream)

    def result(self):
        self.done.synchronize()
        t = self.tables
        sizes = [int(v) for v in self.sizes_host.tolist()]
        for b, n in enumerate(sizes):
            if not 0 < n <= t.cap[b]:
                raise RuntimeError(f"png_encode: image {b} reports {n} bytes (bound {t.cap[b]})")
        host = torch.empty(sum(sizes), dtype=torch.uint8, pin_memory=True)
        at = 0
        with torch.cuda.stream(self.stream):
            for b, n in enumerate(sizes):
                host[at:at + n].copy_(self.out[t.out_off[b]:t.out_off[b] + n], non_blocking=True)
                at += n
        self.stream.synchronize()
        self._keep = None
        flat, files, at = host.numpy(), [], 0
        for n in sizes:
            files.append(flat[at:at + n].tobytes())
            at += n
        return files


def png_encode_async(buffers=None, packed=None, filter_mode: int = -1) -> PendingPng:
    """PNG files of images in device memory: ``buffers`` a list of contiguous uint8 device tensors (H, W), (H, W, 3) or (H, W, 4) - packed
    into one buffer here by one device-to-device copy - or ``packed=(uint8 device buffer, byte offset of every image in it, their
    (H, W, C))``, which is used where it lies.  The bytes are those of ``png.encode_reference``; any PNG reader gives the pixels back.
    Shape sets seen before reuse their descriptor table on the device."""
    if packed is not None:
        pixels, offs, shapes = packed
        shapes = [tuple(int(v) for v in s) for s in shapes]
    else:
        if not buffers:
            raise ValueError("png_encode: no images")
        for tns in buffers:
            if not (torch.is_tensor(tns) and tns.is_cuda and tns.dtype == torch.uint8 and tns.is_contiguous() and tns.dim() in (2, 3)):
                raise RuntimeError("png_encode needs contiguous uint8 tensors on a HIP device (no CPU fallback)")
        shapes = [(t.shape[0], t.shape[1], 1 if t.dim() == 2 else t.shape[2]) for t in buffers]
        offs, o = [], 0
        for h, w, c in shapes:
            offs.append(o)
            o += h * w * c
        pixels = torch.cat([t.reshape(-1) for t in buffers]) if len(buffers) > 1 else buffers[0].reshape(-1)
    if not pixels.is_cuda or pixels.dtype != torch.uint8 or not pixels.is_contiguous():
        raise RuntimeError("png_encode: packed pixels are a contiguous uint8 buffer on the HIP device (no CPU fallback)")
    if len(shapes) != len(offs):
        raise ValueError(f"png_encode: {len(offs)} offsets for {len(shapes)} shapes")
    for (h, w, c), o in zip(shapes, offs):
        if o < 0 or o + h * w * c > pixels.numel():
            raise ValueError("png_encode: an image lies outside the pixel buffer")
    device = pixels.device
    st = torch.cuda.current_stream(device)
    t = _png_tables(tuple((h, w, c, int(o)) for (h, w, c), o in zip(shapes, offs)), int(filter_mode), device)
    st.wait_event(t.ready)
    out = torch.empty(t.out_bytes, dtype=torch.uint8, device=device)
    sizes = torch.empty(t.B, dtype=torch.int64, device=device)
    ws = torch.empty(max(t.ws_bytes, 1), dtype=torch.uint8, device=device)
    N.check(N.load().sm_png_encode_batch_u8(pixels.data_ptr(), t.host, t.dev.data_ptr(), t.B, out.data_ptr(), sizes.data_ptr(), ws.data_ptr(),
                                            t.ws_bytes, st.cuda_stream), "sm_png_encode_batch_u8")
    return PendingPng(t, out, sizes, st, [pixels, ws, sizes])


def png_encode(buffers=None, **kw):
    """``png_encode_async(...).result()``: one ``bytes`` (a PNG file) per image."""
    return png_encode_async(buffers, **kw).result()
