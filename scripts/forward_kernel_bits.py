"""Digests of direct calls of the forward's own kernels, for A/B runs of two builds of the library that must agree bit for bit (a
change of csrc/layernorm.hip, gemm.hip, gemm_f16x2.hip, gemm_w16.hip, qkv_attention.hip, attention_f16x2.hip or attention_probs.hip
that moves no arithmetic).  scripts/forward_bits.py covers whole forwards; this covers the entry points at shapes a forward does not
reach: single rows, tiles with dead rows, key counts at every chunk and block edge, every epilogue.

Runs a fixed, seeded case list on the library that SM_HIP_LIB names (default: lib/libselfmask_hip.so) and prints ONE JSON object
{case: sha256 of the bytes of every output}.  Outputs start as zeros, so rows a launch leaves alone hash the same.  Run it once per
library, each in a fresh process, and compare (profiles/forward_kernel_bits_parent.json: the object of the commit before the shared
pieces of csrc/forward_pieces.h and csrc/attention_split.h):

    SM_HIP_LIB=$PWD/salient-object-detection_amd/lib/libselfmask_hip_prev.so python scripts/forward_kernel_bits.py --out prev.json
    python scripts/forward_kernel_bits.py --out new.json
"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(ROOT, "salient-object-detection_amd"))

import torch  # noqa: E402
from selfmask_amd import _native as N, ops  # noqa: E402

DEV = "cuda:0"
D = N.EMBED
EPIS = {"bias": N.EPI_BIAS, "gelu": N.EPI_GELU, "relu": N.EPI_RELU, "residual": N.EPI_RESIDUAL, "sigmoid2": N.EPI_SIGMOID2,
        "patch": N.EPI_PATCH}
GEMM_SHAPES = [(33, 64, 32), (300, 384, 1536)]  # M, N, K
F16X2_TILES = [(64, 384), (256, 128), (256, 64), (128, 128), (128, 64), (64, 64)]
KEY_COUNTS = [1, 31, 32, 33, 63, 64, 65, 96, 128, 197]
QUERY_COUNTS = [1, 33, 129]
PROBS_RANGES = {1: [(0, 1)], 33: [(0, 33), (1, 32), (32, 1)], 129: [(0, 129), (32, 40), (5, 1), (100, 29)]}  # (q0, nq) by n_q


def _rand(gen, *shape, scale=1.0):
    return (torch.randn(*shape, generator=gen) * scale).to(DEV)


def _zeros(*shape):
    return torch.zeros(*shape, device=DEV, dtype=torch.float32)


def _p(t):
    return None if t is None else t.data_ptr()


def _sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


# ---- LayerNorm ---------------------------------------------------------------------------------------------------------------------
def _ln(x, gamma, beta, eps, rows, **kw):
    a = N.LnArgs()
    a.x, a.ldx, a.gamma, a.beta, a.rows, a.eps = x.data_ptr(), kw.get("ldx", D), gamma.data_ptr(), beta.data_ptr(), rows, eps
    a.in_map, a.out_map = N.RowMap(*kw.get("in_map", (0, 0, 0))), N.RowMap(*kw.get("out_map", (0, 0, 0)))
    a.y, a.ys, a.ldy, a.y2, a.ldy2 = _p(kw.get("y")), _p(kw.get("ys")), D, _p(kw.get("y2")), D
    add = kw.get("add")
    a.add, a.add_rows, a.y2_f16x2 = _p(add), 0 if add is None else add.shape[0], 1 if kw.get("y2_f16x2") else 0
    a.n_partials, a.partial_stride = kw.get("parts", 0), kw.get("partial_stride", 0)
    a.pre_bias, a.residual, a.raw = _p(kw.get("pre_bias")), _p(kw.get("residual")), _p(kw.get("raw"))
    chain = kw.get("chain")
    if chain is not None:
        a.chain_gamma, a.chain_beta, a.chain_eps = chain["gamma"].data_ptr(), chain["beta"].data_ptr(), chain["eps"]
        a.chain_y, a.chain_ys, a.chain_ldy = chain["y"].data_ptr(), chain["ys"].data_ptr(), D
    N.check(N.load().sm_layernorm_rows_f32(a, ops._stream()), "sm_layernorm_rows_f32")


def layernorm_cases(res):
    for rows in (1, 5, 17, 394):
        g = torch.Generator().manual_seed(1000 + rows)
        x = _rand(g, rows, D, scale=1.5) + _rand(g, rows, 1)
        gm, bt, gm2, bt2 = 1 + _rand(g, D, scale=0.1), _rand(g, D, scale=0.1), 1 + _rand(g, D, scale=0.1), _rand(g, D, scale=0.1)
        add = _rand(g, 3, D)
        y, ys = _zeros(rows, D), _zeros(rows, D)
        _ln(x, gm, bt, 1e-6, rows, y=y, ys=ys)
        res[f"layernorm|{rows}|plain"] = _sha(y, ys)
        y, y2 = _zeros(rows, D), _zeros(rows, D)
        _ln(x, gm, bt, 1e-5, rows, y=y, y2=y2, add=add)
        res[f"layernorm|{rows}|add"] = _sha(y, y2)
        groups = (rows + 3) // 4  # rows in groups of 4: read at stride 6 from row 1, written at stride 5
        xm, ym = _rand(g, groups * 6 + 1, D), _zeros(groups * 5, D)
        _ln(xm, gm, bt, 1e-6, rows, y=ym, in_map=(4, 6, 1), out_map=(4, 5, 0))
        res[f"layernorm|{rows}|row_maps"] = _sha(ym)
        y, ys, cy, cys = (_zeros(rows, D) for _ in range(4))
        _ln(x, gm, bt, 1e-6, rows, y=y, ys=ys, chain=dict(gamma=gm2, beta=bt2, eps=1e-5, y=cy, ys=cys))
        res[f"layernorm|{rows}|chain"] = _sha(y, ys, cy, cys)
        parts, stream, ys, y2 = _rand(g, 4, rows, D), _rand(g, rows, D), _zeros(rows, D), _zeros(rows, D)
        _ln(parts, gm, bt, 1e-5, rows, ys=ys, y2=y2, add=add, y2_f16x2=True, parts=4, partial_stride=rows * D, pre_bias=bt2,
            residual=stream, raw=stream)
        res[f"layernorm|{rows}|partials"] = _sha(stream, ys, y2)


# ---- gemm / gemm_f16x2 -------------------------------------------------------------------------------------------------------------
def _gemm(f16x2, a, w, bias, epi, M, Nn, K, *, tile=None, out_f16x2=False, split_k=1, ln=None, gen=None):
    """one launch of sm_gemm_f32(_tile) / sm_gemm_f16x2_tile on 2-D or batched 3-D operands; returns every output"""
    a3, w3 = (t if t.dim() == 3 else t.unsqueeze(0) for t in (a, w))
    nb = a3.shape[0]
    patch_n = M // 3 if epi == N.EPI_PATCH else 0  # PATCH: three images of M // 3 patches (both M are multiples of 3)
    c = _zeros(max(nb, split_k), M + 3 if patch_n else M, Nn)
    g = N.GemmArgs()
    g.A, g.W, g.bias, g.C = a3.data_ptr(), w3.data_ptr(), _p(bias), c.data_ptr()
    g.strideA, g.strideW, g.strideC = a3.stride(0) if nb > 1 else 0, w3.stride(0) if nb > 1 else 0, c.stride(0)
    g.M, g.N, g.K, g.lda, g.ldw, g.ldc = M, Nn, K, a3.stride(1), w3.stride(1), c.stride(1)
    g.batch, g.epilogue, g.split_k, g.patch_n = nb, epi, split_k if split_k > 1 else 0, patch_n
    outs = [c]
    if epi == N.EPI_RESIDUAL or ln is not None:
        r = _rand(gen, nb, M, Nn)
        g.R, g.ldr, g.strideR = r.data_ptr(), r.stride(1), r.stride(0)
    if epi == N.EPI_PATCH:
        r = _rand(gen, patch_n + 1, Nn)
        g.R, g.ldr = r.data_ptr(), r.stride(0)
    if epi == N.EPI_SIGMOID2 or ln is not None:
        outs.append(_zeros(*c.shape))
        g.C2 = outs[1].data_ptr()
    if ln is not None:
        g.epilogue, g.ln_gamma, g.ln_beta, g.ln_eps = N.EPI_RESIDUAL_LN, ln[0].data_ptr(), ln[1].data_ptr(), ln[2]
    lib = N.load()
    if f16x2:
        N.check(lib.sm_gemm_f16x2_tile(g, 1 if out_f16x2 else 0, tile[0], tile[1], ops._stream()), "sm_gemm_f16x2_tile")
    elif tile is None:
        N.check(lib.sm_gemm_f32(g, ops._stream()), "sm_gemm_f32")
    else:
        N.check(lib.sm_gemm_f32_tile(g, tile[0], tile[1], ops._stream()), "sm_gemm_f32_tile")
    return outs


def gemm_cases(res):
    for M, Nn, K in GEMM_SHAPES:
        g = torch.Generator().manual_seed(2000 + M)
        a, w, b = _rand(g, M, K), _rand(g, Nn, K, scale=0.05), _rand(g, Nn, scale=0.1)
        a_s, w_s = ops.split_f16x2(a), ops.split_f16x2(w)
        for name, epi in EPIS.items():
            res[f"gemm|{M}x{Nn}x{K}|{name}"] = _sha(*_gemm(False, a, w, b, epi, M, Nn, K, gen=g))
            res[f"gemm_f16x2|{M}x{Nn}x{K}|{name}"] = _sha(*_gemm(True, a_s, w_s, b, epi, M, Nn, K, tile=(128, 128), gen=g))
        for name in ("bias", "gelu", "relu"):
            res[f"gemm_f16x2|{M}x{Nn}x{K}|{name}|f16x2_out"] = _sha(*_gemm(True, a_s, w_s, b, EPIS[name], M, Nn, K, tile=(128, 128),
                                                                           out_f16x2=True))
        for tile in ((128, 128), (128, 64), (64, 64)):
            res[f"gemm|{M}x{Nn}x{K}|tile{tile[0]}x{tile[1]}"] = _sha(*_gemm(False, a, w, b, N.EPI_BIAS, M, Nn, K, tile=tile))
        for tile in F16X2_TILES:
            res[f"gemm_f16x2|{M}x{Nn}x{K}|tile{tile[0]}x{tile[1]}"] = _sha(*_gemm(True, a_s, w_s, b, N.EPI_BIAS, M, Nn, K, tile=tile))
        ab, wb = _rand(g, 2, M, K), _rand(g, 2, Nn, K, scale=0.05)
        res[f"gemm|{M}x{Nn}x{K}|batched"] = _sha(*_gemm(False, ab, wb, b, N.EPI_BIAS, M, Nn, K))
        res[f"gemm_f16x2|{M}x{Nn}x{K}|batched"] = _sha(*_gemm(True, ops.split_f16x2(ab), ops.split_f16x2(wb), b, N.EPI_GELU, M, Nn, K,
                                                              tile=(128, 64)))
    M, Nn, K = GEMM_SHAPES[1]
    res["gemm|split_k4"] = _sha(*_gemm(False, a, w, None, N.EPI_BIAS, M, Nn, K, split_k=4))
    res["gemm_f16x2|split_k4"] = _sha(*_gemm(True, a_s, w_s, None, N.EPI_BIAS, M, Nn, K, tile=(128, 64), split_k=4))
    for M in (1, 63, 130):  # the LayerNorm epilogue on the full-row tile
        g = torch.Generator().manual_seed(2100 + M)
        a_s, w_s = ops.split_f16x2(_rand(g, M, D)), ops.split_f16x2(_rand(g, D, D, scale=0.05))
        ln = (1 + _rand(g, D, scale=0.1), _rand(g, D, scale=0.1), 1e-6)
        res[f"gemm_f16x2|ln|{M}"] = _sha(*_gemm(True, a_s, w_s, _rand(g, D, scale=0.1), N.EPI_RESIDUAL, M, D, D, tile=(64, 384), ln=ln, gen=g))


# ---- gemm_w16 with the folded LayerNorm, the fused QKV + attention kernel -------------------------------------------------------
def _segment_stats(x):
    seg = x.reshape(x.shape[0], 12, 32)
    mean = seg.mean(2)
    return torch.stack([mean, ((seg - mean[..., None]) ** 2).sum(2)], dim=2).contiguous()


def w16_cases(res):
    for M in (1, 255, 394):
        g = torch.Generator().manual_seed(3000 + M)
        a, w, b, r = _rand(g, M, D), _rand(g, D, D, scale=0.05), _rand(g, D, scale=0.1), _rand(g, M, D, scale=2.0) + _rand(g, M, 1)
        w16, ws = ops.split_w16(w)
        xs, stats, x = _zeros(M, D), _zeros(M, 12, 2), _zeros(M, D)
        ops.gemm_w16(ops.split_f16x2(a), w16, ws, b, epilogue=N.EPI_RESIDUAL, residual=r, variant=47, out=x, xs_out=xs, stats_out=stats)
        res[f"gemm_w16|{M}|stats_out"] = _sha(x, xs, stats)
        fw, fs, fb, fc = ops.fold_layernorm(_rand(g, 768, D, scale=0.05), _rand(g, 768, scale=0.1), torch.rand(D, generator=g).to(DEV) + 0.5,
                                            _rand(g, D, scale=0.2))
        for variant in (47, 42, 44, 45):
            y = _zeros(M, 768)
            ops.gemm_w16(xs, fw, fs, fb, epilogue=N.EPI_GELU, variant=variant, out=y, out_f16x2=True, ln_stats=stats, ln_c=fc, ln_eps=1e-6)
            res[f"gemm_w16|{M}|ln_stats|v{variant}"] = _sha(y)


def qkv_cases(res):
    for n in (1, 17, 197, 208):
        for B in (1, 3):
            g = torch.Generator().manual_seed(4000 + 10 * n + B)
            x = _rand(g, B * n, D, scale=1.5) + _rand(g, B * n, 1, scale=0.5)
            w, b = _rand(g, 3 * D, D, scale=0.05), _rand(g, 3 * D, scale=0.1)
            gamma, beta = torch.rand(D, generator=g).to(DEV) + 0.5, _rand(g, D, scale=0.2)
            res[f"qkv_attention|N{n}|B{B}|plain"] = _sha(ops.qkv_attention(x, w, b, B, 0.125))
            res[f"qkv_attention|N{n}|B{B}|ln"] = _sha(ops.qkv_attention(x, w, b, B, 0.125, ln=(gamma, beta, 1e-6, _segment_stats(x))))


# ---- split-operand attention ------------------------------------------------------------------------------------------------------
def attention_cases(res):
    B, H = 2, 3
    for n_k in KEY_COUNTS:
        for n_q in QUERY_COUNTS:
            g = torch.Generator().manual_seed(5000 + 10 * n_k + n_q)
            q, k, v = _rand(g, B, n_q, H, 64), _rand(g, B, n_k, H, 64), _rand(g, B, n_k, H, 64)
            res[f"attention_split|nq{n_q}|nk{n_k}"] = _sha(ops.attention(q, k, v, 0.125, split=True))
            for q0, nq in PROBS_RANGES[n_q]:
                res[f"attention_probs|nq{n_q}|nk{n_k}|q0_{q0}|n{nq}"] = _sha(ops.attention_probs(q, k, 0.125, q0=q0, nq=nq))


def bits():
    res = {}
    for cases in (layernorm_cases, gemm_cases, w16_cases, qkv_cases, attention_cases):
        cases(res)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="also write the JSON object to this file")
    a = ap.parse_args()
    res = bits()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1, sort_keys=True) + "\n")
    print(json.dumps(res, sort_keys=True))
