"""Per-kernel parity: each C-ABI entry point against the stock torch-CPU op it replaces (fp64 as truth)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from selfmask_amd import _native as N  # noqa: E402
from selfmask_amd import ops  # noqa: E402

DEV = "cuda:0"


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).float()


def _maxerr(a, b):
    return (a.double().cpu() - b.double().cpu()).abs().max().item()


@pytest.mark.parametrize("tile", [(128, 128), (128, 64), (64, 64), None])
@pytest.mark.parametrize("M,Nn,K", [(197 * 3, 1152, 384), (300, 384, 1536), (120, 784, 384), (33, 64, 32)])
def test_gemm_bias_all_tiles(tile, M, Nn, K):
    a, w, b = _rand(M, K, seed=1), _rand(Nn, K, seed=2, scale=0.05), _rand(Nn, seed=3)
    c = ops.gemm(a.to(DEV), w.to(DEV), b.to(DEV), tile=tile)
    ref = a.double() @ w.double().T + b.double()
    # exact-fp32 products, fp32 accumulation: error ~ sqrt(K) * eps * |row|.|col|
    tol = 4e-7 * math.sqrt(K) * (a.abs().max() * w.abs().max() * math.sqrt(K)).item() + 1e-6
    assert _maxerr(c, ref) <= tol
    # and as close to fp64 as torch's own fp32 GEMM is (x3 slack)
    assert _maxerr(c, ref) <= 3 * _maxerr(a @ w.T + b, ref) + 1e-6


@pytest.mark.parametrize("epi", ["gelu", "relu", "residual", "sigmoid2"])
def test_gemm_epilogues(epi):
    M, Nn, K = 257, 192, 384
    a, w, b, r = _rand(M, K, seed=4), _rand(Nn, K, seed=5, scale=0.05), _rand(Nn, seed=6), _rand(M, Nn, seed=7)
    lin = a.double() @ w.double().T + b.double()
    if epi == "gelu":
        c = ops.gemm(a.to(DEV), w.to(DEV), b.to(DEV), epilogue=N.EPI_GELU)
        ref = F.gelu(lin)
    elif epi == "relu":
        c = ops.gemm(a.to(DEV), w.to(DEV), b.to(DEV), epilogue=N.EPI_RELU)
        ref = F.relu(lin)
    elif epi == "residual":
        rd = r.to(DEV)
        c = ops.gemm(a.to(DEV), w.to(DEV), b.to(DEV), epilogue=N.EPI_RESIDUAL, residual=rd, out=rd)  # in place
        ref = r.double() + lin
    else:
        c, c2 = ops.gemm(a.to(DEV), w.to(DEV), None, epilogue=N.EPI_SIGMOID2)
        ref = a.double() @ w.double().T
        assert _maxerr(c2, torch.sigmoid(ref)) <= 2e-6
    assert _maxerr(c, ref) <= 2e-5


def test_gemm_split_k_and_alt_operand():
    M, Nn, K = 300, 384, 1536
    a, w = _rand(M, K, seed=14), _rand(Nn, K, seed=15, scale=0.05)
    parts = ops.gemm(a.to(DEV), w.to(DEV), split_k=4)  # (4, M, N) raw partials
    assert parts.shape == (4, M, Nn)
    assert _maxerr(parts.sum(0), a.double() @ w.double().T) <= 2e-5
    for s_ in range(4):
        ks = slice(s_ * 384, (s_ + 1) * 384)
        assert _maxerr(parts[s_], a[:, ks].double() @ w[:, ks].double().T) <= 1e-5
    # fused split-K reduction in LayerNorm: LN(residual + (sum of slices + bias))
    g, b, bias, res = 1 + 0.1 * _rand(384, seed=16), 0.1 * _rand(384, seed=17), _rand(384, seed=18), _rand(M, 384, seed=19)
    from selfmask_amd import _native as Nn_
    y = torch.empty(M, 384, device=DEV)
    la = Nn_.LnArgs()
    gd, bd, biasd, resd = g.to(DEV), b.to(DEV), bias.to(DEV), res.to(DEV)
    la.x, la.ldx, la.gamma, la.beta, la.y, la.ldy = parts.data_ptr(), 384, gd.data_ptr(), bd.data_ptr(), y.data_ptr(), 384
    la.rows, la.eps, la.n_partials, la.partial_stride = M, 1e-5, 4, M * 384
    la.pre_bias, la.residual = biasd.data_ptr(), resd.data_ptr()
    Nn_.check(Nn_.load().sm_layernorm_rows_f32(la, torch.cuda.current_stream().cuda_stream))
    ref = F.layer_norm(res.double() + a.double() @ w.double().T + bias.double(), (384,), g.double(), b.double(), 1e-5)
    assert _maxerr(y, ref) <= 2e-5
    # ... and the sum itself, in place over the residual (a pre-norm block's stream: the encoder's split fc2 at batch 1-2)
    la.raw = resd.data_ptr()
    y2 = torch.empty(M, 384, device=DEV)
    la.y = y2.data_ptr()
    Nn_.check(Nn_.load().sm_layernorm_rows_f32(la, torch.cuda.current_stream().cuda_stream))
    assert torch.equal(y2, y)
    assert _maxerr(resd, res.double() + a.double() @ w.double().T + bias.double()) <= 2e-5
    # A_alt: columns >= 768 use the second A operand (decoder self-attention q|k from tgt+qpos, v from tgt)
    a1, a2, w3, b3 = _rand(60, 384, seed=20), _rand(60, 384, seed=21), _rand(1152, 384, seed=22, scale=0.05), _rand(1152, seed=23)
    c = ops.gemm(a1.to(DEV), w3.to(DEV), b3.to(DEV), a_alt=a2.to(DEV), alt_from_n=768)
    ref = torch.cat([a1.double() @ w3[:768].double().T, a2.double() @ w3[768:].double().T], 1) + b3.double()
    assert _maxerr(c, ref) <= 2e-5


def test_gemm_batched():
    B, M, Nn, K = 3, 120, 784, 384
    a, w = _rand(B, M, K, seed=8), _rand(B, Nn, K, seed=9, scale=0.1)
    c = ops.gemm(a.to(DEV), w.to(DEV))
    assert _maxerr(c, torch.einsum("bmk,bnk->bmn", a.double(), w.double())) <= 3e-5


@pytest.mark.parametrize("tile", [(128, 128), (128, 64), (64, 64)])
def test_gemm_pipeline_race_screen(tile):
    """The LDS-DMA ring (counted vmcnt + one barrier per K-tile) must give the same bits on every launch and agree
    with fp64 for short (K=32: fewer tiles than stages) and long K."""
    for K in (32, 64, 96, 1536):
        a, w = _rand(391, K, seed=80 + K), _rand(320, K, seed=81 + K, scale=0.1)
        ad, wd = a.to(DEV), w.to(DEV)
        first = ops.gemm(ad, wd, tile=tile)
        assert _maxerr(first, a.double() @ w.double().T) <= 2e-5
        for _ in range(20):
            assert torch.equal(ops.gemm(ad, wd, tile=tile), first)


def test_gemm_rejects_bad_shapes():
    a, w = _rand(8, 40).to(DEV), _rand(64, 40).to(DEV)
    with pytest.raises(RuntimeError, match="multiple of 32"):
        ops.gemm(a, w)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.gemm(_rand(8, 32), _rand(64, 32))


@pytest.mark.parametrize("rows,eps", [(1, 1e-6), (197 * 2, 1e-6), (1283, 1e-5)])
def test_layernorm(rows, eps):
    x, g, b = _rand(rows, 384, seed=20, scale=3.0) + 0.7, 1 + 0.1 * _rand(384, seed=21), 0.1 * _rand(384, seed=22)
    y = ops.layernorm(x.to(DEV), g.to(DEV), b.to(DEV), eps)
    ref = F.layer_norm(x.double(), (384,), g.double(), b.double(), eps)
    assert _maxerr(y, ref) <= 2e-6
    assert _maxerr(y, ref) <= 3 * _maxerr(F.layer_norm(x, (384,), g, b, eps), ref) + 5e-7


def test_layernorm_second_output_and_row_maps():
    # y2 = y + add[r % 20]: the decoder's "tgt + query_pos" operand
    x, g, b, qp = _rand(60, 384, seed=23), 1 + 0.1 * _rand(384, seed=24), 0.1 * _rand(384, seed=25), _rand(20, 384, seed=26)
    y, y2 = ops.layernorm(x.to(DEV), g.to(DEV), b.to(DEV), 1e-5, add=qp.to(DEV))
    ref = F.layer_norm(x.double(), (384,), g.double(), b.double(), 1e-5)
    assert _maxerr(y, ref) <= 2e-6 and _maxerr(y2, ref + qp.repeat(3, 1).double()) <= 2e-6
    # drop the cls row of each image: logical row r reads x row (r/n)*(n+1) + 1 + r%n
    n, Bq = 5, 3
    xt = _rand(Bq * (n + 1), 384, seed=27)
    y = ops.layernorm(xt.to(DEV), g.to(DEV), b.to(DEV), 1e-6, in_map=(n, n + 1, 1), rows=Bq * n)
    ref = F.layer_norm(xt.view(Bq, n + 1, 384)[:, 1:].reshape(-1, 384).double(), (384,), g.double(), b.double(), 1e-6)
    assert _maxerr(y, ref) <= 2e-6
    # scatter layer l of L into a (B, L, nq, 384) stack
    L, l, nq = 4, 2, 5
    xq = _rand(Bq * nq, 384, seed=28)
    out = ops.layernorm(xq.to(DEV), g.to(DEV), b.to(DEV), 1e-5, out_map=(nq, L * nq, l * nq), out_rows=Bq * L * nq)
    ref = F.layer_norm(xq.double(), (384,), g.double(), b.double(), 1e-5).view(Bq, nq, 384)
    assert _maxerr(out.view(Bq, L, nq, 384)[:, l], ref) <= 2e-6


def _attn_ref(q, k, v, scale):
    s = torch.einsum("bqhd,bkhd->bhqk", q.double(), k.double()) * scale
    p = s.softmax(-1)
    return torch.einsum("bhqk,bkhd->bqhd", p, v.double()).reshape(q.shape[0], q.shape[1], -1)


@pytest.mark.parametrize("B,nq,nk", [(2, 197, 197), (1, 785, 785), (1, 577, 577), (3, 20, 20), (3, 20, 196), (2, 20, 784),
                                      (1, 1, 1), (1, 33, 225),
                                      # key counts at the edges of the split kernel's 64-key chunks and 32-key blocks: a chunk exactly
                                      # full, one key over, exactly one block
                                      (1, 5, 32), (1, 5, 64), (1, 40, 65), (2, 33, 96), (1, 64, 128)])
@pytest.mark.parametrize("split", [False, True])
def test_attention_shapes(B, nq, nk, split):
    qkv = _rand(B, max(nq, nk), 3, 6, 64, seed=30, scale=1.5).to(DEV)
    q, k, v = qkv[:, :nq, 0], qkv[:, :nk, 1], qkv[:, :nk, 2]  # strided views like the packed qkv buffer
    o = ops.attention(q, k, v, 0.125, split=split)
    ref = _attn_ref(q.cpu(), k.cpu(), v.cpu(), 0.125)
    ref32 = F.scaled_dot_product_attention(q.cpu().transpose(1, 2), k.cpu().transpose(1, 2), v.cpu().transpose(1, 2),
                                           scale=0.125).transpose(1, 2).reshape(B, nq, -1)
    assert _maxerr(o, ref) <= max(1e-5, 3 * _maxerr(ref32, ref))


@pytest.mark.parametrize("split", [False, True])
def test_attention_online_softmax_rescale_branch(split):
    """Force the running-max rescale between 224-key chunks: the global max sits in the LAST chunk (rule: a rare
    data-dependent branch needs an input that takes it)."""
    B, n = 1, 500
    q, k, v = _rand(B, n, 6, 64, seed=31), _rand(B, n, 6, 64, seed=32), _rand(B, n, 6, 64, seed=33)
    k[:, 470] = q[:, 5] * 4.0  # spike: key 470 (third chunk) dominates query 5
    k[:, 3] = q[:, 100] * 3.0  # and a first-chunk spike for another row
    o = ops.attention(q.to(DEV), k.to(DEV), v.to(DEV), 0.125, split=split)
    assert _maxerr(o, _attn_ref(q, k, v, 0.125)) <= 5e-6


@pytest.mark.parametrize("P,H,W", [(16, 224, 224), (8, 64, 72), (16, 250, 333), (8, 30, 21)])
def test_im2col(P, H, W):
    x = _rand(2, 3, H, W, seed=40)
    cols = ops.im2col_patches(x.to(DEV), P)
    xp = F.pad(x, (0, (P - W % P) % P, 0, (P - H % P) % P))
    ref = F.unfold(xp, kernel_size=P, stride=P).transpose(1, 2).reshape(-1, 3 * P * P)
    assert torch.equal(cols.cpu(), ref)


@pytest.mark.parametrize("g0,gh,gw", [(14, 24, 24), (14, 16, 21), (28, 25, 21), (14, 7, 9)])
def test_pos_embed_bicubic(g0, gh, gw):
    pos = _rand(1 + g0 * g0, 384, seed=50, scale=0.05)
    out = ops.pos_embed_bicubic(pos.to(DEV), gh, gw)
    grid = F.interpolate(pos[1:].reshape(1, g0, g0, 384).permute(0, 3, 1, 2), size=(gh, gw), mode="bicubic",
                         align_corners=False).permute(0, 2, 3, 1).reshape(-1, 384)
    assert torch.equal(out[0].cpu(), pos[0])
    assert _maxerr(out[1:], grid) <= 1e-6


@pytest.mark.parametrize("gh,gw", [(14, 14), (16, 21), (1, 1), (3, 1)])
def test_upsample2x(gh, gw):
    tok = _rand(2, gh * gw, 384, seed=60)
    up = ops.upsample2x_tokens(tok.to(DEV), gh, gw)
    ref = F.interpolate(tok.permute(0, 2, 1).reshape(2, 384, gh, gw), scale_factor=2, mode="bilinear")
    ref = ref.permute(0, 2, 3, 1).reshape(2, 4 * gh * gw, 384)
    assert _maxerr(up, ref) <= 1e-6


def test_rowdot_sigmoid():
    h, w, b = _rand(241, 384, seed=70), _rand(384, seed=71, scale=0.1), _rand(1, seed=72)
    out = ops.rowdot_sigmoid(h.to(DEV), w.to(DEV), b.to(DEV))
    assert _maxerr(out, torch.sigmoid(h.double() @ w.double() + b.double())) <= 1e-6
