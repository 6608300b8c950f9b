"""sm_attention_probs_f16x2 alone: the post-softmax attention matrix (vision_transformer.py:122-123) from F16X2 operands.

Random q, k are rounded to what F16X2 holds; the truth is fp64 softmax(q k^T * scale) of those same values, the witness the
reference's own ops in fp32 on the CPU.  Parity rule, per case:  max|hip - f64| <= 4 * max|f32 - f64|  - the factor 4 is two bits:
the split product keeps 22 significant bits against fp32's 24, nothing else in the kernel is less exact than fp32.  The measured
ratios go to the parity ledger (section "attention_probs")."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from selfmask_amd import ops  # noqa: E402
import _ledger as ledger  # noqa: E402

DEV = "cuda:0"
HEADS = 6
SHAPES = [(1, 1), (2, 21), (2, 197), (1, 209), (1, 337), (1, 526),  # (B, n): single key; small grid; tail masked up to 208;
          #                                                          one past the fused limit; the 250 x 333 grid; the P8 grid
          (1, 32), (1, 64), (1, 65), (1, 96), (1, 128)]  # a 64-key chunk exactly full, one key over, exactly one 32-key block
REGIMES = {"unit": 1.0, "peaky": 15.0}  # unit-variance q, k: |score| <= ~5;  q x 15: |score| reaches ~60, most of a row underflows
GUARD = 257  # floats of NaN behind every image's block (odd: the blocks do not stay aligned), and a sentinel block in front


@functools.lru_cache(maxsize=None)
def _case(B, n, regime):
    g = torch.Generator().manual_seed(1000 * n + B + (7 if regime == "peaky" else 0))
    q = torch.randn(B, n, HEADS, 64, generator=g) * REGIMES[regime]
    k = torch.randn(B, n, HEADS, 64, generator=g)
    # what F16X2 holds: hi + lo / 2048 (22 bits), exact in fp32
    q, k = (ops.unsplit_f16x2(ops.split_f16x2(t.reshape(B, n, HEADS * 64).to(DEV))).reshape(B, n, HEADS, 64).cpu() for t in (q, k))
    qh, kh = q.permute(0, 2, 1, 3), k.permute(0, 2, 1, 3)  # (B, H, n, 64)
    f32 = ((qh @ kh.transpose(-2, -1)) * 0.125).softmax(-1)
    s64 = (qh.double() @ kh.double().transpose(-2, -1)) * 0.125
    f64 = s64.softmax(-1)
    return q.to(DEV), k.to(DEV), f32, f64, float(s64.abs().max())


def _guarded(B, nq, n):
    """(flat buffer, (B, H, nq, n) view into it): sentinel block | image 0 | NaN guard | image 1 | NaN guard ..."""
    blk = HEADS * nq * n
    buf = torch.full((GUARD + B * (blk + GUARD),), float("nan"), device=DEV)
    buf[:GUARD] = 12345.0
    view = torch.as_strided(buf, (B, HEADS, nq, n), (blk + GUARD, nq * n, n, 1), GUARD)
    view.fill_(-7.0)  # an entry the kernel skips stays negative
    return buf, view, blk


@pytest.mark.parametrize("regime", list(REGIMES))
@pytest.mark.parametrize("B,n", SHAPES)
def test_parity_and_structure(B, n, regime):
    q, k, f32, f64, smax = _case(B, n, regime)
    buf, p, blk = _guarded(B, n, n)
    ops.attention_probs(q, k, out=p)
    torch.cuda.synchronize()
    # nothing outside the images' blocks was touched: no masked key (n up to the next multiple of 32 / 64) was written
    assert (buf[:GUARD] == 12345.0).all()
    for b in range(B):
        g0 = GUARD + b * (blk + GUARD) + blk
        assert torch.isnan(buf[g0:g0 + GUARD]).all(), f"guard band behind image {b} was written"
    full = p.contiguous()
    hip = full.cpu()
    assert not torch.isnan(hip).any() and (hip >= 0).all()
    assert (hip.sum(-1) - 1).abs().max() <= 1e-5  # sanity, far above n * 2^-24; not the parity measure
    e_hip = (hip.double() - f64).abs().max().item()
    e_f32 = (f32.double() - f64).abs().max().item()
    ratio = e_hip / e_f32 if e_f32 > 0 else (0.0 if e_hip == 0 else float("inf"))
    print(f"\nB={B} n={n} {regime}: |score|max={smax:.1f} hip-f64={e_hip:.3e} f32-f64={e_f32:.3e} ratio={ratio:.2f}")
    ledger.record("attention_probs", f"B{B}_n{n}_{regime}", {"score_absmax": smax, "hip_minus_f64": e_hip, "f32_minus_f64": e_f32,
                                                             "ratio": ratio})
    assert e_hip <= 4.0 * e_f32
    # a row's bits do not depend on the launch it is part of
    for q0, q1 in {(0, 1), (min(5, n - 1), min(37, n)), (n - 1, n)}:
        part = ops.attention_probs(q, k, q0=q0, nq=q1 - q0)
        assert part.shape == (B, HEADS, q1 - q0, n)
        assert torch.equal(part, full[:, :, q0:q1]), f"rows [{q0}, {q1}) differ from the full launch"
    # ... nor on the batch: image b alone = image b inside the batch
    if B > 1:
        for b in range(B):
            assert torch.equal(ops.attention_probs(q[b:b + 1], k[b:b + 1]), full[b:b + 1])
    # and twice the same launch gives the same bits
    assert torch.equal(ops.attention_probs(q, k), full)


def test_rectangular_and_strided_operands():
    """n_q != n_k, and q / k as column slices of one (B, n, 3 * 384) projection output (the forward's layout)."""
    B, nq, nk = 2, 45, 70
    g = torch.Generator().manual_seed(5)
    qkv = torch.randn(B, nk, 3 * 384, generator=g).to(DEV)
    q = qkv[:, :nq, :384].reshape(B, nq, HEADS, 64)
    k = qkv[:, :, 384:768].reshape(B, nk, HEADS, 64)
    p = ops.attention_probs(q, k, q0=3, nq=40)
    qr, kr = (ops.unsplit_f16x2(ops.split_f16x2(t.reshape(B, -1, 384).contiguous())).reshape(B, -1, HEADS, 64).cpu().double() for t in (q, k))
    f64 = ((qr.permute(0, 2, 1, 3) @ kr.permute(0, 2, 3, 1)) * 0.125).softmax(-1)[:, :, 3:43]
    qf, kf = qr.float(), kr.float()
    f32 = ((qf.permute(0, 2, 1, 3) @ kf.permute(0, 2, 3, 1)) * 0.125).softmax(-1)[:, :, 3:43]
    assert p.shape == (B, HEADS, 40, nk)
    assert (p.cpu().double() - f64).abs().max() <= 4.0 * (f32.double() - f64).abs().max()
