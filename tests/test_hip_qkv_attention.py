"""The fused QKV-projection + attention kernel (qkv_attention.hip, the north-star kernel) through the C ABI against an
fp64 evaluation of Attention.forward up to the output projection (vision_transformer.py:113-131), and against the
unfused pair of launches it replaces.

Below the first four tests: the kernel at every token count where a wave changes what it does (_qkv_attention_cases.COUNTS), with
poisoned padding around strided operands, alone against inside a batch, on inputs that force the running-maximum rescale, at
other softmax scales, and the arguments the library refuses.  Two bounds throughout, the ones of the first test: a flat
3e-6 max(1, |ref|max) for ordinary inputs, and 3 x the error of the unfused pair (W16 GEMM + sm_attention_f16x2: other kernels,
the same number formats) against the same fp64 reference; where the scores are large (stress inputs, scale 1) the witness is the
larger of the pair's error and that of torch fp32 on the CPU.  The measured errors go to the parity ledger, section "qkv_attention"."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from selfmask_amd import ops, _native as N  # noqa: E402
import _ledger as ledger  # noqa: E402
import _qkv_attention_cases as C  # noqa: E402
from _qkv_attention_cases import ref as _ref  # noqa: E402

DEV = "cuda:0"


@pytest.mark.parametrize("B,n,wstd,osplit", [
    (3, 197, 0.02, False),    # the headline shape: ViT-S/16 224^2
    (2, 197, 0.08, True),     # peaky softmax (far from uniform), F16X2 output
    (8, 197, 0.05, False),    # (B*6) % 8 == 0: the XCD-aware (image, head) order
    (1, 208, 0.05, False),    # the largest grid the kernel takes
    (2, 193, 0.05, True),     # one token in the last query block
    (2, 65, 0.05, False),     # small grids: the upper waves hold no queries
    (5, 1, 0.05, False),      # a single token
])
def test_fused_matches_fp64_and_unfused(B, n, wstd, osplit):
    g = torch.Generator().manual_seed(100 + n)
    xn = torch.randn(B * n, 384, generator=g)
    w = torch.randn(1152, 384, generator=g) * wstd
    b = torch.randn(1152, generator=g) * 0.1
    ref = _ref(xn, w, b, B, 0.125)
    got = ops.qkv_attention(xn.to(DEV), w.to(DEV), b.to(DEV), B, 0.125, out_f16x2=osplit)
    got = (ops.unsplit_f16x2(got) if osplit else got).double().cpu()
    err = (got - ref).abs().max().item()
    # the unfused product path: W16 GEMM (F16X2 output) + F16X2 attention
    w16, ws = ops.split_w16(w.to(DEV))
    qkv = ops.gemm_w16(ops.split_f16x2(xn.to(DEV)), w16, ws, b.to(DEV), out_f16x2=True)
    qkv5 = ops.unsplit_f16x2(qkv).reshape(B, n, 3, 6, 64)
    unf = ops.attention(qkv5[:, :, 0], qkv5[:, :, 1], qkv5[:, :, 2], 0.125, split=True).reshape(B * n, 384).double().cpu()
    err_unf = (unf - ref).abs().max().item()
    print(f"\nB={B} N={n} wstd={wstd}: fused-fp64 {err:.2e}  unfused-fp64 {err_unf:.2e}  max|ref| {ref.abs().max():.2f}")
    assert err <= 3e-6 * max(1.0, ref.abs().max().item())
    assert err <= 3.0 * err_unf + 1e-6


def test_rescale_branch_and_masked_tail():
    """One key whose score towers over the rest late in the sequence forces the lazy-maximum rescale branch; the tail
    keys 197..207 (stored duplicates of the last token) and the LDS rows past them must never leak into the result."""
    B, n = 2, 197
    g = torch.Generator().manual_seed(7)
    xn = torch.randn(B * n, 384, generator=g)
    w = torch.randn(1152, 384, generator=g) * 0.05
    b = torch.zeros(1152)
    xn[150] *= 6.0      # a huge key (and query) in the third 64-key chunk of image 0
    xn[n + 196] *= 8.0  # and the very last token of image 1
    ref = _ref(xn, w, b, B, 0.125)
    got = ops.qkv_attention(xn.to(DEV), w.to(DEV), b.to(DEV), B, 0.125).double().cpu()
    assert torch.isfinite(got).all()
    assert (got - ref).abs().max().item() <= 3e-6 * max(1.0, ref.abs().max().item())


def test_token_limit_is_reported():
    lib = N.load()
    assert lib.sm_qkv_attention_max_tokens() == 208
    with pytest.raises(RuntimeError, match="N=209"):
        ops.qkv_attention(torch.zeros(209, 384, device=DEV), torch.zeros(1152, 384, device=DEV) + 0.01,
                          torch.zeros(1152, device=DEV), 1)


@pytest.mark.parametrize("B,n", [(3, 197), (16, 197), (2, 65),
                                 (2, 17), (2, 33), (2, 193), (1, 208)])  # a wave's second tile of one token; a wave of one token; the limit
def test_fused_kernel_with_folded_layernorm(B, n):
    """norm1 folded into the projection (sm_qkv_attn_args.ln_stats): raw residual stream in, the norm's gain in the weights,
    (mu, r) per token from the producer's partial statistics - against LayerNorm + Attention.forward in fp64."""
    g = torch.Generator().manual_seed(300 + n)
    x = torch.randn(B * n, 384, generator=g) * 1.5 + torch.randn(B * n, 1, generator=g) * 0.5
    gamma, beta = torch.rand(384, generator=g) + 0.5, torch.randn(384, generator=g) * 0.2
    w = torch.randn(1152, 384, generator=g) * 0.05
    b = torch.randn(1152, generator=g) * 0.1
    xd = x.double()
    xn = (xd - xd.mean(1, keepdim=True)) / torch.sqrt(xd.var(1, unbiased=False, keepdim=True) + 1e-6) * gamma.double() + beta.double()
    ref = _ref(xn, w, b, B, 0.125)
    seg = x.reshape(B * n, 12, 32)
    mean = seg.mean(2)
    stats = torch.stack([mean, ((seg - mean[..., None]) ** 2).sum(2)], dim=2).contiguous()   # what the residual GEMM emits
    got = ops.qkv_attention(x.to(DEV), w.to(DEV), b.to(DEV), B, 0.125, ln=(gamma.to(DEV), beta.to(DEV), 1e-6, stats.to(DEV)))
    err = (got.double().cpu() - ref).abs().max().item()
    plain = ops.qkv_attention(xn.float().to(DEV), w.to(DEV), b.to(DEV), B, 0.125).double().cpu()
    err_plain = (plain - ref).abs().max().item()
    print(f"\nfolded LN, B={B} N={n}: folded-fp64 {err:.2e}  LayerNorm-first-fp64 {err_plain:.2e}  max|ref| {ref.abs().max():.2f}")
    assert err <= 4e-6 * max(1.0, ref.abs().max().item())
    assert err <= 3.0 * err_plain + 1e-6


def test_folded_layernorm_writes_the_same_f16x2_container():
    """the fold with the F16X2 output: the container is the split of what the fp32 launch stores (both go through store_f16x2_4)"""
    B, n = 2, 33
    g = torch.Generator().manual_seed(300 + n)
    x = torch.randn(B * n, 384, generator=g) * 1.5 + torch.randn(B * n, 1, generator=g) * 0.5
    gamma, beta = torch.rand(384, generator=g) + 0.5, torch.randn(384, generator=g) * 0.2
    w = torch.randn(1152, 384, generator=g) * 0.05
    b = torch.randn(1152, generator=g) * 0.1
    seg = x.reshape(B * n, 12, 32)
    mean = seg.mean(2)
    stats = torch.stack([mean, ((seg - mean[..., None]) ** 2).sum(2)], dim=2).contiguous()
    ln = (gamma.to(DEV), beta.to(DEV), 1e-6, stats.to(DEV))
    f32 = ops.qkv_attention(x.to(DEV), w.to(DEV), b.to(DEV), B, 0.125, ln=ln)
    f16 = ops.qkv_attention(x.to(DEV), w.to(DEV), b.to(DEV), B, 0.125, out_f16x2=True, ln=ln)
    assert torch.isfinite(f32).all()
    assert torch.equal(f16.view(torch.int32), ops.split_f16x2(f32).view(torch.int32))


# ---- every token count, strides, batch independence, the rescale branch, other scales -------------------------------------------
def _unfused(xn, w, b, B, scale):
    """the two launches the kernel replaces: W16 GEMM (F16X2 output) + F16X2 attention, on device tensors -> float64 on the CPU"""
    n = xn.shape[0] // B
    w16, ws = ops.split_w16(w)
    qkv = ops.gemm_w16(ops.split_f16x2(xn), w16, ws, b, out_f16x2=True)
    qkv5 = ops.unsplit_f16x2(qkv).reshape(B, n, 3, 6, 64)
    return ops.attention(qkv5[:, :, 0], qkv5[:, :, 1], qkv5[:, :, 2], scale, split=True).reshape(B * n, 384).double().cpu()


@functools.lru_cache(maxsize=None)
def _witness(kind, B, n, scale=0.125):
    """(xn, w, b on the device; fp64 reference; error of the unfused pair; error of torch fp32 on the CPU) - once per input"""
    xn, w, b = C.ordinary(B, n) if kind == "ordinary" else C.stress(kind, B, n)
    ref = C.ref(xn, w, b, B, scale)
    dev = tuple(t.to(DEV) for t in (xn, w, b))
    err_unf = (_unfused(*dev, B, scale) - ref).abs().max().item()
    err_f32 = (C.ref_f32(xn, w, b, B, scale).double() - ref).abs().max().item()
    return dev, ref, err_unf, err_f32


def _values(t, osplit):
    return (ops.unsplit_f16x2(t) if osplit else t).double().cpu()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _ordinary_rule(test, key, got, ref, err_unf):
    err = (got - ref).abs().max().item()
    flat, rel = 3e-6 * max(1.0, ref.abs().max().item()), 3.0 * err_unf + 1e-6
    print(f"\n{test} {key}: fused-fp64 {err:.2e}  unfused-fp64 {err_unf:.2e}  max|ref| {ref.abs().max():.2f}")
    ledger.record("qkv_attention", f"{test}|{key}", {"fused_minus_f64": err, "unfused_minus_f64": err_unf, "bound_flat": flat,
                                                    "bound_unfused": rel, "err_over_bound": err / min(flat, rel)})
    assert torch.isfinite(got).all()
    assert err <= flat
    assert err <= rel


def _stress_rule(test, key, got, ref, err_unf, err_f32):
    err = (got - ref).abs().max().item()
    bound = 3.0 * max(err_unf, err_f32) + 1e-6
    print(f"\n{test} {key}: fused-fp64 {err:.2e}  unfused-fp64 {err_unf:.2e}  f32-fp64 {err_f32:.2e}  max|ref| {ref.abs().max():.2f}")
    ledger.record("qkv_attention", f"{test}|{key}", {"fused_minus_f64": err, "unfused_minus_f64": err_unf, "f32_minus_f64": err_f32,
                                                    "bound": bound, "err_over_bound": err / bound})
    assert torch.isfinite(got).all()
    assert err <= bound


@pytest.mark.parametrize("osplit", [False, True], ids=["f32", "f16x2"])
@pytest.mark.parametrize("n", C.COUNTS)
def test_token_count_sweep(n, osplit):
    """B = 2 at every count of COUNTS: one or two tiles per wave, waves without a query, every number of key steps, every fill of
    the last one.  The F16X2 container is the split of what the fp32 launch stores."""
    B = 2
    (xn, w, b), ref, err_unf, _ = _witness("ordinary", B, n)
    got = ops.qkv_attention(xn, w, b, B, 0.125, out_f16x2=osplit)
    if osplit:
        f32 = ops.qkv_attention(xn, w, b, B, 0.125)
        assert torch.equal(_bits(got), _bits(ops.split_f16x2(f32)))
    _ordinary_rule("sweep", f"N{n}_{'f16x2' if osplit else 'f32'}", _values(got, osplit), ref, err_unf)


@pytest.mark.parametrize("osplit", [False, True], ids=["f32", "f16x2"])
@pytest.mark.parametrize("n", [33, 197, 208])
def test_poisoned_padding_and_strides(n, osplit):
    """ldx = 400 and ldo = 416: the input is a column slice (from column 8) of a buffer that is NaN everywhere else - the gap
    columns, a row in front, a row behind; the output a column slice (from column 16) of a buffer of sentinels between two NaN rows.
    Nothing outside the 384 columns of the B N rows is read (the result is finite and right) or written (every other word keeps its
    bits), and the result has the bits of the contiguous launch."""
    B = 3
    M = B * n
    (xn, w, b), ref, err_unf, _ = _witness("ordinary", B, n)
    bufx = torch.full((M + 2, 400), float("nan"), device=DEV)
    xs = bufx[1:M + 1, 8:392]
    xs.view(torch.int32).copy_(ops.split_f16x2(xn).view(torch.int32))
    bufo = torch.full((M + 2, 416), -12345.0, device=DEV)
    bufo[0] = float("nan")
    bufo[M + 1] = float("nan")
    out = bufo[1:M + 1, 16:400]
    assert xs.stride(0) == 400 and out.stride(0) == 416
    x_before, o_before = bufx.view(torch.int32).clone(), bufo.view(torch.int32).clone()
    res = ops.qkv_attention(None, w, b, B, 0.125, out_f16x2=osplit, xs=xs, out=out)
    torch.cuda.synchronize()
    assert res.data_ptr() == out.data_ptr()
    assert torch.equal(bufx.view(torch.int32), x_before)
    outside = torch.ones((M + 2, 416), dtype=torch.bool, device=DEV)
    outside[1:M + 1, 16:400] = False
    assert torch.equal(bufo.view(torch.int32)[outside], o_before[outside]), "a word outside the output slice was written"
    _ordinary_rule("strides", f"N{n}_{'f16x2' if osplit else 'f32'}", _values(out.contiguous(), osplit), ref, err_unf)
    assert torch.equal(_bits(out), _bits(ops.qkv_attention(xn, w, b, B, 0.125, out_f16x2=osplit)))


@pytest.mark.parametrize("n", [17, 99, 197])
def test_bits_do_not_depend_on_the_batch(n):
    """F16X2 output (the forward's): image b alone (6 workgroups) = image b inside B = 3 (18 workgroups in plain order) = image b
    inside B = 8 (48 workgroups in the XCD-aware order), and a second launch reproduces the first."""
    (xn, w, b), _, _, _ = _witness("ordinary", 8, n)
    run = lambda rows, B: _bits(ops.qkv_attention(rows, w, b, B, 0.125, out_f16x2=True))  # noqa: E731
    in8, in3 = run(xn, 8), run(xn[:3 * n], 3)
    assert torch.equal(run(xn, 8), in8) and torch.equal(run(xn[:3 * n], 3), in3)
    assert torch.isfinite(ops.unsplit_f16x2(in8.view(torch.float32))).all()
    for img in range(8):
        alone = run(xn[img * n:(img + 1) * n], 1)
        assert torch.equal(alone, in8[img * n:(img + 1) * n]), f"image {img} alone differs from image {img} of 8"
        if img < 3:
            assert torch.equal(alone, in3[img * n:(img + 1) * n]), f"image {img} alone differs from image {img} of 3"


@pytest.mark.parametrize("osplit", [False, True], ids=["f32", "f16x2"])
@pytest.mark.parametrize("n", C.STRESS_COUNTS)
@pytest.mark.parametrize("recipe", C.RECIPES)
def test_rescale_recipes(recipe, n, osplit):
    """Inputs whose running maximum keeps rising / rises in one query tile of a wave only / arrives in the last, masked step
    (test_qkv_attention_cases_cpu.py replays the kernel's rule on them).  Scores reach ~70 after scaling, ten times the ordinary
    ones, so the bound is relative to the witnesses alone: 3 max(unfused pair, torch fp32) + 1e-6."""
    B = 2
    (xn, w, b), ref, err_unf, err_f32 = _witness(recipe, B, n)
    got = ops.qkv_attention(xn, w, b, B, 0.125, out_f16x2=osplit)
    _stress_rule("rescale", f"{recipe}_N{n}_{'f16x2' if osplit else 'f32'}", _values(got, osplit), ref, err_unf, err_f32)


@pytest.mark.parametrize("n", [99, 197])
@pytest.mark.parametrize("scale", [0.05, 0.25, 1.0])
def test_other_softmax_scales(scale, n):
    """the laziness limit 8 / (scale log2 e) and the exponent both derive from `scale`; at 1.0 the softmax is peaky"""
    B = 2
    (xn, w, b), ref, err_unf, err_f32 = _witness("ordinary", B, n, scale)
    got = ops.qkv_attention(xn, w, b, B, scale)
    _stress_rule("scales", f"scale{scale}_N{n}", _values(got, False), ref, err_unf, err_f32)


# ---- arguments the library refuses -------------------------------------------------------------------------------------------------
def _bad_ldx380(a, t): a.ldx = 380                                   # noqa: E704  not a multiple of 8
def _bad_ldx376(a, t): a.ldx = 376                                   # noqa: E704  a multiple of 8 below the row length
def _bad_ldo(a, t): a.ldo = 388                                      # noqa: E704  not a multiple of 8
def _bad_o_ptr(a, t): a.O = t["o"].data_ptr() + 16                   # noqa: E704  16-B aligned only
def _bad_scale(a, t): a.scale = 0.0                                  # noqa: E704
def _bad_w_scale(a, t): a.w_scale = 0.3                              # noqa: E704  not a power of two
def _bad_ln(a, t): a.ln_stats, a.ln_eps = t["stats"].data_ptr(), 1e-6  # noqa: E704  statistics without ln_c
def _bad_b(a, t): a.B = 0                                            # noqa: E704
def _bad_n(a, t): a.N = 0                                            # noqa: E704


@pytest.mark.parametrize("spoil", [_bad_ldx380, _bad_ldx376, _bad_ldo, _bad_o_ptr, _bad_scale, _bad_w_scale, _bad_ln, _bad_b, _bad_n],
                         ids=lambda f: f.__name__[5:])
def test_arguments_are_refused_before_a_launch(spoil):
    """real device pointers, one field wrong: RuntimeError, and the output keeps its fill.  (N = 209: test_token_limit_is_reported.)"""
    B, n = 2, 33
    (xn, w, b), _, _, _ = _witness("ordinary", B, n)
    w16, ws = ops.split_w16(w)
    t = {"xs": ops.split_f16x2(xn), "o": torch.full((B * n + 1, 384), -7.0, device=DEV), "stats": torch.zeros(B * n, 12, 2, device=DEV)}

    def args():
        a = N.QkvAttnArgs()
        a.Xn, a.Wqkv, a.bias, a.O = t["xs"].data_ptr(), w16.data_ptr(), b.data_ptr(), t["o"].data_ptr()
        a.ldx, a.ldo, a.B, a.N, a.w_scale, a.scale, a.out_f16x2 = 384, 384, B, n, ws, 0.125, 0
        return a

    lib = N.load()
    a = args()
    spoil(a, t)
    with pytest.raises(RuntimeError, match="sm_qkv_attention_w16"):
        N.check(lib.sm_qkv_attention_w16(a, torch.cuda.current_stream().cuda_stream), "sm_qkv_attention_w16")
    torch.cuda.synchronize()
    assert bool((t["o"] == -7.0).all())
    # the same arguments unspoiled are taken: each refusal above is that of the one field
    N.check(lib.sm_qkv_attention_w16(args(), torch.cuda.current_stream().cuda_stream), "sm_qkv_attention_w16")
    torch.cuda.synchronize()
    assert torch.equal(t["o"][:B * n], ops.qkv_attention(xn, w, b, B, 0.125)) and bool((t["o"][B * n:] == -7.0).all())
