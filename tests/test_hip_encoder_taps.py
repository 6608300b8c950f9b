"""Encoder taps on the device (MaskFormer.encoder_taps / encoder_layers, the methods of ``model.encoder``, forward(return_layers=...))
against the REAL reference's vectors (tests/golden/encoder_taps_*.npz, scripts/gen_encoder_taps_golden.py), against each other bit for
bit, and - for shapes without a fixture - against the fp64 restatement (tests/_encoder_taps_ref.py).

Rule, per fixture, gemm mode and attention path:  max|hip - ref64| <= 4 * f32_vs_f64_maxabs  of that layer over the stored entries, and
the same for every block's CLS attention row - the reference side is frozen in the fixture; the code under test never sets its own
bar.  Measured figures go to the parity ledger (section "encoder_taps"; committed as profiles/encoder_taps_parity.json)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _encoder_taps_ref as R  # noqa: E402
import _ledger as ledger  # noqa: E402
from selfmask_amd import MaskFormer, ops, synthetic_images, synthetic_state_dict  # noqa: E402
from selfmask_amd.graphs import GraphedForward  # noqa: E402

DEV = "cuda:0"
MODES = ["w16", "f16x2", "fp32"]  # gemm_mode 2, 1, 0


@functools.lru_cache(maxsize=4)
def _fixture(name):
    return R.Fixture(name)


@functools.lru_cache(maxsize=2)
def _model(patch, wseed, style, mode):
    m = MaskFormer(n_queries=20, patch_size=patch, n_decoder_layers=6, return_intermediate=True, use_binary_classifier=True,
                   gemm_mode=mode)
    m.load_state_dict(synthetic_state_dict(wseed, style, patch_size=patch), strict=True)
    return m.to(DEV)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", R.FIXTURES)
def test_matches_reference_vectors(name, mode):
    """MEASURED on MI355X (per layer / block, max|hip - ref64| over 4 * f32_vs_f64_maxabs): see profiles/encoder_taps_parity.json."""
    fx = _fixture(name)
    m = _model(fx.patch, fx.wseed, fx.style, mode)
    x = fx.images().to(DEV)
    ok = True
    for path in (1, 2):  # at N = 197 path 1 runs the fused kernel; above 208 tokens both are the two-launch pair
        t = m.encoder_taps(x, layers=None, attn_layers=None, attn="cls", patch_mean=True, attn_path=path)
        assert t["tokens"].shape == (fx.B, 12, fx.n, 384) and t["attn"].shape == (12, fx.B, 6, fx.n)
        tok, att = t["tokens"].cpu(), t["attn"].cpu()
        assert not torch.isnan(tok).any() and not torch.isnan(att).any() and (att.sum(-1) - 1).abs().max() <= 1e-5
        d, da = fx.token_errors(tok.numpy()), fx.attn_errors(att.numpy())
        dm = float(np.abs(t["patch_mean"].cpu().numpy().astype(np.float64) - fx.mean_f64).max())
        print(f"\n[{mode} path {path}] {name}: tokens hip-ref64 / (ref32-ref64) per layer {np.round(d / fx.bar, 2).tolist()}"
              f"\n    attention per block {np.round(da / fx.attn_bar, 2).tolist()} (bar 4); patch mean hip-ref64 = {dm:.2e}")
        ledger.record("encoder_taps", f"{name}|{mode}|path{path}", {
            "token_ratio_per_layer": (d / fx.bar).tolist(), "attn_ratio_per_block": (da / fx.attn_bar).tolist(),
            "worst_token_ratio": float((d / fx.bar).max()), "worst_attn_ratio": float((da / fx.attn_bar).max()),
            "ref32_minus_ref64_per_layer": fx.bar.tolist(), "patch_mean_hip_minus_ref64": dm})
        ok = ok and bool((d <= 4.0 * fx.bar).all()) and bool((da <= 4.0 * fx.attn_bar).all())
    assert ok


@pytest.fixture(scope="module")
def peaky():
    fx = _fixture("p16_224_peaky")
    return fx, _model(fx.patch, fx.wseed, fx.style, "w16"), fx.images().to(DEV)


# ---- exact relations: no tolerance -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["auto", "fused", "unfused"])
def test_exact_relations_between_the_taps(peaky, path):
    fx, m, x = peaky
    m.attention_path = path
    try:
        full = m.encoder_layers(x)
        assert full.shape == (fx.B, 12, fx.n, 384)
        # layer 12's patch rows are the forward's own patch tokens
        assert torch.equal(full[:, 11, 1:], m(x, return_logits=True)["patch_tokens"])
        assert torch.equal(full[:, 11, 1:], m(x, encoder_only=True)["patch_tokens"].reshape(fx.B, -1, 384))
        # row selections are slices: the other rows are never read, the selected ones keep their bits
        assert torch.equal(m.encoder_layers(x, tokens="cls"), full[:, :, :1])
        assert torch.equal(m.encoder_layers(x, tokens="patch"), full[:, :, 1:])
        # one layer asked alone (early stop), and a few in another order
        for i in (0, 5, 11):
            assert torch.equal(m.encoder_layers(x, [i])[:, 0], full[:, i]), i
        assert torch.equal(m.encoder_layers(x, [9, 2]), full[:, [9, 2]])
        # norm=True is sm_layernorm_f32 of the raw stream
        raw = m.encoder_layers(x, norm=False)
        e = m.encoder
        assert torch.equal(ops.layernorm(raw.reshape(-1, 384), e.norm.weight.detach(), e.norm.bias.detach(), 1e-6).view_as(full), full)
        assert torch.equal(m.encoder_layers(x, [3, 7], tokens="patch", norm=False), raw[:, [3, 7], 1:])
    finally:
        m.attention_path = "auto"


@pytest.mark.parametrize("path", ["fused", "unfused"])
def test_attention_of_every_block(peaky, path):
    fx, m, x = peaky
    m.attention_path = path
    try:
        e = m.encoder
        last = m.get_last_selfattention(x)
        a = e.forward_selfattention(x, return_interm_attn=True)
        assert a.shape == (12 * fx.B, 6, fx.n, fx.n)
        assert torch.equal(a[11 * fx.B:], last)  # block 12 through the new path: the bits last_attn gives
        assert torch.equal(e.forward_selfattention(x), last)
        assert torch.equal(e.forward_selfattention(x, return_interm_attn=True, cls_only=True), a[:, :, 0])
        assert torch.equal(e.forward_selfattention(x, cls_only=True), last[:, :, 0])
        # a subset, stopped inside block 6, together with token taps of earlier blocks
        t = m.encoder_taps(x, layers=[1, 4], attn_layers=[5, 2])
        assert torch.equal(t["attn"], a.view(12, fx.B, 6, fx.n, fx.n)[[2, 5]])
        assert torch.equal(t["tokens"], m.encoder_layers(x, [1, 4]))
        assert (a.sum(-1) - 1).abs().max() <= 1e-5
    finally:
        m.attention_path = "auto"


def test_encoder_methods_index_the_dict(peaky):
    fx, m, x = peaky
    e = m.encoder
    d = e(x)
    assert list(d) == [f"layer{i}" for i in range(1, 13)] and all(v.shape == (fx.B, fx.n, 384) for v in d.values())
    assert torch.equal(e(x, layer="layer7"), d["layer7"])
    assert torch.equal(e.forward_features(x), d["layer12"][:, 0])
    ref = R.layer_dict(torch.stack(list(d.values()), dim=1))
    assert torch.equal(m.forward_encoder(x), R.forward_encoder(ref))
    for layers, pt in ((None, False), ([0, 6, 11], True), ([11], False)):
        got = e.get_tokens(x, layers, patch_tokens=pt)
        want = torch.stack([d[f"layer{i + 1}"] for i in (range(12) if layers is None else layers)], dim=1)
        assert torch.equal(got, want if pt else want[:, :, 0])
    for n in (1, 4):
        assert torch.equal(e.forward_return_n_last_blocks(x, n), R.forward_return_n_last_blocks(ref, n))
        assert torch.equal(e.return_patch_emb_from_n_last_blocks(x, n), R.return_patch_emb_from_n_last_blocks(ref, n))
    pooled = e.forward_return_n_last_blocks(x, 2, return_patch_avgpool=True)
    assert pooled.shape == (fx.B, 3 * 384) and torch.equal(pooled[:, :768], R.forward_return_n_last_blocks(ref, 2))
    # the tokens in front of the blocks: post_pe is what block 1 starts from, input_tokens has no position table in it
    pre = e.get_tokens(x, [0], patch_tokens=True, norm=False, input_tokens=True, post_pe=True)
    assert pre.shape == (fx.B, 3, fx.n, 384)
    assert torch.equal(pre[:, 2], m.encoder_layers(x, [0], norm=False)[:, 0])
    pos = e.pos_embed.detach()  # 224^2 at P = 16: the table as trained, no interpolation
    # input + pos against the epilogue's own sum: each side rounds at most twice, 4 * 2^-24 (|input| + |pos|) covers both
    assert ((pre[:, 0] + pos - pre[:, 1]).abs() <= 2.0 ** -22 * (pre[:, 0].abs() + pos.abs())).all()
    assert torch.equal(e.get_tokens(x, [], input_tokens=True, post_pe=True), pre[:, :2, 0])


# ---- the tap changes nothing else --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["fused", "unfused"])
def test_forward_tap_changes_nothing_else(peaky, path):
    fx, m, x = peaky
    m.attention_path = path
    try:
        base = {k: v.clone() for k, v in m(x).items()}
        stack = m.encoder_layers(x)
        tap = m(x, return_layers=range(12))
        assert set(tap) == set(base) | {"encoder_layers"}
        for k in ("mask_pred", "objectness", "features"):
            assert torch.equal(tap[k], base[k]), k
        assert torch.equal(tap["encoder_layers"], stack)
        some = m(x, return_layers=[8, 3], return_logits=True, return_attention="cls")
        assert torch.equal(some["encoder_layers"], stack[:, [8, 3]]) and torch.equal(some["mask_pred"], base["mask_pred"])
        assert torch.equal(some["patch_tokens"], stack[:, 11, 1:])
        # stopped calls of every kind in between, then a plain forward: the workspace is in no other state than before
        m.encoder.get_tokens(x, [2], input_tokens=True, post_pe=True)
        m.encoder.forward_return_n_last_blocks(x, 2, return_patch_avgpool=True)
        m.encoder_taps(x, attn_layers=[0, 7], attn="cls")
        again = m(x)
        assert set(again) == set(base) and all(torch.equal(again[k], base[k]) for k in base)
    finally:
        m.attention_path = "auto"


def test_graph_replay_is_untouched_by_tapped_calls(peaky):
    fx, m, x = peaky
    m.attention_path = "fused"
    try:
        gf = GraphedForward(m, admit_after=0)
        first = {k: v.clone() for k, v in gf(x).items()}
        assert gf.failed is None and gf.captures == 1
        tapped = gf(x, return_layers=[5, 11])  # asks for taps: runs eagerly, outside the cache
        assert gf.captures == 1 and tapped["encoder_layers"].shape == (fx.B, 2, fx.n, 384)
        assert all(torch.equal(tapped[k], first[k]) for k in first)
        replay = gf(x)
        assert gf.captures == 1 and gf.replays >= 2 and set(replay) == set(first)
        assert all(torch.equal(replay[k], first[k]) for k in first)
    finally:
        m.attention_path = "auto"


# ---- batch invariance on a pinned path ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", [1, 2])
def test_batch_invariance(peaky, path):
    _fx, m, _x = peaky
    x3 = torch.from_numpy(synthetic_images(77, (3, 3, 224, 224))).to(DEV)
    kw = dict(layers=None, patch_mean=True, attn_layers=[0, 6, 11], attn_path=path)
    t3, t1 = m.encoder_taps(x3, **kw), m.encoder_taps(x3[1:2].contiguous(), **kw)
    assert torch.equal(t3["tokens"][1:2], t1["tokens"])
    assert torch.equal(t3["patch_mean"][1:2], t1["patch_mean"])
    assert torch.equal(t3["attn"][:, 1:2], t1["attn"])


# ---- small shapes against the fp64 restatement (no fixture) ------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _small(H, W):
    """B = 3 at P = 8: the restatement in fp64 and fp32, and the per-layer bars 4 * |fp32 - fp64| they give"""
    sd = synthetic_state_dict(21, "calib", patch_size=8)
    x = torch.from_numpy(synthetic_images(31, (3, 3, H, W)))
    r64, r32 = R.encoder_taps(x, sd, 8, torch.float64, attn="none"), R.encoder_taps(x, sd, 8, torch.float32, attn="none")
    return sd, x, r64, r32


# 72 x 88: N = 100 (the variant tests' shape); 56 x 72: n = 63, N = 64 - the patch count is no multiple of the tap kernel's four rows per
# wave nor of its sixteen per workgroup
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("H,W", [(72, 88), (56, 72)])
def test_small_shapes_against_fp64_restatement(H, W, mode):
    sd, x, r64, r32 = _small(H, W)
    m = _model(8, 21, "calib", mode)
    xd = x.to(DEV)
    n_tok = (H // 8) * (W // 8) + 1
    ok = True
    for path in (1, 2):
        for tokens, sel in (("all", slice(None)), ("patch", slice(1, None))):
            got = m.encoder_layers(xd, tokens=tokens, attn_path=path).cpu().double()
            want = r64["normed"][:, :, sel]
            assert got.shape == want.shape == (3, 12, n_tok if tokens == "all" else n_tok - 1, 384)
            bar = 4.0 * (r32["normed"][:, :, sel].double() - want).abs().amax(dim=(0, 2, 3))
            d = (got - want).abs().amax(dim=(0, 2, 3))
            print(f"\n[{mode} path {path}] {H}x{W} {tokens}: hip-r64 / (4 |r32-r64|) per layer {np.round((d / bar).numpy(), 2).tolist()}")
            ledger.record("encoder_taps", f"small_{H}x{W}|{mode}|path{path}|{tokens}", {"ratio_to_bound_per_layer": (d / bar).tolist()})
            ok = ok and bool((d <= bar).all())
        # the tokens in front of the blocks, same rule
        pre = m.encoder_taps(xd, tokens="all", input_tokens=True, post_pe=True, attn_path=path)
        for k in ("input_tokens", "post_pe"):
            d = (pre[k].cpu().double() - r64[k]).abs().max().item()
            bar = 4.0 * (r32[k].double() - r64[k]).abs().max().item()
            print(f"[{mode} path {path}] {H}x{W} {k}: hip-r64 = {d:.2e}, bound {bar:.2e}")
            ok = ok and d <= bar
    assert ok


# ---- patch mean ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["p16_224_peaky", "p8_200x168_calib"])
def test_patch_mean_against_the_device_tokens(name):
    """Against the fp64 mean of the device's own normed patch tokens: summing n fp32 values in any order stays within
    n * 2^-24 * sum|x| of the exact sum, so the mean within n * 2^-24 * mean|x|, per column (the division adds half an ulp, far below)."""
    fx = _fixture(name)
    m = _model(fx.patch, fx.wseed, fx.style, "w16")
    x = fx.images().to(DEV)
    t = m.encoder_taps(x, layers=[11], tokens="patch", patch_mean=True)
    tok = t["tokens"][:, 0].cpu().double()  # (B, n, 384)
    n = tok.shape[1]
    assert n == fx.n - 1 and t["patch_mean"].shape == (fx.B, 384)
    d = (t["patch_mean"].cpu().double() - tok.mean(dim=1)).abs()
    bound = n * 2.0 ** -24 * tok.abs().mean(dim=1)
    print(f"\n{name}: n = {n}, worst |mean - mean64| / bound = {(d / bound).max().item():.3f}")
    assert (d <= bound).all()
    # the same bits beside another set of token taps
    assert torch.equal(m.encoder.forward_return_n_last_blocks(x, 1, return_patch_avgpool=True)[:, 384:], t["patch_mean"])


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals(peaky):
    _fx, m, x = peaky
    for bad in ([12], [-1], []):
        with pytest.raises(ValueError):
            m.encoder_layers(x, bad)
        with pytest.raises(ValueError):
            m(x, return_layers=bad)
    with pytest.raises(ValueError, match="encoder_only"):
        m(x, encoder_only=True, return_layers=[0])
    f16 = _model(16, 1, "peaky", "f16")
    for call in (lambda: f16.encoder_layers(x), lambda: f16(x, return_layers=[0]), lambda: f16.encoder(x),
                 lambda: f16.encoder.forward_selfattention(x, return_interm_attn=True)):
        with pytest.raises(RuntimeError, match="'f16'"):
            call()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.encoder_layers(x.cpu())
