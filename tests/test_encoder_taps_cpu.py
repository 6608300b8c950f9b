"""CPU-only checks of the encoder-taps surface: the restatement (tests/_encoder_taps_ref.py) against the reference's own vectors
(tests/golden/encoder_taps_*.npz) in fp64 and - under the rule the device has to meet - in fp32, the selection logic of every method of
``model.encoder`` against plain indexing of the reference's dict, and the validation of sm_maskformer_forward_taps (its layout:
tests/test_abi_cpu.py)."""
import functools
import types

import numpy as np
import pytest
import torch

import _encoder_taps_ref as R
from selfmask_amd import _native as N
from selfmask_amd import MaskFormer, synthetic_images, synthetic_state_dict
from selfmask_amd.maskformer import VisionTransformerParams


@functools.lru_cache(maxsize=None)
def _restated(name, dtype):
    fx = R.Fixture(name)
    torch.set_num_threads(8)
    return fx, R.encoder_taps(fx.images(), fx.state_dict(), fx.patch, dtype)


@pytest.mark.parametrize("name", R.FIXTURES)
def test_fp64_restatement_matches_reference_fp64(name):
    """Both sides fp64: 1e-12 absolute, the tolerance of the attention restatement (tokens here stay below 7 in magnitude)."""
    fx, t = _restated(name, torch.float64)
    assert t["normed"].shape == (fx.B, 12, fx.n, 384) and t["attn"].shape == (12, fx.B, 6, fx.n)
    d, da = fx.token_errors(t["normed"].numpy()), fx.attn_errors(t["attn"].numpy())
    dm = np.abs(t["normed"][:, -1, 1:].mean(dim=1).numpy() - fx.mean_f64).max()
    print(f"\n{name}: restatement - ref64: tokens {d.max():.2e}, attention {da.max():.2e}, patch mean {dm:.2e}")
    assert d.max() <= 1e-12 and da.max() <= 1e-12 and dm <= 1e-12
    # the fixture's bars are what they say: |ref32 - ref64| over the stored fp32 entries never exceeds them
    d32 = np.maximum(np.abs(fx.cls_f32 - fx.cls_f64).max(axis=(0, 2)), np.abs(fx.rows_f32 - fx.rows_f64).max(axis=(0, 2, 3)))
    assert (d32 <= fx.bar).all() and (np.abs(fx.attn_cls_f32 - fx.attn_cls_f64).max(axis=(1, 2, 3)) <= fx.attn_bar).all()
    assert np.abs(fx.mean_f32 - fx.mean_f64).max() <= fx.mean_bar


@pytest.mark.parametrize("name", R.FIXTURES)
def test_fp32_restatement_meets_the_device_rule(name):
    """max |fp32 - ref64| <= 4 * f32_vs_f64_maxabs per layer and per block: an independent fp32 evaluation meets the bar the GPU
    tests set, before the device is asked to."""
    fx, t = _restated(name, torch.float32)
    d, da = fx.token_errors(t["normed"].numpy()), fx.attn_errors(t["attn"].numpy())
    print(f"\n{name}: fp32 restatement / bar: tokens {(d / fx.bar).max():.2f}, attention {(da / fx.attn_bar).max():.2f} (bar 4)")
    assert (d <= 4.0 * fx.bar).all(), d / fx.bar
    assert (da <= 4.0 * fx.attn_bar).all(), da / fx.attn_bar


# ---- selection logic: the product's methods over a CPU stand-in for the device call ----------------------------------------------
@pytest.fixture(scope="module")
def staged():
    """A MaskFormer whose ``encoder_taps`` (the one device call under every method) is served by the fp64 restatement in the layout
    the device gives: what is checked is the Python around it."""
    patch, B = 16, 2
    sd = synthetic_state_dict(3, "soft", patch_size=patch)
    x = torch.from_numpy(synthetic_images(11, (B, 3, 64, 48)))
    taps = R.encoder_taps(x, sd, patch, torch.float64, attn="full")
    m = MaskFormer(n_queries=20, patch_size=patch, n_decoder_layers=6, return_intermediate=True, use_binary_classifier=True)
    calls = []

    def fake(self, x_, layers=(), tokens="all", norm=True, post_pe=False, input_tokens=False, patch_mean=False, attn_layers=(),
             attn="full", attn_path=0, workspace=None):
        lay = [] if layers is not None and len(list(layers)) == 0 else self._check_layers(layers)
        alay = [] if attn_layers is not None and len(list(attn_layers)) == 0 else self._check_layers(attn_layers, "attn_layers")
        calls.append((sorted(set(lay)), tokens, sorted(set(alay))))
        sel = {"all": slice(None), "cls": slice(0, 1), "patch": slice(1, None)}[tokens]
        out = {}
        if lay:
            out["tokens"] = taps["normed" if norm else "raw"][:, sorted(set(lay))][:, :, sel]
        if post_pe:
            out["post_pe"] = taps["post_pe"][:, sel]
        if input_tokens:
            out["input_tokens"] = taps["input_tokens"][:, sel]
        if patch_mean:
            out["patch_mean"] = taps["normed"][:, -1, 1:].mean(dim=1)
        if alay:
            a = taps["attn"][sorted(set(alay))]
            out["attn"] = a[:, :, :, 0] if attn == "cls" else a
        return out

    m.encoder_taps = types.MethodType(fake, m)
    return m, x, taps, R.layer_dict(taps["normed"]), calls


def test_encoder_call_is_the_reference_dict(staged):
    m, x, taps, d, calls = staged
    out = m.encoder(x)
    assert list(out) == [f"layer{i}" for i in range(1, 13)]
    assert all(out[k].shape == (2, 13, 384) and torch.equal(out[k], d[k]) for k in d)
    del calls[:]
    assert torch.equal(m.encoder(x, layer="layer7"), d["layer7"])
    assert calls == [([6], "all", [])]  # one block asked: the device stops after it
    with pytest.raises(KeyError):
        m.encoder(x, layer="layer13")
    assert torch.equal(m.forward_encoder(x), R.forward_encoder(d)) and m.forward_encoder(x).shape == (2, 12, 384, 12)


def test_encoder_layers_order_and_selection(staged):
    m, x, taps, d, _ = staged
    assert torch.equal(m.encoder_layers(x), taps["normed"])
    got = m.encoder_layers(x, [7, 2, 11], tokens="patch")  # 0-based, in the order asked
    assert got.shape == (2, 3, 12, 384)
    assert all(torch.equal(got[:, k], d[f"layer{i + 1}"][:, 1:]) for k, i in enumerate([7, 2, 11]))
    assert torch.equal(m.encoder_layers(x, [0], tokens="cls", norm=False), taps["raw"][:, :1, :1])
    for bad in ([12], [-1], [], [3, 12]):
        with pytest.raises(ValueError):
            m.encoder_layers(x, bad)


@pytest.mark.parametrize("layers", [None, [11], [0, 5], [9, 3, 3]])
@pytest.mark.parametrize("patch_tokens", [False, True])
def test_get_tokens_stacking_order(staged, layers, patch_tokens):
    m, x, taps, _, _ = staged
    for norm, inp, pe in [(True, False, False), (False, True, False), (True, False, True), (False, True, True)]:
        got = m.encoder.get_tokens(x, layers, patch_tokens=patch_tokens, norm=norm, input_tokens=inp, post_pe=pe)
        want = R.get_tokens(taps, layers, patch_tokens, norm, inp, pe)
        assert got.shape == want.shape and torch.equal(got, want), (layers, patch_tokens, norm, inp, pe)
    k = 12 if layers is None else len(set(layers))
    assert m.encoder.get_tokens(x, layers, patch_tokens=patch_tokens).shape == ((2, k, 13, 384) if patch_tokens else (2, k, 384))


def test_get_tokens_without_blocks_and_refusals(staged):
    m, x, taps, _, _ = staged
    got = m.encoder.get_tokens(x, [], patch_tokens=True, input_tokens=True, post_pe=True)
    assert torch.equal(got, torch.stack([taps["input_tokens"], taps["post_pe"]], dim=1))
    for bad in ([], [12], [-1]):
        with pytest.raises(ValueError):
            m.encoder.get_tokens(x, bad)


@pytest.mark.parametrize("n", [1, 4, 12])
def test_n_last_blocks(staged, n):
    m, x, taps, d, _ = staged
    e = m.encoder
    assert torch.equal(e.forward_return_n_last_blocks(x, n), R.forward_return_n_last_blocks(d, n))
    got = e.forward_return_n_last_blocks(x, n, return_patch_avgpool=True)
    assert got.shape == (2, 384 * n + 384) and torch.equal(got, R.forward_return_n_last_blocks(d, n, True))
    got = e.return_patch_emb_from_n_last_blocks(x, n)
    assert got.shape == (2, 12, 384, n) and torch.equal(got, R.return_patch_emb_from_n_last_blocks(d, n))
    with pytest.raises(ValueError, match="torch.stack cannot succeed"):
        e.return_patch_emb_from_n_last_blocks(x, n, return_patch_avgpool=True)


def test_features_selfattention_and_n_range(staged):
    m, x, taps, d, _ = staged
    e = m.encoder
    assert torch.equal(e.forward_features(x), d["layer12"][:, 0]) and e.forward_features(x).shape == (2, 384)
    a = e.forward_selfattention(x, return_interm_attn=True)
    assert a.shape == (24, 6, 13, 13) and torch.equal(a, torch.cat(list(taps["attn"]), dim=0))  # blocks along dim 0
    assert torch.equal(e.forward_selfattention(x, return_interm_attn=True, cls_only=True), a[:, :, 0])
    for bad in (0, 13):
        with pytest.raises(ValueError):
            e.forward_return_n_last_blocks(x, bad)
        with pytest.raises(ValueError):
            e.return_patch_emb_from_n_last_blocks(x, bad)


def test_encoder_without_owner_raises():
    e = VisionTransformerParams(patch_size=16)
    x = torch.zeros(1, 3, 32, 32)
    calls = [lambda: e(x), lambda: e.get_tokens(x, [0]), lambda: e.forward_features(x), lambda: e.forward_return_n_last_blocks(x),
             lambda: e.return_patch_emb_from_n_last_blocks(x), lambda: e.forward_selfattention(x, True), lambda: e.get_last_selfattention(x)]
    for call in calls:
        with pytest.raises(RuntimeError, match="parameter container"):
            call()


def test_refusals_before_any_launch():
    m = MaskFormer(n_queries=20, patch_size=16, n_decoder_layers=6, return_intermediate=True, use_binary_classifier=True)
    x = torch.zeros(1, 3, 32, 32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.encoder_layers(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.encoder(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(x, return_layers=[0])
    with pytest.raises(ValueError, match="encoder_only"):
        m(x, encoder_only=True, return_layers=[0])
    for bad in ([12], [-1], []):
        with pytest.raises(ValueError):
            m(x, return_layers=bad)
    with pytest.raises(ValueError):
        m.encoder_layers(x, tokens="rows")
    with pytest.raises(ValueError, match="nothing requested"):
        m.encoder_taps(x)
    f16 = MaskFormer(n_queries=20, patch_size=16, n_decoder_layers=6, return_intermediate=True, use_binary_classifier=True, gemm_mode="f16")
    with pytest.raises(RuntimeError, match="'f16'"):
        f16._new_taps(1, 5, "cpu", [0])
    # the encoder gained methods, not state: the module tree and the state_dict are what they were
    assert "_owner" not in dict(m.encoder.named_modules()) and len(m.state_dict()) == 267


# ---- sm_maskformer_forward_taps: validation happens on the host before any launch -------------------------------------------------
def _weights(mode=0):
    w = N.Weights()
    w.patch, w.n_dec_layers, w.n_queries, w.pos_grid, w.gemm_mode = 16, 6, 20, 14, mode
    w.dec_kv_w = w.dec_kv_b = 256  # validation only looks at NULL-ness; nothing is launched
    if mode >= 2:
        for f in ("patch_s", "dec_kv_s", "ffn0_s", "ffn1_s"):
            setattr(w, f, 1.0)
        for i in range(N.ENC_DEPTH):
            for f in ("qkv_s", "proj_s", "fc1_s", "fc2_s"):
                setattr(w.enc[i], f, 1.0)
        for l in range(6):
            for f in ("sa_in_s", "sa_out_s", "ca_in_s", "ca_out_s", "lin1_s", "lin2_s"):
                setattr(w.dec[l], f, 1.0)
    return w


def _io(outputs=False):
    io = N.ForwardIO()
    io.x, io.B, io.H, io.W = 256, 1, 224, 224
    if outputs:
        io.mask_pred = io.objectness = io.features = 256
    return io


def _taps(**kw):
    t = N.EncoderTaps()
    t.layer_mask, t.tokens, t.norm, t.stop = 0b100000, 256, 1, 1
    for k, v in kw.items():
        setattr(t, k, v)
    return t


def test_taps_validation_without_gpu():
    lib = N.load()
    call = lambda t, io=None, w=None: lib.sm_maskformer_forward_taps(w or _weights(), io or _io(), t, None, 0, None)  # noqa: E731
    # a well-formed stopped request passes validation with every output of sm_forward_io NULL: the next stop is the workspace check
    assert call(_taps()) == -3
    assert call(_taps(layer_mask=0, tokens=None, attn_mask=1 << 11, attn_cls=256)) == -3
    assert call(_taps(layer_mask=0, tokens=None, patch_mean=256)) == -3
    for mode in (1, 2):
        assert call(_taps(), w=_weights(mode)) == -3
    # taps == NULL is sm_maskformer_forward
    assert call(None) == -1 and b"null output" in lib.sm_last_error()
    assert call(None, _io(True)) == lib.sm_maskformer_forward(_weights(), _io(True), None, 0, None) == -3
    # without stop the forward's own outputs are still asked for
    assert call(_taps(stop=0)) == -1 and b"null output" in lib.sm_last_error()
    assert call(_taps(stop=0), _io(True)) == -3
    # refusals
    assert call(_taps(layer_mask=0, tokens=None)) == -1 and b"nothing requested" in lib.sm_last_error()
    assert call(_taps(layer_mask=1 << 12)) == -1 and b"layer_mask" in lib.sm_last_error()
    assert call(_taps(attn_mask=1 << 12, attn=256)) == -1 and b"attn_mask" in lib.sm_last_error()
    assert call(_taps(attn_mask=1 << 31, attn=256)) == -1
    assert call(_taps(tokens=None)) == -1 and b"layer_mask and tokens" in lib.sm_last_error()
    assert call(_taps(attn_mask=1)) == -1 and b"attn_mask and attn" in lib.sm_last_error()
    assert call(_taps(layer_mask=0)) == -1  # a destination without its mask
    assert call(_taps(attn=256)) == -1
    for bad in ({"select": 3}, {"select": -1}, {"norm": 2}, {"stop": 2}):
        assert call(_taps(**bad)) == -1, bad
    assert call(_taps(tokens=260)) == -1 and b"16-B aligned" in lib.sm_last_error()
    assert call(_taps(), w=_weights(3)) == -1 and b"gemm_mode 3" in lib.sm_last_error()
    io = _io()
    io.attn_only, io.last_attn_cls = 1, 256
    assert call(_taps(), io) == -1 and b"attn_only with taps" in lib.sm_last_error()
    io = _io()
    io.last_attn = 256
    assert call(_taps(), io) == -1 and b"stop with last_attn" in lib.sm_last_error()
