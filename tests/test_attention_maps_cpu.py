"""CPU-only checks of the attention-map surface: the fp64 restatement (tests/_attention_ref.py) against the reference's own fp64
vectors, the validation of the new ABI fields (their layout: tests/test_abi_cpu.py), and the state_dict contract after the encoder
gained its method."""
import numpy as np
import pytest
import torch

import _attention_ref as R
from selfmask_amd import _native as N
from selfmask_amd import MaskFormer, state_shapes


@pytest.mark.parametrize("name", R.FIXTURES)
def test_fp64_restatement_matches_reference_fp64(name):
    """Both sides fp64 on probabilities <= 1 through 12 blocks: 1e-12 absolute is some 10^4 ulps of head-room."""
    fx = R.Fixture(name)
    a = R.last_selfattention(fx.images(), fx.state_dict(), fx.patch).numpy()
    assert a.shape == (fx.B, 6, fx.n, fx.n)
    d = fx.max_abs_vs_f64(a)
    print(f"\n{name}: restatement - ref64 = {d:.2e}; fixture ref32 - ref64 = {fx.bar:.2e}")
    assert d <= 1e-12
    # the fixture's own bar is what it says: |ref32 - ref64| over the stored fp32 entries never exceeds it
    d32 = np.abs(fx.cls_f32.astype(np.float64) - fx.cls_f64).max()
    if fx.rows:
        d32 = max(d32, np.abs(fx.rows_f32.astype(np.float64) - fx.rows_f64).max())
    assert d32 <= fx.bar
    assert np.abs(a.sum(-1) - 1).max() <= 1e-12


def _weights():
    w = N.Weights()
    w.patch, w.n_dec_layers, w.n_queries, w.pos_grid, w.gemm_mode = 16, 6, 20, 14, 0
    w.dec_kv_w = w.dec_kv_b = 256  # validation only looks at NULL-ness; nothing is launched
    return w


def test_forward_validation_of_attention_fields_without_gpu():
    lib = N.load()
    io = N.ForwardIO()
    io.x, io.B, io.H, io.W = 256, 1, 224, 224
    io.attn_only = 1
    assert lib.sm_maskformer_forward(_weights(), io, None, 0, None) == -1
    assert b"attn_only needs last_attn or last_attn_cls" in lib.sm_last_error()
    io.attn_only = 2
    assert lib.sm_maskformer_forward(_weights(), io, None, 0, None) == -1 and b"attn_only=2" in lib.sm_last_error()
    # with a pointer set, attn_only passes validation with every other output NULL: the next stop is the workspace check
    io.attn_only, io.last_attn_cls = 1, 256
    assert lib.sm_maskformer_forward(_weights(), io, None, 0, None) == -3
    # the one-MFMA diagnostic has no attention maps
    w = _weights()
    w.gemm_mode = 3
    for f in ("patch_s", "dec_kv_s", "ffn0_s", "ffn1_s"):
        setattr(w, f, 1.0)
    for i in range(N.ENC_DEPTH):
        for f in ("qkv_s", "proj_s", "fc1_s", "fc2_s"):
            setattr(w.enc[i], f, 1.0)
    for l in range(6):
        for f in ("sa_in_s", "sa_out_s", "ca_in_s", "ca_out_s", "lin1_s", "lin2_s"):
            setattr(w.dec[l], f, 1.0)
    assert lib.sm_maskformer_forward(w, io, None, 0, None) == -1 and b"gemm_mode 3" in lib.sm_last_error()
    # without the new fields a forward still asks for its outputs
    io = N.ForwardIO()
    io.x, io.B, io.H, io.W = 256, 1, 224, 224
    assert lib.sm_maskformer_forward(_weights(), io, None, 0, None) == -1 and b"null output" in lib.sm_last_error()


def test_kernel_argument_validation_without_gpu():
    lib = N.load()

    def args(**kw):
        a = N.AttnProbsArgs()
        a.Q, a.K, a.P = 256, 512, 1024
        a.sQb = a.sKb = 197 * 768
        a.sQr = a.sKr = 768
        a.batch, a.heads, a.n_q, a.n_k, a.q0, a.nq, a.scale = 1, 6, 197, 197, 0, 197, 0.125
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    for bad in ({"Q": None}, {"K": None}, {"P": None}):
        assert lib.sm_attention_probs_f16x2(args(**bad), None) == -1 and b"null pointer" in lib.sm_last_error()
    for bad in ({"sQr": 772}, {"sKr": 772}, {"sQb": 197 * 768 + 4}, {"sKb": 4}):
        assert lib.sm_attention_probs_f16x2(args(**bad), None) == -1 and b"multiples of 8" in lib.sm_last_error()
    for bad in ({"Q": 256 + 16}, {"K": 512 + 4}):
        assert lib.sm_attention_probs_f16x2(args(**bad), None) == -1 and b"32-B aligned" in lib.sm_last_error()
    assert lib.sm_attention_probs_f16x2(args(heads=7), None) == -1
    assert lib.sm_attention_probs_f16x2(args(n_k=0), None) == -1
    assert lib.sm_attention_probs_f16x2(args(q0=190, nq=8), None) == -1 and b"query range" in lib.sm_last_error()
    assert lib.sm_attention_probs_f16x2(args(nq=0), None) == -1
    assert lib.sm_attention_probs_f16x2(args(scale=0.0), None) == -1
    assert lib.sm_attention_probs_f16x2(args(sPb=5), None) == -1 and b"sPb" in lib.sm_last_error()


@pytest.mark.parametrize("patch,ubc", [(16, True), (8, False)])
def test_state_dict_unchanged_by_the_encoder_method(patch, ubc):
    m = MaskFormer(n_queries=20, patch_size=patch, n_decoder_layers=6, return_intermediate=ubc, use_binary_classifier=ubc)
    assert callable(m.encoder.get_last_selfattention)
    exp = state_shapes(20, patch, 6, ubc)
    assert list(m.state_dict().keys()) == list(exp.keys())
    if ubc:
        assert len(exp) == 267
    # the back-reference is no submodule and no parameter: the module tree is what it was
    assert all(mod is not m for name, mod in m.named_modules() if name)
    assert "_owner" not in dict(m.encoder.named_modules()) and not any("_owner" in k for k in m.state_dict())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.encoder.get_last_selfattention(torch.zeros(1, 3, 224, 224))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.get_last_selfattention(torch.zeros(1, 3, 224, 224), cls_only=True)
