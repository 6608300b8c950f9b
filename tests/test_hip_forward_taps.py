"""The timing taps of the forward (sm_forward_timing / sm_forward_timing_read, through the C ABI): how many launches each kernel
name collects in one forward.  The counts follow from the model's structure and the documented path rules
(sm_forward_io.attn_path, sm_weights.ln_fold), not from a measurement."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from selfmask_amd import MaskFormer, synthetic_state_dict, synthetic_images  # noqa: E402
from selfmask_amd import _native as N  # noqa: E402

DEV = "cuda:0"
LN, ATTN, FUSED = "layernorm384_kernel", "attention_f16x2_kernel<4, false>", "qkv_attention_m16_kernel<2, 3, 4>"
# GEMMs of one forward at L = 6: patch embedding, 12 x (proj, fc1, fc2), all-layer K/V, 6 x (sa_in, sa_out, ca_in, ca_out, lin1, lin2),
# mask einsum, 2 objectness layers - plus the 12 qkv projections where they are launches of their own
GEMMS = 1 + 36 + 1 + 36 + 1 + 2


@pytest.fixture(scope="module")
def models():
    x = torch.from_numpy(synthetic_images(11, (1, 3, 224, 224))).to(DEV)
    out = {}
    for pre in (False, True):
        m = MaskFormer(n_queries=20, patch_size=16, n_decoder_layers=6, normalize_before=pre, return_intermediate=True,
                       use_binary_classifier=True, gemm_mode="w16")
        m.load_state_dict(synthetic_state_dict(0, "calib", patch_size=16), strict=True)
        out[pre] = m.to(DEV)
    return x, out


def _forward(m, x, path):
    m.attention_path = path
    try:
        out = m(x, return_logits=True)
        torch.cuda.synchronize()
    finally:
        m.attention_path = "auto"
    return out


@pytest.mark.parametrize("path,pre,n_ln,n_gemm,n_attn,n_fused", [
    # 24 encoder pre-norms + final norm; post-norm decoder: 3 per layer (the shared final norm is chained onto norm3)
    ("fused", False, 24 + 1 + 3 * 6, GEMMS, 12, 12),
    ("fused", True, 24 + 1 + 4 * 6, GEMMS, 12, 12),            # pre-norm decoder: norm1-3 and the shared final norm are launches
    ("unfused", False, 1 + 1 + 18, GEMMS + 12, 24, 0),          # pre-norms folded: block 0's norm1 and the final norm remain
    ("auto", False, 1 + 11 + 1 + 18, GEMMS + 12, 24, 0),        # B = 1: folded norm2, split-K fc2 + the norm that sums it (11 blocks)
], ids=["fused-post", "fused-pre", "unfused-post", "auto-post"])
def test_tap_counts_of_one_forward(models, path, pre, n_ln, n_gemm, n_attn, n_fused):
    x, by_norm = models
    m, lib = by_norm[pre], N.load()
    before = _forward(m, x, path)
    N.check(lib.sm_forward_timing(1), "sm_forward_timing")
    try:
        _forward(m, x, path)
        buf = (N.KernelTime * 64)()
        n = lib.sm_forward_timing_read(buf, 64)
    finally:
        lib.sm_forward_timing(0)
    assert n > 0, lib.sm_last_error().decode()
    taps = {buf[k].name.decode(): buf[k] for k in range(n)}
    count = {name: t.launches for name, t in taps.items()}
    print(f"\n {path} pre={pre}: {count}")
    assert count[LN] == n_ln
    assert sum(v for k, v in count.items() if k.startswith("gemm_")) == n_gemm
    assert count[ATTN] == n_attn
    assert count.get(FUSED, 0) == n_fused
    for name, t in taps.items():
        assert t.total_us >= 0, name
        if name.startswith("gemm_") or "attention" in name:
            assert t.flops > 0, name
    assert lib.sm_forward_timing_read(buf, 64) == 0   # switched off: the taps are gone ...
    after = _forward(m, x, path)
    assert lib.sm_forward_timing_read(buf, 64) == 0   # ... and a forward records none
    for k in before:
        assert torch.equal(before[k], after[k]), k
