#!/usr/bin/env python3
"""Generate tests/golden/encoder_taps_*.npz: every block's tokens and CLS attention of the REAL reference encoder on the CPU.

Usage (from the repository root, on the build machine that has the reference checkout):
    python scripts/gen_encoder_taps_golden.py

The reference is imported through oracle.gen_golden (_import_reference / build_reference_model, used as they are); this script holds
none of its text.  Inputs are the synthetic checkpoints and images of the forward fixtures (the seeds and styles of
oracle.gen_golden.FORWARD_CASES, the four cases of the attention fixtures), so the tests re-generate them from the seeds.

Tokens come from ``model.encoder(x)`` - the dict layer1 .. layer12 of final-normed block outputs (vision_transformer.py:293-304) -
evaluated in fp32 and in fp64.  Stored in both:
  cls_f32 / cls_f64            (B, 12, 384)     the CLS row of every layer
  rows, rows_f32 / rows_f64    (4,), (B, 12, 4, 384)  four patch rows (token indices: first, second, middle, last patch)
  mean_f32 / mean_f64          (B, 384)         mean over the patch rows of layer 12
  f32_vs_f64_maxabs            (12,)            per layer, max |fp32 - fp64| over exactly the token entries the fixture stores
  mean_f32_vs_f64_maxabs       ()               the same for the patch mean
Attention comes from the reference's own blocks called with return_attention=True (:164-167) on ``prepare_tokens(x)`` (:269-281),
block after block:
  attn_cls_f32 / attn_cls_f64  (12, B, 6, N)    row 0 of every block's post-softmax attention
  attn_f32_vs_f64_maxabs       (12,)            per block
The peaky 224^2 case also stores image 0's whole fp64 token matrix of layer 6 in a file of its own
(encoder_taps_<name>_layer6.npz: full_f64 (N, 384)); layer 6's bar then covers it too.
"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from oracle import gen_golden as G  # noqa: E402

CASES = {"p16_224_peaky": True, "p16_224_soft": False, "p16_250x333_peaky": False, "p8_200x168_calib": False}  # name -> layer 6 in full
DEPTH, FULL_LAYER = 12, 6


@torch.no_grad()
def run(model, x):
    """(tokens (B, 12, N, 384), CLS attention rows (12, B, 6, N)) in the model's dtype, returned as fp64"""
    enc = model.encoder
    out = enc(x)
    tokens = torch.stack([out[f"layer{i + 1}"] for i in range(DEPTH)], dim=1)
    t, rows = enc.prepare_tokens(x), []
    for blk in enc.blocks:
        rows.append(blk(t, return_attention=True)[:, :, 0])
        t = blk(t)
    assert torch.equal(enc.norm(t), out[f"layer{DEPTH}"])  # the loop walked the same stream
    return tokens.double(), torch.stack(rows).double()


def main():
    _vits, mf = G._import_reference()
    torch.set_num_threads(G.N_THREADS)
    forward = {c[0]: c for c in G.FORWARD_CASES}
    for name, full in CASES.items():
        _, patch, (B, Hh, Ww), wseed, style, xseed, _ = forward[name]
        sd = G.synthetic_state_dict(wseed, style, patch_size=patch)
        x = torch.from_numpy(G.synthetic_images(xseed, (B, 3, Hh, Ww)))
        t32, a32 = run(G.build_reference_model(mf, patch, sd), x)
        t64, a64 = run(G.build_reference_model(mf, patch, sd, torch.float64), x.double())
        n = t64.shape[2]
        assert t64.shape == (B, DEPTH, n, 384) and a64.shape == (DEPTH, B, 6, n)
        rows = [1, 2, n // 2, n - 1]
        idx = torch.tensor([0] + rows)
        err = (t32 - t64)[:, :, idx].abs().amax(dim=(0, 2, 3))
        if full:
            err[FULL_LAYER - 1] = max(err[FULL_LAYER - 1], (t32 - t64)[0, FULL_LAYER - 1].abs().max())
            fp = os.path.join(G.GOLD, f"encoder_taps_{name}_layer{FULL_LAYER}.npz")
            np.savez_compressed(fp, layer=np.array(FULL_LAYER), full_f64=t64[0, FULL_LAYER - 1].numpy())
            print(f"  {os.path.basename(fp)}: {os.path.getsize(fp) / 1e6:.2f} MB")
        m32, m64 = t32[:, -1, 1:].float().mean(dim=1).double(), t64[:, -1, 1:].mean(dim=1)
        ridx = torch.tensor(rows)
        save = dict(meta=np.array([patch, B, Hh, Ww, wseed, xseed, G.N_THREADS]), style=np.array(style), n_tokens=np.array(n),
                    cls_f32=t32[:, :, 0].float().numpy(), cls_f64=t64[:, :, 0].numpy(), rows=np.array(rows),
                    rows_f32=t32[:, :, ridx].float().numpy(), rows_f64=t64[:, :, ridx].numpy(),
                    mean_f32=m32.float().numpy(), mean_f64=m64.numpy(), f32_vs_f64_maxabs=err.numpy(),
                    mean_f32_vs_f64_maxabs=np.array((m32 - m64).abs().max().item()),
                    attn_cls_f32=a32.float().numpy(), attn_cls_f64=a64.numpy(),
                    attn_f32_vs_f64_maxabs=(a32 - a64).abs().amax(dim=(1, 2, 3)).numpy())
        fp = os.path.join(G.GOLD, f"encoder_taps_{name}.npz")
        np.savez_compressed(fp, **save)
        print(f"{name}: N={n} max|token|={t64.abs().max().item():.2f} token f32-f64 per layer {err.min().item():.2e}..{err.max().item():.2e} "
              f"attention {save['attn_f32_vs_f64_maxabs'].min():.2e}..{save['attn_f32_vs_f64_maxabs'].max():.2e} "
              f"-> {os.path.getsize(fp) / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
