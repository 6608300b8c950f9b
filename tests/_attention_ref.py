"""fp64 restatement of the last encoder block's attention matrix - VisionTransformer.get_last_selfattention
(vision_transformer.py:307-314): blocks 1-11, then norm1 -> qkv -> softmax(q k^T * scale) of block 12 (Attention.forward :113-123).
Built from oracle.selfmask_oracle's own pieces; checked against the reference's fp64 vectors in test_attention_maps_cpu.py, and the
witness for shapes that have no fixture."""
import glob
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle import selfmask_oracle as O
from selfmask_amd import synthetic_images, synthetic_state_dict

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ["p16_224_peaky", "p16_224_soft", "p16_250x333_peaky", "p8_200x168_calib"]


@torch.no_grad()
def last_selfattention(x: torch.Tensor, sd, patch: int, dtype=torch.float64) -> torch.Tensor:
    """(B, 6, N, N) post-softmax attention of block 12, evaluated in ``dtype``."""
    sd = O.cast_state(sd, dtype)
    t, _grid = O.prepare_tokens(x.to(dtype), sd, patch)
    for i in range(11):
        t = O.encoder_block(t, sd, i)
    p = "encoder.blocks.11."
    y = F.layer_norm(t, (O.D,), sd[p + "norm1.weight"], sd[p + "norm1.bias"], 1e-6)
    B, N, _ = y.shape
    qkv = O._lin(y, sd, p + "attn.qkv").reshape(B, N, 3, O.H, O.DH).permute(2, 0, 3, 1, 4)
    return ((qkv[0] @ qkv[1].transpose(-2, -1)) * (O.DH ** -0.5)).softmax(dim=-1)


class Fixture:
    """One tests/golden/attention_<name>.npz (scripts/gen_attention_golden.py): the reference's own fp32 / fp64 results."""

    def __init__(self, name: str):
        g = np.load(os.path.join(GOLD, f"attention_{name}.npz"))
        self.name = name
        self.patch, self.B, self.H, self.W, self.wseed, self.xseed, _ = [int(v) for v in g["meta"]]
        self.style = str(g["style"])
        self.n = int(g["n_tokens"])
        self.bar = float(g["f32_vs_f64_maxabs"])  # |ref32 - ref64| over exactly the stored entries
        self.cls_f32, self.cls_f64 = g["cls_f32"], g["cls_f64"]
        self.rows = [int(r) for r in g["rows"]] if "rows" in g else []
        self.rows_f32 = g["rows_f32"] if self.rows else None
        self.rows_f64 = g["rows_f64"] if self.rows else None
        self.full_f64 = None  # image 0, (6, N, N)
        parts = sorted(glob.glob(os.path.join(GOLD, f"attention_{name}_full_h*.npz")))
        if parts:
            full = np.zeros((6, self.n, self.n))
            for fp in parts:
                h = np.load(fp)
                full[h["heads"]] = h["full_f64"]
            self.full_f64 = full

    def state_dict(self):
        return synthetic_state_dict(self.wseed, self.style, patch_size=self.patch)

    def images(self) -> torch.Tensor:
        return torch.from_numpy(synthetic_images(self.xseed, (self.B, 3, self.H, self.W)))

    def max_abs_vs_f64(self, attn) -> float:
        """max |attn - ref64| over exactly the entries the fixture stores; attn (B, 6, N, N), numpy or a CPU tensor."""
        a = np.asarray(attn, dtype=np.float64)
        assert a.shape == (self.B, 6, self.n, self.n), a.shape
        d = np.abs(a[:, :, 0] - self.cls_f64).max()
        if self.rows:
            d = max(d, np.abs(a[:, :, self.rows] - self.rows_f64).max())
        if self.full_f64 is not None:
            d = max(d, np.abs(a[0] - self.full_f64).max())
        return float(d)
