"""fp64 / fp32 restatement of the encoder's per-block outputs - VisionTransformer.forward's dict layer1 .. layer12
(vision_transformer.py:293-304), every block's attention (Block.forward(return_attention=True) :164-167) and the selections the DINO
feature-extraction family makes of them (get_tokens :316-357, forward_features :359-375, forward_return_n_last_blocks :448-471,
return_patch_emb_from_n_last_blocks :473-497, forward_selfattention :403-446, MaskFormer.forward_encoder maskformer.py:99-113), all on
prepare_tokens' tokens.  Built from oracle.selfmask_oracle's own pieces; checked against the reference's vectors in
test_encoder_taps_cpu.py, and the witness for shapes that have no fixture."""
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle import selfmask_oracle as O
from selfmask_amd import synthetic_images, synthetic_state_dict

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ["p16_224_peaky", "p16_224_soft", "p16_250x333_peaky", "p8_200x168_calib"]
DEPTH = 12


def _norm(t, sd):
    return F.layer_norm(t, (O.D,), sd["encoder.norm.weight"], sd["encoder.norm.bias"], 1e-6)


@torch.no_grad()
def encoder_taps(x: torch.Tensor, sd, patch: int, dtype=torch.float64, attn: str = "cls") -> dict:
    """Everything the taps can give, evaluated in ``dtype``:
    "input_tokens", "post_pe" (B, N, 384); "raw", "normed" (B, 12, N, 384): the residual stream after every block and
    encoder.norm of it; "attn": every block's post-softmax attention, (12, B, 6, N, N) for attn="full", its row 0 (12, B, 6, N) for
    "cls", absent for "none"."""
    sd = O.cast_state(sd, dtype)
    x = x.to(dtype)
    post_pe, grid = O.prepare_tokens(x, sd, patch)
    pos = O.interpolate_pos_encoding(sd["encoder.pos_embed"], grid)
    emb = F.conv2d(O.make_input_divisible(x, patch), sd["encoder.patch_embed.proj.weight"], sd["encoder.patch_embed.proj.bias"],
                   stride=patch).flatten(2).transpose(1, 2)
    out = {"input_tokens": torch.cat((sd["encoder.cls_token"].expand(x.shape[0], -1, -1), emb), dim=1), "post_pe": post_pe,
           "pos": pos}
    t, raw, maps = post_pe, [], []
    B, N, _ = t.shape
    for i in range(DEPTH):
        if attn != "none":
            p = f"encoder.blocks.{i}."
            y = F.layer_norm(t, (O.D,), sd[p + "norm1.weight"], sd[p + "norm1.bias"], 1e-6)
            qkv = O._lin(y, sd, p + "attn.qkv").reshape(B, N, 3, O.H, O.DH).permute(2, 0, 3, 1, 4)
            a = ((qkv[0] @ qkv[1].transpose(-2, -1)) * (O.DH ** -0.5)).softmax(dim=-1)
            maps.append(a[:, :, 0] if attn == "cls" else a)
        t = O.encoder_block(t, sd, i)
        raw.append(t)
    out["raw"] = torch.stack(raw, dim=1)
    out["normed"] = _norm(out["raw"], sd)
    if maps:
        out["attn"] = torch.stack(maps)
    return out


# ---- the reference's methods as selections of its dict {"layer1": (B, N, 384), ...} (plain indexing: the witness of the product's
# selection logic) ----------------------------------------------------------------------------------------------------------------
def layer_dict(normed: torch.Tensor) -> dict:
    return {f"layer{i + 1}": normed[:, i] for i in range(DEPTH)}


def get_tokens(taps: dict, layers, patch_tokens=False, norm=True, input_tokens=False, post_pe=False) -> torch.Tensor:
    """vision_transformer.py:326-357 on the restatement's tensors"""
    lst = ([taps["input_tokens"]] if input_tokens else []) + ([taps["post_pe"]] if post_pe else [])
    for i in range(DEPTH):
        if layers is None or i in layers:
            lst.append(taps["normed" if norm else "raw"][:, i])
    tokens = torch.stack(lst, dim=1)
    return tokens if patch_tokens else tokens[:, :, 0, :]


def forward_return_n_last_blocks(d: dict, n=1, return_patch_avgpool=False) -> torch.Tensor:
    out = [d[f"layer{i + 1}"][:, 0] for i in range(DEPTH) if DEPTH - i <= n]
    if return_patch_avgpool:
        out.append(torch.mean(d[f"layer{DEPTH}"][:, 1:], dim=1))
    return torch.cat(out, dim=-1)


def return_patch_emb_from_n_last_blocks(d: dict, n=1) -> torch.Tensor:
    return torch.stack([d[f"layer{i + 1}"][:, 1:] for i in range(DEPTH) if DEPTH - i <= n], dim=-1)


def forward_encoder(d: dict) -> torch.Tensor:
    return torch.stack([d[f"layer{i + 1}"][:, 1:, :] for i in range(DEPTH)], dim=0).permute(1, 0, 3, 2)


class Fixture:
    """One tests/golden/encoder_taps_<name>.npz (scripts/gen_encoder_taps_golden.py): the reference's own fp32 / fp64 results."""

    def __init__(self, name: str):
        g = np.load(os.path.join(GOLD, f"encoder_taps_{name}.npz"))
        self.name = name
        self.patch, self.B, self.H, self.W, self.wseed, self.xseed, _ = [int(v) for v in g["meta"]]
        self.style = str(g["style"])
        self.n = int(g["n_tokens"])
        self.bar = g["f32_vs_f64_maxabs"]            # (12,) |ref32 - ref64| per layer over exactly the stored token entries
        self.attn_bar = g["attn_f32_vs_f64_maxabs"]  # (12,) per block, over the CLS attention rows
        self.mean_bar = float(g["mean_f32_vs_f64_maxabs"])
        self.rows = [int(r) for r in g["rows"]]
        for k in ("cls_f32", "cls_f64", "rows_f32", "rows_f64", "mean_f32", "mean_f64", "attn_cls_f32", "attn_cls_f64"):
            setattr(self, k, g[k])
        self.full_layer, self.full_f64 = None, None  # image 0's whole (N, 384) matrix of one layer (1-based)
        fp = os.path.join(GOLD, f"encoder_taps_{name}_layer6.npz")
        if os.path.exists(fp):
            h = np.load(fp)
            self.full_layer, self.full_f64 = int(h["layer"]), h["full_f64"]

    def state_dict(self):
        return synthetic_state_dict(self.wseed, self.style, patch_size=self.patch)

    def images(self) -> torch.Tensor:
        return torch.from_numpy(synthetic_images(self.xseed, (self.B, 3, self.H, self.W)))

    def token_errors(self, tokens) -> np.ndarray:
        """(12,) max |tokens - ref64| per layer over exactly the entries the fixture stores; tokens (B, 12, N, 384)."""
        t = np.asarray(tokens, dtype=np.float64)
        assert t.shape == (self.B, DEPTH, self.n, O.D), t.shape
        d = np.maximum(np.abs(t[:, :, 0] - self.cls_f64).max(axis=(0, 2)), np.abs(t[:, :, self.rows] - self.rows_f64).max(axis=(0, 2, 3)))
        if self.full_f64 is not None:
            k = self.full_layer - 1
            d[k] = max(d[k], np.abs(t[0, k] - self.full_f64).max())
        return d

    def attn_errors(self, attn_cls) -> np.ndarray:
        """(12,) max |row 0 - ref64| per block; attn_cls (12, B, 6, N)."""
        a = np.asarray(attn_cls, dtype=np.float64)
        assert a.shape == self.attn_cls_f64.shape, a.shape
        return np.abs(a - self.attn_cls_f64).max(axis=(1, 2, 3))
