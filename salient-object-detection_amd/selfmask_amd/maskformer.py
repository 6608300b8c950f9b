"""Host-side mirror of the reference's ``networks.maskformer.maskformer.MaskFormer`` (maskformer.py:11-251).

Same constructor arguments, same 267-tensor ``state_dict`` (so ``selfmask_nq20.pt`` loads unchanged), same
``forward(x, encoder_only=False, skip_decoder=False) -> dict``; the arithmetic runs in libselfmask_hip.so.
The sub-modules below are parameter containers only (they give the parameters the reference's names); they hold no
arithmetic of their own.  ``model.encoder`` carries the reference's call surface (the per-layer dict, get_tokens, ...) and
delegates every call to the MaskFormer that owns it.
"""
from math import ceil
from typing import Dict, Optional

import torch
import torch.nn as nn

from . import _native as N


class _Mlp(nn.Module):  # vision_transformer.py:78-94
    def __init__(self, d, hidden):
        super().__init__()
        self.fc1 = nn.Linear(d, hidden)
        self.fc2 = nn.Linear(hidden, d)


class _Attention(nn.Module):  # vision_transformer.py:97-133
    def __init__(self, d):
        super().__init__()
        self.qkv = nn.Linear(d, 3 * d, bias=True)
        self.proj = nn.Linear(d, d)


class _Block(nn.Module):  # vision_transformer.py:136-170
    def __init__(self, d, hidden):
        super().__init__()
        self.norm1 = nn.LayerNorm(d, eps=1e-6)
        self.attn = _Attention(d)
        self.norm2 = nn.LayerNorm(d, eps=1e-6)
        self.mlp = _Mlp(d, hidden)


class _PatchEmbed(nn.Module):  # vision_transformer.py:173-188
    def __init__(self, patch, d):
        super().__init__()
        self.proj = nn.Conv2d(3, d, kernel_size=patch, stride=patch)


class VisionTransformerParams(nn.Module):
    """Parameter container with the attributes callers read off ``model.encoder``."""

    def __init__(self, patch_size: int = 16, embed_dim: int = N.EMBED, depth: int = N.ENC_DEPTH,
                 num_heads: int = N.HEADS, mlp_ratio: int = 4):
        super().__init__()
        self.patch_embed = _PatchEmbed(patch_size, embed_dim)
        n0 = (224 // patch_size) ** 2  # PatchEmbed is always built for 224x224 (vision_transformer.py:213-218)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, n0 + 1, embed_dim))
        self.blocks = nn.ModuleList([_Block(embed_dim, embed_dim * mlp_ratio) for _ in range(depth)])
        self.norm = nn.LayerNorm(embed_dim, eps=1e-6)
        nn.init.trunc_normal_(self.pos_embed, std=.02)
        nn.init.trunc_normal_(self.cls_token, std=.02)
        self.depth = depth
        self.embed_dim = self.n_embs = embed_dim
        self.mlp_ratio = mlp_ratio
        self.n_heads = num_heads
        self.patch_size = patch_size

    def _need_owner(self, what: str):
        owner = self.__dict__.get("_owner")
        if owner is None:
            raise RuntimeError(f"this encoder is a parameter container: {what} needs the MaskFormer that owns it")
        return owner

    def get_last_selfattention(self, x: torch.Tensor) -> torch.Tensor:
        """vision_transformer.py:307-314: the post-softmax attention of the last block, (B, heads, N, N) with N = 1 + gh*gw.
        The arithmetic lives in the owning MaskFormer's forward (``MaskFormer.get_last_selfattention``)."""
        return self._need_owner("get_last_selfattention").get_last_selfattention(x)

    # ---- the DINO feature-extraction family (vision_transformer.py:293-497).  Every method is a selection of what the device taps
    # give (MaskFormer.encoder_taps); all of them are defined on prepare_tokens' tokens (:269-281): the input zero-padded to the patch
    # size, the position table interpolated to the token grid.  get_tokens, forward_features, forward_return_n_last_blocks and
    # return_patch_emb_from_n_last_blocks call interpolate_pos_encoding without its `size` argument in the reference and raise there:
    # what is built is their evident intent, selections of the dict forward() returns.
    def forward(self, x: torch.Tensor, layer: Optional[str] = None):
        """vision_transformer.py:293-304: the dict ``layer1 .. layer12`` of (B, N, 384) final-normed block outputs (views of one
        (B, 12, N, 384) stack), or the one tensor for ``layer="layer7"`` (the encoder then stops after that block)."""
        owner = self._need_owner("forward")
        names = [f"layer{i + 1}" for i in range(self.depth)]
        if layer is not None:
            if layer not in names:
                raise KeyError(layer)
            return owner.encoder_layers(x, [names.index(layer)])[:, 0]
        stack = owner.encoder_layers(x)
        return {name: stack[:, i] for i, name in enumerate(names)}

    def get_tokens(self, x: torch.Tensor, layers, patch_tokens: bool = False, norm: bool = True, input_tokens: bool = False,
                   post_pe: bool = False) -> torch.Tensor:
        """vision_transformer.py:316-357.  ``layers``: 0-based block indices (None: all twelve), taken in ascending order as the
        reference's ``i in layers`` does.  Stacked along dim 1 in the reference's order: the input tokens (before the position
        embedding), the post-PE tokens, then the blocks.  ``patch_tokens=False`` returns the CLS rows (B, k, 384), True ALL tokens
        (B, k, N, 384) - the reference's naming."""
        owner = self._need_owner("get_tokens")
        if layers is not None and len(list(layers)) == 0 and (input_tokens or post_pe):
            idx = []  # only the tokens in front of the blocks
        else:
            idx = sorted(set(owner._check_layers(layers)))  # refuses an empty list: the reference's torch.stack of nothing raises too
        t = owner.encoder_taps(x, layers=idx, tokens="all" if patch_tokens else "cls", norm=norm, input_tokens=input_tokens,
                               post_pe=post_pe)
        parts = [t[k].unsqueeze(1) for k in ("input_tokens", "post_pe") if k in t] + ([t["tokens"]] if idx else [])
        out = parts[0] if len(parts) == 1 else torch.cat(parts, dim=1)
        return out if patch_tokens else out[:, :, 0, :]

    def forward_features(self, x: torch.Tensor) -> torch.Tensor:
        """vision_transformer.py:359-375: the final-normed CLS token, (B, 384)."""
        return self._need_owner("forward_features").encoder_layers(x, [self.depth - 1], tokens="cls")[:, 0, 0]

    def forward_return_n_last_blocks(self, x: torch.Tensor, n: int = 1, return_patch_avgpool: bool = False) -> torch.Tensor:
        """vision_transformer.py:448-471: the normed CLS tokens of the ``n`` last blocks side by side, (B, 384 n), with
        ``return_patch_avgpool`` followed by the mean of block 12's normed patch tokens, (B, 384 n + 384)."""
        owner = self._need_owner("forward_return_n_last_blocks")
        if not 1 <= n <= self.depth:
            raise ValueError(f"n={n}: 1..{self.depth} last blocks")
        t = owner.encoder_taps(x, layers=range(self.depth - n, self.depth), tokens="cls", patch_mean=return_patch_avgpool)
        out = t["tokens"].reshape(x.shape[0], n * self.embed_dim)
        return torch.cat((out, t["patch_mean"]), dim=-1) if return_patch_avgpool else out

    def return_patch_emb_from_n_last_blocks(self, x: torch.Tensor, n: int = 1, return_patch_avgpool: bool = False) -> torch.Tensor:
        """vision_transformer.py:473-497: the normed patch tokens of the ``n`` last blocks, (B, n_patches, 384, n)."""
        owner = self._need_owner("return_patch_emb_from_n_last_blocks")
        if return_patch_avgpool:
            raise ValueError("return_patch_avgpool=True: the reference appends a (B, 384) mean to (B, n_patches, 384) tensors and its "
                             "torch.stack cannot succeed; take the mean from forward_return_n_last_blocks")
        if not 1 <= n <= self.depth:
            raise ValueError(f"n={n}: 1..{self.depth} last blocks")
        return owner.encoder_layers(x, range(self.depth - n, self.depth), tokens="patch").permute(0, 2, 3, 1)

    def forward_selfattention(self, x: torch.Tensor, return_interm_attn: bool = False, cls_only: bool = False) -> torch.Tensor:
        """vision_transformer.py:403-446.  False: the last block's attention (``get_last_selfattention``); True: every block's,
        (12 B, 6, N, N), blocks concatenated along dim 0 as the reference does (``cls_only``: row 0 only, (.., 6, N)).
        Defined on prepare_tokens' tokens like every other method here.  Off 224 x 224 the reference's own method differs: it
        interpolates the position table with ``scale_factor=`` instead of ``size=`` (other sampling positions) and does not pad
        the input to the patch size."""
        owner = self._need_owner("forward_selfattention")
        if not return_interm_attn:
            return owner.get_last_selfattention(x, cls_only=cls_only)
        t = owner.encoder_taps(x, attn_layers=range(self.depth), attn="cls" if cls_only else "full")
        return t["attn"].flatten(0, 1)

    def make_input_divisible(self, x: torch.Tensor) -> torch.Tensor:
        """vision_transformer.py:260-267 (shape helper for callers; the HIP im2col pads implicitly)."""
        h0, w0 = x.shape[-2:]
        pad_w = (self.patch_size - w0 % self.patch_size) % self.patch_size
        pad_h = (self.patch_size - h0 % self.patch_size) % self.patch_size
        return nn.functional.pad(x, (0, pad_w, 0, pad_h), value=0)


class _DecoderLayer(nn.Module):  # transformer_decoder.py:229-258
    def __init__(self, d, heads, hidden):
        super().__init__()
        self.self_attn = nn.MultiheadAttention(d, heads, dropout=0.0)
        self.multihead_attn = nn.MultiheadAttention(d, heads, dropout=0.0)
        self.linear1 = nn.Linear(d, hidden)
        self.linear2 = nn.Linear(hidden, d)
        self.norm1 = nn.LayerNorm(d)
        self.norm2 = nn.LayerNorm(d)
        self.norm3 = nn.LayerNorm(d)


class _Decoder(nn.Module):  # transformer_decoder.py:104-111
    def __init__(self, d, heads, hidden, n_layers):
        super().__init__()
        self.layers = nn.ModuleList([_DecoderLayer(d, heads, hidden) for _ in range(n_layers)])
        self.norm = nn.LayerNorm(d)
        self.num_layers = n_layers


class _MLPHead(nn.Module):  # maskformer.py:254-268
    def __init__(self, d_in, d_hidden, d_out, num_layers):
        super().__init__()
        h = [d_hidden] * (num_layers - 1)
        self.num_layers = num_layers
        self.layers = nn.ModuleList(nn.Linear(n, k) for n, k in zip([d_in] + h, h + [d_out]))


class MaskFormer(nn.Module):
    def __init__(
            self,
            n_queries: int = 100,
            arch: str = "vit_small",
            patch_size: int = 8,
            training_method: str = "dino",
            n_decoder_layers: int = 6,
            normalize_before: bool = False,
            return_intermediate: bool = False,
            learnable_pixel_decoder: bool = False,
            lateral_connection: bool = False,
            scale_factor: int = 2,
            abs_2d_pe_init: bool = False,
            use_binary_classifier: bool = False,
            *,
            gemm_mode: Optional[str] = None,
    ):
        """Same arguments as the reference.  ``gemm_mode`` (extra, keyword-only) picks the GEMM back end:
        "w16" (default; f16 matrix cores, split operands, weights pre-scaled per tensor so every weight GEMM sums in ONE
        fp32 accumulator - fp32-grade results), "f16x2" (the same arithmetic with two accumulators and unscaled weights)
        or "fp32" (exact fp32 MFMA).  "f16" is the throughput-mode DIAGNOSTIC of SURVEY.md 7.2 (b): the w16 kernels with ONE
        f16 MFMA per product (plain f16 operands, fp32 accumulate, fp32 LayerNorm / softmax statistics, fp32-grade mask
        einsum) - two orders of magnitude outside the 1e-4 logit gate, reported beside the metric, never as it.  The
        environment variable SM_GEMM_MODE overrides the default."""
        super().__init__()
        if arch != "vit_small":
            raise NotImplementedError(f"arch={arch!r}: only the DINO ViT-S encoder is on the MI355X hot path "
                                      f"(resnet50 backbones are out of scope, SURVEY.md section 2 #11)")
        if patch_size not in (8, 16):
            raise ValueError(f"patch_size={patch_size}: ViT-S/8 and ViT-S/16 are supported")
        if int(scale_factor) != scale_factor or not 1 <= scale_factor <= 16:
            raise ValueError(f"scale_factor={scale_factor}: an integer 1..16 (maskformer.py:161 passes it to F.interpolate)")
        # learnable_pixel_decoder is stored and never read by the reference's forward (maskformer.py:71,144-162): accepted,
        # no effect.  lateral_connection=True is accepted here as there and fails in forward as there (see forward()).
        if not 1 <= n_decoder_layers <= N.MAX_DEC_LAYERS:
            raise ValueError(f"n_decoder_layers={n_decoder_layers} (1..{N.MAX_DEC_LAYERS})")
        d = N.EMBED
        # NB: unlike utils/misc.py:196,243 no remote DINO weights are fetched; the checkpoint overwrites them anyway.
        self.encoder = VisionTransformerParams(patch_size=patch_size)
        # back-reference for encoder.get_last_selfattention, kept out of nn.Module's registries (no submodule cycle, no
        # state_dict entries)
        self.encoder.__dict__["_owner"] = self
        self.decoder = _Decoder(d, N.HEADS, d * self.encoder.mlp_ratio, n_decoder_layers)
        self.query_embed = nn.Embedding(n_queries, d).weight  # registered as parameter "query_embed"
        if use_binary_classifier:
            self.ffn = _MLPHead(d, d, 1, num_layers=3)
        else:
            self.ffn = _MLPHead(d, d, d, num_layers=3)
            self.linear_classifier = nn.Linear(d, 2)
            self.norm = nn.LayerNorm(d)
        self.arch = arch
        self.use_binary_classifier = use_binary_classifier
        self.lateral_connection = lateral_connection
        self.learnable_pixel_decoder = learnable_pixel_decoder
        self.scale_factor = int(scale_factor)
        self.normalize_before = bool(normalize_before)  # TransformerDecoderLayer.forward_pre (transformer_decoder.py:299-327)
        self.return_intermediate = return_intermediate
        self.n_queries = n_queries
        self.n_decoder_layers = n_decoder_layers
        import os
        self.gemm_mode = gemm_mode or os.environ.get("SM_GEMM_MODE", "w16")
        if self.gemm_mode not in ("w16", "f16x2", "fp32", "f16"):
            raise ValueError(f"gemm_mode={self.gemm_mode!r}: 'w16', 'f16x2', 'fp32' (or the 'f16' throughput-mode diagnostic)")
        # encoder kernel set (sm_forward_io.attn_path): "auto" = by batch size - from 16 images up the fused QKV + attention
        # kernel with LayerNorm launches, below that the GEMM + attention pair with the pre-norms folded into the GEMMs around them
        # (each set where it is faster); "fused" / "unfused" pin the large- / small-batch set - the two differ in the last bits,
        # so a caller that compares results across batch sizes bit for bit (the Evaluator) pins one for the whole run
        self.attention_path = "auto"
        # folded pre-norms available to the small-batch set (sm_weights.ln_fold; w16 / f16 modes): 23 launches fewer per forward
        # there, same results to rounding.  SM_LN_FOLD=0 in the environment keeps the LayerNorm launches everywhere (A/B runs).
        self.ln_fold = os.environ.get("SM_LN_FOLD", "1") != "0"
        self._table = None       # (Weights struct, key) cache
        self._packed = None      # tensors derived from the state_dict (kept alive here, rebuilt when weights change)
        self.weights_generation = 0  # bumped whenever the packed weights are dropped: captured hipGraphs hold raw
                                     # pointers into them, graphs.GraphedForward destroys its graphs when this changes
        self._workspace = {}     # (device, stream) -> uint8 tensor sized for the largest forward that stream has run
        self.register_load_state_dict_post_hook(lambda module, incompatible_keys: module.refresh_packed())
        self.eval()

    # ---- weight pointer table -------------------------------------------------------------------------------
    def _apply(self, fn, *a, **kw):  # .to() / .cuda() / .float() move storage: drop cached pointers
        self._table = None
        self._packed = None
        self._workspace = {}
        self.weights_generation = getattr(self, "weights_generation", 0) + 1
        return super()._apply(fn, *a, **kw)

    def refresh_packed(self):
        """Drop the weight pointer table and the packed (derived) weights; call after editing parameters in place.
        ``load_state_dict`` and ``.to()`` do it automatically."""
        self._table = None
        self._packed = None
        self.weights_generation += 1

    def _weights(self) -> N.Weights:
        key = (self.query_embed.data_ptr(), self.ffn.layers[2].bias.data_ptr(), self.encoder.pos_embed.data_ptr(),
               self.gemm_mode, self.ln_fold)
        if self._table is not None and self._table[1] == key:
            return self._table[0]
        if self._table is not None:  # a knob changed (gemm_mode, ln_fold): the packed tensors are rebuilt below and graphs
            self.weights_generation += 1  # captured over the old ones hold dangling pointers
        for n_, p in self.named_parameters():
            if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
                raise RuntimeError(f"parameter {n_} must be a contiguous float32 tensor on a HIP device "
                                   f"(got {p.device}, {p.dtype}); the product path has no CPU fallback")
        w = N.Weights()
        e = self.encoder
        split = self.gemm_mode in ("f16x2", "w16", "f16")
        w16 = self.gemm_mode in ("w16", "f16")
        packed = {}
        d = N.EMBED
        # cross-attention K/V projections of all layers packed into one (L*768, 384) weight: rows [384:1152) of each
        # multihead_attn.in_proj_weight (transformer_decoder.py:283-289 with key = value = memory)
        packed["dec_kv_w"] = torch.cat([lay.multihead_attn.in_proj_weight.detach()[d:] for lay in self.decoder.layers]).contiguous()
        packed["dec_kv_b"] = torch.cat([lay.multihead_attn.in_proj_bias.detach()[d:] for lay in self.decoder.layers]).contiguous()

        def gws(name: str, t: torch.Tensor):
            """(pointer, 2^-s) of a GEMM weight: the tensor itself (fp32 mode), its F16X2 copy (f16x2 mode) or its W16
            copy with the per-tensor power-of-two scale (w16 mode)"""
            t2 = t.detach().reshape(t.shape[0], -1)
            if not split:
                return t2.data_ptr(), 0.0
            from . import ops
            if w16:
                packed["s:" + name], scale = ops.split_w16(t2.contiguous())
                return packed["s:" + name].data_ptr(), scale
            packed["s:" + name] = ops.split_f16x2(t2.contiguous())
            return packed["s:" + name].data_ptr(), 0.0

        def fold(name: str, lin, norm):
            """LayerNorm folded into the Linear it feeds (sm_weights.ln_fold): W16 copy of W diag(gamma), the folded bias
            b + W beta, and the row sums of the gain-scaled weight AS ROUNDED to W16 (hi + lo, times 2^-s) - the epilogue
            subtracts mu times that sum from what the MFMAs accumulated over exactly those rounded values."""
            from . import ops
            t, scale, packed["b:" + name], packed["c:" + name] = ops.fold_layernorm(
                lin.weight.detach(), lin.bias.detach(), norm.weight.detach(), norm.bias.detach())
            packed["f:" + name] = t
            return t.data_ptr(), scale, packed["b:" + name].data_ptr(), packed["c:" + name].data_ptr()

        w.query_embed = self.query_embed.data_ptr()
        w.cls_token = e.cls_token.data_ptr()
        w.pos_embed = e.pos_embed.data_ptr()
        w.patch_w, w.patch_s = gws("patch_w", e.patch_embed.proj.weight)
        w.patch_b = e.patch_embed.proj.bias.data_ptr()
        for i, blk in enumerate(e.blocks):
            L = w.enc[i]
            L.norm1_w, L.norm1_b = blk.norm1.weight.data_ptr(), blk.norm1.bias.data_ptr()
            (L.qkv_w, L.qkv_s), L.qkv_b = gws(f"enc{i}.qkv", blk.attn.qkv.weight), blk.attn.qkv.bias.data_ptr()
            (L.proj_w, L.proj_s), L.proj_b = gws(f"enc{i}.proj", blk.attn.proj.weight), blk.attn.proj.bias.data_ptr()
            L.norm2_w, L.norm2_b = blk.norm2.weight.data_ptr(), blk.norm2.bias.data_ptr()
            (L.fc1_w, L.fc1_s), L.fc1_b = gws(f"enc{i}.fc1", blk.mlp.fc1.weight), blk.mlp.fc1.bias.data_ptr()
            (L.fc2_w, L.fc2_s), L.fc2_b = gws(f"enc{i}.fc2", blk.mlp.fc2.weight), blk.mlp.fc2.bias.data_ptr()
            if w16 and self.ln_fold:
                L.fc1_fw, L.fc1_fs, L.fc1_fb, L.fc1_c = fold(f"enc{i}.fc1", blk.mlp.fc1, blk.norm2)
                if i > 0:  # block 0's norm1 stays a launch (its input comes from the patch embedding)
                    L.qkv_fw, L.qkv_fs, L.qkv_fb, L.qkv_c = fold(f"enc{i}.qkv", blk.attn.qkv, blk.norm1)
        w.enc_norm_w, w.enc_norm_b = e.norm.weight.data_ptr(), e.norm.bias.data_ptr()
        for j, lay in enumerate(self.decoder.layers):
            L = w.dec[j]
            (L.sa_in_w, L.sa_in_s), L.sa_in_b = gws(f"dec{j}.sa_in", lay.self_attn.in_proj_weight), lay.self_attn.in_proj_bias.data_ptr()
            (L.sa_out_w, L.sa_out_s), L.sa_out_b = gws(f"dec{j}.sa_out", lay.self_attn.out_proj.weight), lay.self_attn.out_proj.bias.data_ptr()
            # only rows [0:384) (the query projection) of the cross-attention in_proj are used through this pointer;
            # the K/V rows travel in dec_kv_w with their own scale
            (L.ca_in_w, L.ca_in_s), L.ca_in_b = gws(f"dec{j}.ca_in", lay.multihead_attn.in_proj_weight[:d]), lay.multihead_attn.in_proj_bias.data_ptr()
            L.ca_out_w, L.ca_out_s = gws(f"dec{j}.ca_out", lay.multihead_attn.out_proj.weight)
            L.ca_out_b = lay.multihead_attn.out_proj.bias.data_ptr()
            (L.lin1_w, L.lin1_s), L.lin1_b = gws(f"dec{j}.lin1", lay.linear1.weight), lay.linear1.bias.data_ptr()
            (L.lin2_w, L.lin2_s), L.lin2_b = gws(f"dec{j}.lin2", lay.linear2.weight), lay.linear2.bias.data_ptr()
            L.norm1_w, L.norm1_b = lay.norm1.weight.data_ptr(), lay.norm1.bias.data_ptr()
            L.norm2_w, L.norm2_b = lay.norm2.weight.data_ptr(), lay.norm2.bias.data_ptr()
            L.norm3_w, L.norm3_b = lay.norm3.weight.data_ptr(), lay.norm3.bias.data_ptr()
        w.dec_norm_w, w.dec_norm_b = self.decoder.norm.weight.data_ptr(), self.decoder.norm.bias.data_ptr()
        f = self.ffn.layers
        (w.ffn0_w, w.ffn0_s), w.ffn0_b = gws("ffn0", f[0].weight), f[0].bias.data_ptr()
        (w.ffn1_w, w.ffn1_s), w.ffn1_b = gws("ffn1", f[1].weight), f[1].bias.data_ptr()
        if self.use_binary_classifier:  # objectness MLP: the last layer is a (1, 384) row, applied as a row dot product
            w.ffn2_w, w.ffn2_b, w.mask_head_ffn = f[2].weight.data_ptr(), f[2].bias.data_ptr(), 0
        else:  # 384 -> 384 mask head (maskformer.py:59-66): a GEMM weight like the others; used on the 5-D path only
            (w.ffn2_w, w.ffn2_s), w.ffn2_b = gws("ffn2", f[2].weight), f[2].bias.data_ptr()
            w.mask_head_ffn = 1 if self.return_intermediate else 0
            w.no_objectness = 1  # no binary classifier: forward.hip stops before the objectness tail
        (w.dec_kv_w, w.dec_kv_s), w.dec_kv_b = gws("dec_kv", packed["dec_kv_w"]), packed["dec_kv_b"].data_ptr()
        w.gemm_mode = 3 if self.gemm_mode == "f16" else 2 if w16 else (1 if split else 0)
        w.normalize_before = 1 if self.normalize_before else 0
        w.ln_fold = 1 if (w16 and self.ln_fold) else 0
        w.scale_factor = self.scale_factor
        self._packed = packed
        w.patch = e.patch_size
        w.pos_grid = int(round((e.pos_embed.shape[1] - 1) ** 0.5))
        w.n_queries = self.n_queries
        w.n_dec_layers = self.n_decoder_layers
        # the ~90 split kernels above ran on the current stream; forwards on OTHER streams (streams.StreamRing) reuse this
        # table without an event dependency on it, so finish the packing here, once per weight generation
        torch.cuda.current_stream(self.query_embed.device).synchronize()
        self._table = (w, key)
        return w

    def new_workspace(self, x: torch.Tensor) -> torch.Tensor:
        """A private scratch buffer for forwards of x's shape (for callers that keep several forwards in flight or
        capture the forward into a hipGraph: pass it as ``forward(x, workspace=...)``)."""
        B, _, H, W = x.shape
        nbytes = N.load().sm_forward_workspace_bytes(self._weights(), B, H, W)
        if nbytes == 0:
            raise RuntimeError("sm_forward_workspace_bytes returned 0 (bad shape)")
        return torch.empty(nbytes, dtype=torch.uint8, device=x.device)

    def _get_workspace(self, w: N.Weights, x: torch.Tensor) -> torch.Tensor:
        """One scratch buffer per STREAM (batches in flight on different streams must not share scratch; the forwards of one
        stream run one after the other), grown to the largest forward that stream has seen and never shrunk: native-resolution
        evaluation walks ~50 token grids on three streams, and a buffer per (shape, stream) - round 2 cleared the cache, round 3
        first kept the 12 most recent - turned every batch into a free + malloc of a different size (the same evaluation ran
        at 2.3 k or at 3.4 k images/s depending on what the allocator's cache held).  A smaller forward uses a prefix."""
        B, _, H, W = x.shape
        nbytes = N.load().sm_forward_workspace_bytes(w, B, H, W)
        if nbytes == 0:
            raise RuntimeError("sm_forward_workspace_bytes returned 0 (bad shape)")
        k = (x.device, torch.cuda.current_stream().cuda_stream)
        ws = self._workspace.get(k)
        if ws is None or ws.numel() < nbytes:
            ws = self._workspace[k] = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        return ws

    # ---- forward ----------------------------------------------------------------------------------------------
    _ATTN_PATHS = {"auto": 0, "fused": 1, "unfused": 2}

    @torch.no_grad()
    def get_last_selfattention(self, x: torch.Tensor, cls_only: bool = False, attn_path=0,
                               workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
        """VisionTransformer.get_last_selfattention (vision_transformer.py:307-314): the post-softmax attention matrix of the last
        encoder block, (B, 6, N, N) with N = 1 + gh*gw - or, with ``cls_only``, only row 0 (the CLS token's attention over all
        tokens) as (B, 6, N), the same bits as ``[:, :, 0, :]`` of the full result.  The forward stops right after writing it
        (sm_forward_io.attn_only).  ``attn_path``: the encoder kernel set of blocks 1-11 (0 / "auto": the model's
        ``attention_path``; 1 / "fused"; 2 / "unfused")."""
        if not x.is_cuda:
            raise RuntimeError("MaskFormer (MI355X) needs its input on a HIP device; there is no CPU fallback")
        if self.gemm_mode == "f16":
            raise RuntimeError("attention maps are not available in the 'f16' throughput-mode diagnostic")
        lib = N.load()
        x = x.contiguous().float()
        B, c, H, W = x.shape
        assert c == 3, "expected an RGB image batch (B,3,H,W)"
        p = self.encoder.patch_size
        n_tok = ceil(H / p) * ceil(W / p) + 1
        w = self._weights()
        ws = workspace if workspace is not None else self._get_workspace(w, x)
        io = N.ForwardIO()
        io.x, io.B, io.H, io.W = x.data_ptr(), B, H, W
        path = self._ATTN_PATHS.get(attn_path, attn_path)
        if path not in (0, 1, 2):
            raise ValueError(f"attn_path={attn_path!r}: 0 / 'auto', 1 / 'fused' or 2 / 'unfused'")
        io.attn_path = path if path else self._ATTN_PATHS[self.attention_path]
        io.attn_only = 1
        if cls_only:
            out = torch.empty((B, N.HEADS, n_tok), device=x.device, dtype=torch.float32)
            io.last_attn_cls = out.data_ptr()
        else:
            out = torch.empty((B, N.HEADS, n_tok, n_tok), device=x.device, dtype=torch.float32)
            io.last_attn = out.data_ptr()
        N.check(lib.sm_maskformer_forward(w, io, ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream),
                "sm_maskformer_forward")
        return out

    # ---- encoder taps (sm_encoder_taps) ---------------------------------------------------------------------
    _TAP_SELECT = {"all": N.TAP_ALL, "cls": N.TAP_CLS, "patch": N.TAP_PATCH}

    def _check_layers(self, layers, what: str = "layers"):
        """0-based block indices as a list; None = all twelve.  Empty, 12 and -1 are refused."""
        idx = list(range(N.ENC_DEPTH)) if layers is None else [int(i) for i in layers]
        if not idx:
            raise ValueError(f"{what} is empty: name at least one block (0..{N.ENC_DEPTH - 1})")
        bad = [i for i in idx if not 0 <= i < N.ENC_DEPTH]
        if bad:
            raise ValueError(f"{what}={bad}: 0-based block indices 0..{N.ENC_DEPTH - 1}")
        return idx

    def _check_tap_args(self, tokens: str = "all", attn: str = "full"):
        if self.gemm_mode == "f16":
            raise RuntimeError("encoder taps are not available in the 'f16' throughput-mode diagnostic")
        if tokens not in self._TAP_SELECT:
            raise ValueError(f"tokens={tokens!r}: 'all', 'cls' or 'patch'")
        if attn not in ("full", "cls"):
            raise ValueError(f"attn={attn!r}: 'full' or 'cls'")

    def _new_taps(self, B: int, n_tok: int, dev, layers=(), tokens: str = "all", norm: bool = True, post_pe: bool = False,
                  input_tokens: bool = False, patch_mean: bool = False, attn_layers=(), attn: str = "full", stop: bool = True):
        """(sm_encoder_taps, {name: output tensor}) for one call.  Blocks are stacked in ASCENDING order whatever the order of
        ``layers`` / ``attn_layers`` (duplicates count once)."""
        self._check_tap_args(tokens, attn)
        t, out = N.EncoderTaps(), {}
        t.select, t.norm, t.stop = self._TAP_SELECT[tokens], 1 if norm else 0, 1 if stop else 0
        R = {"all": n_tok, "cls": 1, "patch": n_tok - 1}[tokens]
        new = lambda *shape: torch.empty(shape, device=dev, dtype=torch.float32)  # noqa: E731
        lay = sorted(set(layers))
        if lay:
            t.layer_mask = sum(1 << i for i in lay)
            out["tokens"] = new(B, len(lay), R, N.EMBED)
            t.tokens = out["tokens"].data_ptr()
        for name, want, shape in (("post_pe", post_pe, (B, R, N.EMBED)), ("input_tokens", input_tokens, (B, R, N.EMBED)),
                                  ("patch_mean", patch_mean, (B, N.EMBED))):
            if want:
                out[name] = new(*shape)
                setattr(t, name, out[name].data_ptr())
        alay = sorted(set(attn_layers))
        if alay:
            t.attn_mask = sum(1 << i for i in alay)
            if attn == "cls":
                out["attn"] = new(len(alay), B, N.HEADS, n_tok)
                t.attn_cls = out["attn"].data_ptr()
            else:
                out["attn"] = new(len(alay), B, N.HEADS, n_tok, n_tok)
                t.attn = out["attn"].data_ptr()
        return t, out

    @torch.no_grad()
    def encoder_taps(self, x: torch.Tensor, layers=(), tokens: str = "all", norm: bool = True, post_pe: bool = False,
                     input_tokens: bool = False, patch_mean: bool = False, attn_layers=(), attn: str = "full", attn_path=0,
                     workspace: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """Tokens and attention of any encoder blocks in one stopped forward (sm_maskformer_forward_taps with ``stop``): the encoder
        runs up to the last block asked for, the decoder not at all.  Returns the entries asked for:
        "tokens" (B, k, R, 384) - the outputs of the blocks ``layers`` (0-based, ascending), final-normed (``norm``) or the raw
        residual stream, R = N / 1 / n rows for ``tokens`` = "all" / "cls" / "patch"; "post_pe" and "input_tokens" (B, R, 384) - the
        stream after / before the position embedding; "patch_mean" (B, 384) - the mean of block 12's normed patch rows; "attn" -
        the post-softmax attention of the blocks ``attn_layers``, (k, B, 6, N, N) or with ``attn="cls"`` row 0 only, (k, B, 6, N).
        Everything is defined on prepare_tokens' tokens (input zero-padded to the patch size, position table interpolated to the
        grid).  ``attn_path`` as in ``get_last_selfattention``."""
        self._check_tap_args(tokens, attn)
        lay = [] if layers is not None and len(list(layers)) == 0 else self._check_layers(layers)  # () = none, None = all twelve
        alay = [] if attn_layers is not None and len(list(attn_layers)) == 0 else self._check_layers(attn_layers, "attn_layers")
        if not (lay or alay or post_pe or input_tokens or patch_mean):
            raise ValueError("encoder_taps: nothing requested")
        if not x.is_cuda:
            raise RuntimeError("MaskFormer (MI355X) needs its input on a HIP device; there is no CPU fallback")
        lib = N.load()
        x = x.contiguous().float()
        B, c, H, W = x.shape
        assert c == 3, "expected an RGB image batch (B,3,H,W)"
        p = self.encoder.patch_size
        n_tok = ceil(H / p) * ceil(W / p) + 1
        taps, out = self._new_taps(B, n_tok, x.device, lay, tokens, norm, post_pe, input_tokens, patch_mean, alay, attn, stop=True)
        w = self._weights()
        ws = workspace if workspace is not None else self._get_workspace(w, x)
        io = N.ForwardIO()
        io.x, io.B, io.H, io.W = x.data_ptr(), B, H, W
        path = self._ATTN_PATHS.get(attn_path, attn_path)
        if path not in (0, 1, 2):
            raise ValueError(f"attn_path={attn_path!r}: 0 / 'auto', 1 / 'fused' or 2 / 'unfused'")
        io.attn_path = path if path else self._ATTN_PATHS[self.attention_path]
        N.check(lib.sm_maskformer_forward_taps(w, io, taps, ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream),
                "sm_maskformer_forward_taps")
        return out

    def encoder_layers(self, x: torch.Tensor, layers=None, tokens: str = "all", norm: bool = True, attn_path=0,
                       workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
        """(B, len(layers), R, 384): the outputs of the encoder blocks ``layers`` (0-based indices as get_tokens uses them,
        vision_transformer.py:346-349; None = all twelve) in the order asked, through the final norm as VisionTransformer.forward's
        dict holds them (:299) or, ``norm=False``, the raw residual stream.  ``tokens``: "all" (R = N), "cls" (R = 1) or "patch"
        (R = n).  The encoder stops after the last block asked for."""
        idx = self._check_layers(layers)
        stack = self.encoder_taps(x, layers=idx, tokens=tokens, norm=norm, attn_path=attn_path, workspace=workspace)["tokens"]
        asc = sorted(set(idx))
        return stack if idx == asc else stack[:, [asc.index(i) for i in idx]]

    def forward_encoder(self, x: torch.Tensor) -> torch.Tensor:
        """maskformer.py:99-113: the patch tokens of all twelve layers, (B, depth, 384, hw)."""
        return self.encoder_layers(x, tokens="patch").permute(0, 1, 3, 2)

    @torch.no_grad()
    def forward(self, x: torch.Tensor, encoder_only: bool = False, skip_decoder: bool = False,
                return_logits: bool = False, workspace: Optional[torch.Tensor] = None,
                return_attention=False, return_layers=None) -> Dict[str, torch.Tensor]:
        """x: (B,3,H,W) normalised image on a HIP device.  Output dict as maskformer.py:240-251:
        5-D path -> {"objectness" (B,L,nq,1), "mask_pred" (B,L,nq,s gh,s gw) in [0,1] (s = scale_factor), "features" (B,384)};
        3-D path (return_intermediate=False, use_binary_classifier=False) -> {"mask_pred" logits (B,nq,s gh,s gw),
        "features"}.  ``return_logits`` additionally returns the pre-sigmoid einsum as "mask_logits" and the decoder
        queries / encoder patch tokens (parity taps).  ``return_attention``: True adds "last_selfattention" (B,6,N,N), the last
        encoder block's post-softmax attention (vision_transformer.py:307-314), "cls" adds "cls_attention" (B,6,gh,gw), its CLS
        row without the CLS column on the token grid; every other entry keeps the bits it has without it.  ``return_layers``: 0-based
        encoder block indices (as ``encoder_layers``): adds "encoder_layers" (B, len, N, 384), their final-normed outputs in the order
        asked, as a tap - every other entry keeps its bits."""
        if return_layers is not None:
            if encoder_only:
                raise ValueError("return_layers with encoder_only: call encoder_layers(x, layers) for the tokens alone")
            return_layers = self._check_layers(return_layers, "return_layers")
            self._check_tap_args()
        if return_attention not in (False, True, "cls"):
            raise ValueError(f"return_attention={return_attention!r}: False, True or 'cls'")
        if return_attention and encoder_only:
            raise ValueError("return_attention with encoder_only: call get_last_selfattention(x) for the attention alone")
        if return_attention and self.gemm_mode == "f16":
            raise RuntimeError("attention maps are not available in the 'f16' throughput-mode diagnostic")
        if not x.is_cuda:
            raise RuntimeError("MaskFormer (MI355X) needs its input on a HIP device; there is no CPU fallback")
        if self.training:
            raise RuntimeError("inference-only implementation: call model.eval()")
        if self.lateral_connection:
            # the reference hands the 5-D (b, depth, n_dims, hw) stack to forward_pixel_decoder, whose own
            # `assert len(patch_tokens.shape) == 4` (maskformer.py:160) then fails for every input: same outcome here
            raise AssertionError("lateral_connection=True: forward_pixel_decoder expects 4-D patch tokens "
                                 "(the reference asserts at maskformer.py:160)")
        if not self.return_intermediate and self.use_binary_classifier:
            # the reference permutes a 3-D tensor with 4 indices at maskformer.py:229 and raises
            raise RuntimeError("use_binary_classifier=True requires loss_every_decoder_layer/return_intermediate=True")
        lib = N.load()
        x = x.contiguous().float()
        B, c, H, W = x.shape
        assert c == 3, "expected an RGB image batch (B,3,H,W)"
        p = self.encoder.patch_size
        gh, gw = ceil(H / p), ceil(W / p)
        L, nq, dev = self.n_decoder_layers, self.n_queries, x.device
        w = self._weights()
        ws = workspace if workspace is not None else self._get_workspace(w, x)
        io = N.ForwardIO()
        io.x, io.B, io.H, io.W = x.data_ptr(), B, H, W
        io.attn_path = self._ATTN_PATHS[self.attention_path]
        if encoder_only:
            # the reference's encoder_only branch raises on a non-contiguous view (maskformer.py:188); return the
            # evident intent: (B, gh, gw, 384) patch tokens
            tokens = torch.empty((B, gh * gw, N.EMBED), device=dev, dtype=torch.float32)
            io.patch_tokens, io.encoder_only = tokens.data_ptr(), 1
            N.check(lib.sm_maskformer_forward(w, io, ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream),
                    "sm_maskformer_forward")
            return {"patch_tokens": tokens.view(B, gh, gw, N.EMBED)}
        Lm = L if self.return_intermediate else 1  # the 3-D path only builds the last layer's masks (maskformer.py:219-220)
        io.last_layer_only = 0 if self.return_intermediate else 1
        sf = self.scale_factor
        mask_pred = torch.empty((B, Lm, nq, sf * gh, sf * gw), device=dev, dtype=torch.float32)
        objectness = torch.empty((B, L, nq, 1), device=dev, dtype=torch.float32)
        features = torch.empty((B, N.EMBED), device=dev, dtype=torch.float32)
        io.mask_pred, io.objectness, io.features = mask_pred.data_ptr(), objectness.data_ptr(), features.data_ptr()
        extras = {}
        if return_logits or not self.return_intermediate:
            logits = torch.empty_like(mask_pred)
            io.mask_logits = logits.data_ptr()
            extras["mask_logits"] = logits
        if return_logits:
            extras["queries"] = torch.empty((B, L, nq, N.EMBED), device=dev, dtype=torch.float32)
            extras["patch_tokens"] = torch.empty((B, gh * gw, N.EMBED), device=dev, dtype=torch.float32)
            io.queries, io.patch_tokens = extras["queries"].data_ptr(), extras["patch_tokens"].data_ptr()
        attn = {}
        if return_attention == "cls":
            cls_row = torch.empty((B, N.HEADS, gh * gw + 1), device=dev, dtype=torch.float32)
            io.last_attn_cls = cls_row.data_ptr()
            attn["cls_attention"] = cls_row[:, :, 1:].reshape(B, N.HEADS, gh, gw)
        elif return_attention:
            attn["last_selfattention"] = torch.empty((B, N.HEADS, gh * gw + 1, gh * gw + 1), device=dev, dtype=torch.float32)
            io.last_attn = attn["last_selfattention"].data_ptr()
        stream = torch.cuda.current_stream().cuda_stream
        if return_layers is not None:
            taps, tapped = self._new_taps(B, gh * gw + 1, dev, return_layers, stop=False)
            N.check(lib.sm_maskformer_forward_taps(w, io, taps, ws.data_ptr(), ws.numel(), stream), "sm_maskformer_forward_taps")
            asc = sorted(set(return_layers))
            stack = tapped["tokens"]
            attn["encoder_layers"] = stack if return_layers == asc else stack[:, [asc.index(i) for i in return_layers]]
        else:
            N.check(lib.sm_maskformer_forward(w, io, ws.data_ptr(), ws.numel(), stream), "sm_maskformer_forward")
        if not self.return_intermediate:  # 3-D path: last layer, un-sigmoided (maskformer.py:219-220)
            out = {"mask_pred": extras["mask_logits"][:, -1], "features": features}
        elif not self.use_binary_classifier:  # 5-D path with the ffn mask head: no objectness (maskformer.py:225,246-249)
            out = {"mask_pred": mask_pred, "features": features}
        else:
            out = {"objectness": objectness, "mask_pred": mask_pred, "features": features}
        if return_logits:
            out.update(extras)
        out.update(attn)
        return out


def load_checkpoint(model: MaskFormer, path: str, map_location="cpu", strict: bool = True):
    """Accept both checkpoint forms of the reference: a raw state_dict (evaluator.pyc@L357-359) or
    ``{'model': state_dict, ...}`` (app.py:185-186, test_model.py:112-113)."""
    ckpt = torch.load(path, map_location=map_location, weights_only=True)
    sd = ckpt.get("model", ckpt) if isinstance(ckpt, dict) and "model" in ckpt else ckpt
    return model.load_state_dict(sd, strict=strict)
