"""Host-side mirror of the reference's ``networks.resnet.ResNet50`` (resnet.py:8-56): the dilated ResNet-50 whose last feature map
the pseudo-mask generator clusters for its ``"mocov2"`` and ``"swav"`` feature types (mask_generator.pyc@L136-200;
utils/misc.py:220-223 builds it as ``ResNet50(training_method)``).

Same 318-entry ``state_dict`` under ``network.`` (``ResNetBackbone("resnet50_dilated8")``: resnet_backbone.py:42-105,
resnet_models.py:57-154), same ``forward(x) -> [four NCHW feature maps]``; the arithmetic runs in libselfmask_hip.so
(csrc/conv.hip: sm_resnet50_forward).  The sub-modules are parameter containers only; there is no CPU fallback.

The maps come back as (B, C, h, w) tensors in channels-last memory (the kernels work on NHWC rows), values and shapes as the
reference's.  BatchNorm (eval, eps 1e-5) is folded into each convolution in fp64 on the host, the folded weights are packed once
into the W16 GEMM format and re-packed when the ``state_dict`` changes.
"""
from collections import OrderedDict
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn

from . import _native as N

BN_EPS = 1e-5
STAGES = (("layer1", 64, 3), ("layer2", 128, 4), ("layer3", 256, 6), ("layer4", 512, 3))  # resnet_models.py:122-125,218
STEM_K = 160  # 7 * 7 * 3 = 147 taps, zero-padded to a multiple of 32
TOTAL_STRIDE = 8  # mask_generator.pyc@L150-157: the ResNet branches pad to a multiple of 8


class _Bottleneck(nn.Module):  # resnet_models.py:57-71
    def __init__(self, inplanes: int, planes: int, downsample: bool):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, kernel_size=1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, kernel_size=1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        if downsample:
            self.downsample = nn.Sequential(nn.Conv2d(inplanes, planes * 4, kernel_size=1, bias=False), nn.BatchNorm2d(planes * 4))


class _Backbone(nn.Module):
    """Parameter container with ResNetBackbone's names (prefix.conv1, prefix.bn1, layer1.0.conv1, ...).  The strides and dilations
    live in the native launch plan (conv.hip), chosen by ``dilated``; they are no part of the state_dict."""

    def __init__(self):
        super().__init__()
        self.prefix = nn.Sequential(OrderedDict([("conv1", nn.Conv2d(3, 64, kernel_size=7, stride=2, padding=3, bias=False)),
                                                 ("bn1", nn.BatchNorm2d(64))]))
        inplanes = 64
        for name, planes, blocks in STAGES:
            layer = nn.Sequential(*[_Bottleneck(inplanes if i == 0 else planes * 4, planes, i == 0) for i in range(blocks)])
            setattr(self, name, layer)
            inplanes = planes * 4
        self.num_features = 2048


def fold_batchnorm(weight: torch.Tensor, gamma, beta, mean, var, eps: float = BN_EPS) -> Tuple[torch.Tensor, torch.Tensor]:
    """conv + BatchNorm(eval) as one convolution with a bias, in fp64: (w * g, beta - mean * g) with g = gamma / sqrt(var + eps)
    per output channel."""
    g = gamma.double() / torch.sqrt(var.double() + eps)
    return weight.double() * g.view(-1, *([1] * (weight.dim() - 1))), beta.double() - mean.double() * g


def gemm_weight(w: torch.Tensor) -> torch.Tensor:
    """(Cout, Cin, kh, kw) -> the (Cout, K) matrix whose columns match the device gathers: (kh, kw, Cin) for 1 x 1 / 3 x 3
    (sm_conv_gather_f16x2 lays whole input rows tap after tap), (Cin, kh, kw) as it lies, zero-padded to 160, for the 7 x 7 stem
    (sm_resnet_stem_gather_f16x2)."""
    co, ci, kh, kw = w.shape
    if kh == 7:
        out = w.new_zeros((co, STEM_K))
        out[:, :ci * kh * kw] = w.reshape(co, -1)
        return out
    return w.permute(0, 2, 3, 1).reshape(co, kh * kw * ci).contiguous()


def filter_pretrained(state_dict: Dict[str, torch.Tensor], training_method: str) -> Dict[str, torch.Tensor]:
    """The key filters of ResNet50._load_pretrained (resnet.py:22-33) on a dict the caller has loaded: MoCo-v2 checkpoints lose the
    ``fc.0`` / ``fc.2`` head, SwAV ones the ``projection_head`` and ``prototypes``."""
    drop = {"mocov2": ("fc.0", "fc.2"), "swav": ("projection_head", "prototypes")}.get(training_method)
    if drop is None:
        raise ValueError(f"training_method={training_method!r}: 'mocov2' or 'swav'")
    return OrderedDict((k, v) for k, v in state_dict.items() if not any(w in k for w in drop))


class ResNet50(nn.Module):
    def __init__(self, weight_type: Optional[str] = None, use_dilated_resnet: bool = True):
        """``weight_type`` is kept for the reference's signature; no weights are fetched or read from a path here (the reference's
        three modes download through torchvision or read hard-coded home directories): load a checkpoint with ``load_state_dict``
        or, for a raw MoCo-v2 / SwAV checkpoint, ``load_pretrained(state_dict, weight_type)``."""
        super().__init__()
        self.network = _Backbone()
        self.n_embs = self.network.num_features
        self.use_dilated_resnet = bool(use_dilated_resnet)
        self.weight_type = weight_type
        self._table = None       # (Resnet50Weights struct, key) cache
        self._packed = None      # folded + packed weights (kept alive here, rebuilt when the weights change)
        self.weights_generation = 0
        self._workspace = {}     # (device, stream) -> uint8 tensor, grown to the largest forward that stream has run
        self.register_load_state_dict_post_hook(lambda module, incompatible_keys: module.refresh_packed())
        self.eval()

    # ---- weights ----------------------------------------------------------------------------------------------------
    def _apply(self, fn, *a, **kw):  # .to() / .cuda() move storage: drop cached pointers
        self._table = None
        self._packed = None
        self._workspace = {}
        self.weights_generation = getattr(self, "weights_generation", 0) + 1
        return super()._apply(fn, *a, **kw)

    def refresh_packed(self):
        """Drop the packed weights; call after editing parameters or buffers in place (``load_state_dict``, ``load_pretrained`` and
        ``.to()`` do it themselves)."""
        self._table = None
        self._packed = None
        self.weights_generation += 1

    @torch.no_grad()
    def load_pretrained(self, state_dict: Dict[str, torch.Tensor], training_method: str) -> None:
        """ResNet50._load_pretrained (resnet.py:20-53) for a checkpoint dict the caller has loaded (for MoCo-v2 its
        ``["state_dict"]``): filter the keys, assert equal length, copy BY POSITION."""
        state_dict = filter_pretrained(state_dict, training_method)
        curr = self.network.state_dict()
        assert len(curr) == len(state_dict), f"# layers are different: {len(curr)} != {len(state_dict)}"
        for k_curr, k in zip(curr.keys(), state_dict.keys()):
            curr[k_curr].copy_(state_dict[k])
        self.refresh_packed()

    def _convs(self):
        """(struct path, conv, bn) of the 53 convolutions, in launch order"""
        net = self.network
        yield ("stem", None), net.prefix.conv1, net.prefix.bn1
        n = 0
        for name, _planes, _blocks in STAGES:
            for blk in getattr(net, name):
                yield ("conv1", n), blk.conv1, blk.bn1
                yield ("conv2", n), blk.conv2, blk.bn2
                yield ("conv3", n), blk.conv3, blk.bn3
                if hasattr(blk, "downsample"):
                    yield ("down", n), blk.downsample[0], blk.downsample[1]
                n += 1

    def _weights(self) -> N.Resnet50Weights:
        first = self.network.prefix.conv1.weight
        key = (first.data_ptr(), self.network.layer4[2].bn3.running_var.data_ptr())
        if self._table is not None and self._table[1] == key:
            return self._table[0]
        for n_, t in list(self.named_parameters()) + list(self.named_buffers()):
            if not t.is_cuda or (t.dtype != torch.float32 and not n_.endswith("num_batches_tracked")):
                raise RuntimeError(f"{n_} must be a float32 tensor on a HIP device (got {t.device}, {t.dtype}); the product path "
                                   f"has no CPU fallback")
        from . import ops
        w = N.Resnet50Weights()
        packed = []
        for (field, n), conv, bn in self._convs():
            # the fold is host arithmetic: the tensors come to the CPU, fp64 there, and go back rounded to fp32
            wf, bf = fold_batchnorm(*(t.detach().cpu() for t in (conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var)), bn.eps)
            w16, scale = ops.split_w16(gemm_weight(wf).float().contiguous().to(first.device))
            bias = bf.float().contiguous().to(first.device)
            packed += [w16, bias]
            cw = w.stem if field == "stem" else getattr(w.block[n], field)
            cw.w, cw.bias, cw.w_scale = w16.data_ptr(), bias.data_ptr(), scale
        # the split kernels ran on the current stream; forwards on other streams reuse the table without an event dependency
        torch.cuda.current_stream(first.device).synchronize()
        self._packed = packed
        self._table = (w, key)
        return w

    def _get_workspace(self, x: torch.Tensor) -> torch.Tensor:
        B, _, H, W = x.shape
        nbytes = N.load().sm_resnet50_workspace_bytes(B, H, W, 1 if self.use_dilated_resnet else 0)
        if nbytes == 0:
            raise RuntimeError(f"sm_resnet50_workspace_bytes returned 0 for a {tuple(x.shape)} input (bad shape, or too large a batch)")
        k = (x.device, torch.cuda.current_stream().cuda_stream)
        ws = self._workspace.get(k)
        if ws is None or ws.numel() < nbytes:
            ws = self._workspace[k] = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        return ws

    def output_shapes(self, B: int, H: int, W: int) -> List[Tuple[int, int, int, int]]:
        """(B, C, h, w) of the four maps for a (B, 3, H, W) input"""
        def o(n, k, s, d, p):
            return (n + 2 * p - d * (k - 1) - 1) // s + 1
        h, w = (o(o(n, 7, 2, 1, 3), 3, 2, 1, 1) for n in (H, W))
        out = [(B, 256, h, w)]
        for c, strided in ((512, True), (1024, not self.use_dilated_resnet), (2048, not self.use_dilated_resnet)):
            if strided:
                h, w = o(h, 3, 2, 1, 1), o(w, 3, 2, 1, 1)
            out.append((B, c, h, w))
        return out

    # ---- forward ----------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def forward(self, x: torch.Tensor, workspace: Optional[torch.Tensor] = None) -> List[torch.Tensor]:
        """x: (B, 3, H, W) normalised image batch on a HIP device -> the reference's list of four feature maps (resnet.py:55-56):
        (B, 256 | 512 | 1024 | 2048, h, w), strides 4, 8, 8, 8 (dilated) or 4, 8, 16, 32."""
        if not x.is_cuda:
            raise RuntimeError("ResNet50 (MI355X) needs its input on a HIP device; there is no CPU fallback")
        if self.training:
            raise RuntimeError("inference-only implementation: call model.eval()")
        lib = N.load()
        x = x.contiguous().float()
        B, c, H, W = x.shape
        assert c == 3, "expected an RGB image batch (B,3,H,W)"
        w = self._weights()
        ws = workspace if workspace is not None else self._get_workspace(x)
        maps = [torch.empty((b_, h_, w_, c_), device=x.device, dtype=torch.float32) for b_, c_, h_, w_ in self.output_shapes(B, H, W)]
        N.check(lib.sm_resnet50_forward(w, x.data_ptr(), B, H, W, 1 if self.use_dilated_resnet else 0, *(m.data_ptr() for m in maps),
                                        ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream), "sm_resnet50_forward")
        return [m.permute(0, 3, 1, 2) for m in maps]


def upsample_nhwc_aligned(f: torch.Tensor, scale: int = 2, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """F.interpolate(scale_factor=scale, mode="bilinear", align_corners=True) of a channels-last map: (B, h, w, C) -> (B, scale h,
    scale w, C) on the device (sm_upsample_nhwc_aligned_f32).  ``out``: a contiguous float32 tensor of that many elements to write into
    (a caller's scratch)."""
    if not f.is_cuda or f.dtype != torch.float32:
        raise RuntimeError("upsample_nhwc_aligned needs a float32 tensor on a HIP device (no CPU fallback)")
    f = f.contiguous()
    B, h, w, C = f.shape
    shape = (B, scale * h, scale * w, C)
    if out is None:
        up = torch.empty(shape, device=f.device, dtype=torch.float32)
    else:
        assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == B * scale * h * scale * w * C
        up = out.view(shape)
    N.check(N.load().sm_upsample_nhwc_aligned_f32(f.data_ptr(), up.data_ptr(), B, h, w, C, scale, torch.cuda.current_stream().cuda_stream),
            "sm_upsample_nhwc_aligned_f32")
    return up


@torch.no_grad()
def resnet_features(model: ResNet50, x: torch.Tensor, out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, Tuple[int, int]]:
    """What mask_generator.pyc@L150-159 hands the clusterer for a ResNet feature type: x zero-padded right / bottom to a multiple of
    the total stride 8 (pad_input_image @L124-134), ``model(x)[-1]``, bilinear x 2 (align_corners=True), one row per position:
    ((B, 2h * 2w, n_embs), (h, w)) with (h, w) the last map's grid.  ``out``: scratch for the rows (``upsample_nhwc_aligned``)."""
    if not x.is_cuda:
        raise RuntimeError("resnet_features needs its input on a HIP device; there is no CPU fallback")
    H, W = x.shape[-2:]
    s = TOTAL_STRIDE
    x = nn.functional.pad(x, (0, (s - W % s) % s, 0, (s - H % s) % s), value=0)
    f = model(x)[-1].permute(0, 2, 3, 1)  # the (B, h, w, C) rows the forward wrote
    B, h, w, C = f.shape
    return upsample_nhwc_aligned(f, 2, out).view(B, 4 * h * w, C), (h, w)
