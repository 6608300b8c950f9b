"""CPU checks of the ResNet-50 backbone: the restatement (tests/_resnet_ref.py) against the fixtures of the real reference, the
state_dict contract of ``selfmask_amd.ResNet50``, ``load_pretrained``, the host-side weight preparation (BatchNorm fold, weight
re-order) and the host-side validation of the ABI additions (their layout and exports: tests/test_abi_cpu.py)."""
import json
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _resnet_cases as RC
import _resnet_ref as RR
from selfmask_amd import ResNet50, get_model, resnet_features
from selfmask_amd import _native as N
from selfmask_amd import resnet as R


@pytest.mark.parametrize("name", list(RC.CASES))
def test_restatement_reproduces_reference_fixture(name, golden_dir):
    """our layer table (every stride, dilation and pad) against the real reference's fp64 maps"""
    dilated, shape, wseed, xseed = RC.CASES[name]
    fx = np.load(os.path.join(golden_dir, f"resnet50_{name}.npz"))
    maps = RR.forward(RC.synthetic_resnet_state_dict(wseed, dilated), RC.synthetic_input(xseed, shape), dilated)
    assert [list(m.shape) for m in maps] == fx["shapes"].tolist()
    for i, m in enumerate(maps):
        ref = fx[f"map{i + 1}_f64"]
        got = (m if i == 3 else m[:, ::RC.STORE_EVERY]).numpy()
        d = np.abs(got - ref).max()
        print(f"{name} map{i + 1}: max |restatement - reference| = {d:.2e}")
        assert d <= 1e-10
    assert (fx["e32"] <= 1e-5).all()


def test_expected_map_shapes():
    for (h, w), dil, exp in (((17, 23), True, [(5, 6), (3, 3), (3, 3), (3, 3)]), ((40, 56), True, [(10, 14), (5, 7), (5, 7), (5, 7)]),
                             ((64, 64), True, [(16, 16), (8, 8), (8, 8), (8, 8)]), ((64, 64), False, [(16, 16), (8, 8), (4, 4), (2, 2)])):
        shapes = ResNet50(use_dilated_resnet=dil).output_shapes(2, h, w)
        assert [s[2:] for s in shapes] == exp and [s[1] for s in shapes] == [256, 512, 1024, 2048]


def test_state_dict_contract(golden_dir):
    keys = json.load(open(os.path.join(golden_dir, "resnet50_keys.json")))
    m = ResNet50()
    sd = m.state_dict()
    assert len(keys) == 318
    assert [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in sd.items()] == keys
    assert [["network." + n, list(s), d] for n, s, d in RC.state_entries()] == keys
    syn = RC.synthetic_resnet_state_dict(11)
    gen = m.weights_generation
    m.load_state_dict(syn, strict=True)
    assert m.weights_generation > gen  # the packed weights are dropped on load
    back = m.state_dict()
    assert all(torch.equal(back[k], syn[k]) for k in syn)
    assert m.n_embs == 2048 and m.use_dilated_resnet and not ResNet50(use_dilated_resnet=False).use_dilated_resnet


def _fake_checkpoint(extra):
    """318 backbone entries under foreign names, values marked by position, with head entries mixed in"""
    out = OrderedDict()
    for i, (name, shape, dt) in enumerate(RC.state_entries()):
        out[f"module.encoder_q.{name}"] = torch.full(shape, float(i % 97) + 0.5).to(getattr(torch, dt))
        if i == 100:
            for k in extra[:1]:
                out[k] = torch.zeros(3)
    for k in extra[1:]:
        out[k] = torch.zeros(3)
    return out


@pytest.mark.parametrize("method,extra", [("mocov2", ["module.encoder_q.fc.0.weight", "module.encoder_q.fc.0.bias", "module.encoder_q.fc.2.weight"]),
                                          ("swav", ["module.projection_head.0.weight", "module.prototypes.weight"])])
def test_load_pretrained(method, extra):
    m = ResNet50(method)
    ck = _fake_checkpoint(extra)
    assert len(R.filter_pretrained(ck, method)) == 318
    m.load_pretrained(ck, method)
    for i, (k, v) in enumerate(m.state_dict().items()):
        assert torch.all(v == torch.tensor(float(i % 97) + 0.5).to(v.dtype)), k
    other = "swav" if method == "mocov2" else "mocov2"
    with pytest.raises(AssertionError, match="layers are different"):  # the other filter leaves the head entries in
        m.load_pretrained(ck, other)
    ck.popitem()
    ck.popitem(last=False)
    with pytest.raises(AssertionError, match="layers are different"):
        m.load_pretrained(ck, method)
    with pytest.raises(ValueError):
        m.load_pretrained(ck, "supervised")


def test_batchnorm_fold_fp64():
    """conv + bias with the folded weight equals conv -> batch_norm (eval) of the restatement, in fp64"""
    sd = {k[len("network."):]: v.double() for k, v in RC.synthetic_resnet_state_dict(11).items()}
    p = "layer3.1"
    x = torch.from_numpy(np.random.RandomState(5).standard_normal((2, 256, 5, 7)))
    w = sd[p + ".conv2.weight"]
    ref = RR._bn(F.conv2d(x, w, None, 1, 2, 2), sd, p + ".bn2")
    wf, bf = R.fold_batchnorm(w, sd[p + ".bn2.weight"], sd[p + ".bn2.bias"], sd[p + ".bn2.running_mean"], sd[p + ".bn2.running_var"])
    assert wf.dtype == torch.float64 and bf.dtype == torch.float64
    d = (F.conv2d(x, wf, bf, 1, 2, 2) - ref).abs().max().item()
    print(f"fold: max |folded - conv + bn| = {d:.2e}")
    assert d <= 1e-12


@pytest.mark.parametrize("k,stride,dil", [(1, 2, 1), (3, 1, 1), (3, 2, 1), (3, 1, 2), (3, 1, 4)])
def test_weight_reorder_matches_gather(k, stride, dil):
    """numpy tap gather x re-ordered weight = F.conv2d (fp64): the (Cout, kh, kw, Cin) order is the gather's"""
    rng = np.random.RandomState(k * 100 + stride * 10 + dil)
    pad = dil if k == 3 else 0
    x = rng.standard_normal((2, 16, 5, 7))
    w = rng.standard_normal((24, 16, k, k))
    ref = F.conv2d(torch.from_numpy(x), torch.from_numpy(w), None, stride, pad, dil).permute(0, 2, 3, 1).numpy()
    g = RR.gather_taps(np.ascontiguousarray(x.transpose(0, 2, 3, 1)), k, stride, dil, pad)
    got = g @ R.gemm_weight(torch.from_numpy(w)).numpy().T
    assert got.shape == ref.shape and np.abs(got - ref).max() <= 1e-12


def test_stem_weight_matches_stem_gather():
    rng = np.random.RandomState(3)
    x, w = rng.standard_normal((2, 3, 17, 23)), rng.standard_normal((8, 3, 7, 7))
    ref = F.conv2d(torch.from_numpy(x), torch.from_numpy(w), None, 2, 3).permute(0, 2, 3, 1).numpy()
    gw = R.gemm_weight(torch.from_numpy(w))
    assert gw.shape == (8, 160) and (gw[:, 147:] == 0).all()
    g = RR.gather_stem(x)
    assert (g[..., 147:] == 0).all()
    assert np.abs(g @ gw.numpy().T - ref).max() <= 1e-12


def test_maxpool_witness_matches_torch():
    x = -np.abs(np.random.RandomState(4).standard_normal((2, 9, 12, 8))) - 0.1  # all negative: the padding must not win
    ref = F.max_pool2d(torch.from_numpy(x).permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).numpy()
    assert np.array_equal(RR.maxpool3x3s2(x), ref) and ref.max() < 0


def test_no_cpu_fallback():
    m = ResNet50()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(1, 3, 32, 32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        resnet_features(m, torch.zeros(1, 3, 32, 32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        R.upsample_nhwc_aligned(torch.zeros(1, 3, 3, 8))


def test_argument_validation_without_gpu():
    lib = N.load()
    assert N.RESNET50_BLOCKS == sum(b for _, _, b in R.STAGES)  # the ABI's block table is as long as the host's layer table
    assert lib.sm_resnet50_workspace_bytes(0, 64, 64, 1) == 0
    b1, b4 = lib.sm_resnet50_workspace_bytes(1, 224, 224, 1), lib.sm_resnet50_workspace_bytes(4, 224, 224, 1)
    assert b1 >= 28 * 28 * 4608 * 4 and b1 < b4 < 2 ** 31
    assert lib.sm_resnet50_workspace_bytes(1, 224, 224, 0) < b1  # strided layers 3 / 4: smaller gathered operands
    assert lib.sm_resnet50_workspace_bytes(512, 224, 224, 1) == 0  # the gathered operand would pass the GEMM's 4 GiB limit
    assert lib.sm_conv_gather_f16x2(None, None, 1, 3, 3, 64, 3, 1, 1, 1, None) == -1
    assert lib.sm_resnet50_forward(None, None, 1, 64, 64, 1, None, None, None, None, None, 0, None) == -1
    assert b"null pointer" in lib.sm_last_error()


def test_get_model_resnet50_still_raises():
    with pytest.raises(ValueError):
        get_model("resnet50", training_method="swav")
    from selfmask_amd.mask_generator import MaskGenerator
    with pytest.raises(NotImplementedError):
        MaskGenerator(feature_types=["mocov2", "dino"], network=None)
