"""CPU-only checks of the drop-in boundary: the C-ABI library loads and exports every symbol include/*.h declares, the
whole ctypes mirror - every struct, field, prototype and constant of selfmask_amd/_native.py - is what a compiler sees in
the header (tests/_abi_probe.py), and the host mirror keeps the reference's state_dict contract."""
import ctypes
import os
import re

import pytest
import torch

import _abi_probe as P
from selfmask_amd import _native as N
from selfmask_amd import MaskFormer, get_model, BaseStructure, state_shapes, synthetic_state_dict

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    hdr = open(os.path.join(REPO, "include", "selfmask_hip.h")).read()
    declared = set(re.findall(r"\b(sm_[a-z0-9_]+)\s*\(", hdr))
    assert declared, "no prototypes found in the header"
    lib = N.load()
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in selfmask_hip.h but not exported by the .so"
    assert declared == set(N.SYMBOLS), (declared ^ set(N.SYMBOLS))
    assert lib.sm_version() >= 100


def test_every_header_struct_has_one_mirror():
    assert set(P.header_structs()) == set(N.STRUCTS), set(P.header_structs()) ^ set(N.STRUCTS)
    defined = {c for c in vars(N).values() if isinstance(c, type) and issubclass(c, ctypes.Structure) and c.__module__ == N.__name__}
    assert defined == set(N.STRUCTS.values()), defined ^ set(N.STRUCTS.values())


def test_mirror_equals_what_the_compiler_sees():
    """struct: sizeof and alignof; field: offset, kind and element count; proto: the kinds of the return value and of every parameter
    (ctypes converts a Python number to whatever argtypes says, so a c_int32 where the header has int64_t never raises)"""
    for what in ("struct", "field", "proto"):
        c, py = P.header()[what], P.mirror()[what]
        assert c.keys() == py.keys(), what
        wrong = {k: {"header": c[k], "mirror": py[k]} for k in c if c[k] != py[k]}
        assert not wrong, (what, wrong)


def test_field_names_in_header_order():
    """a trailing field that tail padding hides, or two same-typed neighbours swapped, move no offset the layout test looks at"""
    hdr = P.header_structs()
    for cname, ct in N.STRUCTS.items():
        assert hdr[cname] == [f for f, _ in ct._fields_], cname


# macros the binding has no use for; every other SM_X of the header is the module's X
UNMIRRORED = {"SM_OK", "SM_EINVAL", "SM_ELAUNCH", "SM_ENOSPACE", "SM_JPEG_MAX_SCAN_BYTES", "SM_JPEG_SUBSEQ_BITS_MAX", "SM_PNG_MAX_DATA_BYTES"}


def test_every_header_macro_is_mirrored_or_listed():
    c, py = P.header()["macro"], P.mirror()["macro"]
    assert set(c) - set(py) == UNMIRRORED, (set(c) - set(py)) ^ UNMIRRORED
    wrong = {m: {"header": c[m], "mirror": py[m]} for m in py if c[m] != py[m]}
    assert not wrong, wrong
    assert N.KNN_METHODS == {"auto": N.KNN_AUTO, "gram": N.KNN_GRAM, "stream": N.KNN_STREAM}


def test_pinned_values_on_both_sides():
    """the literal numbers the features' own tests used to pin: a change made on both sides at once still fails here"""
    c = P.header()
    for cname, size in {"sm_present_image": 40, "sm_png_image": 48, "sm_object": 56, "sm_jpeg_segment": 16, "sm_jpeg_scan": 160,
                        "sm_jpeg_image": 64}.items():
        assert c["struct"][cname][0] == ctypes.sizeof(N.STRUCTS[cname]) == size, cname
    for macro, value in {"SM_PNG_STREAM_MAGIC": 0x474e5073, "SM_PNG_MAX_PIXELS": 1 << 24, "SM_OBJ_SUMMARY_INTS": 10,
                         "SM_RESNET50_BLOCKS": 16}.items():
        assert c["macro"][macro] == getattr(N, macro[3:]) == value, macro
    # the attention-map fields were appended at the END: nothing in front of them moved
    last3 = ["last_attn", "last_attn_cls", "attn_only"]
    assert P.header_structs()["sm_forward_io"][-3:] == [f for f, _ in N.ForwardIO._fields_][-3:] == last3
    assert N.PNG_UNSUPPORTED != N.JPEG_UNSUPPORTED  # the two decoders' "hand it to Pillow" verdicts stay apart


def test_argument_validation_without_gpu():
    """Validation happens on the host before any launch, so it is testable without a GPU."""
    lib = N.load()
    g = N.GemmArgs()
    assert lib.sm_gemm_f32(g, None) == -1 and b"null pointer" in lib.sm_last_error()
    assert lib.sm_layernorm_f32(None, 384, None, None, None, 384, 4, 384, 1e-6, None) == -1
    assert lib.sm_layernorm_rows_f32(N.LnArgs(), None) == -1
    w = N.Weights()
    w.patch = 7
    assert lib.sm_forward_workspace_bytes(w, 1, 224, 224) == 0
    w.patch, w.n_dec_layers, w.n_queries, w.pos_grid = 16, 6, 20, 14
    b1, b64 = lib.sm_forward_workspace_bytes(w, 1, 224, 224), lib.sm_forward_workspace_bytes(w, 64, 224, 224)
    assert 0 < b1 < b64 < 2 ** 31


@pytest.mark.parametrize("patch,ubc", [(16, True), (8, True), (16, False)])
def test_state_dict_contract(patch, ubc):
    m = MaskFormer(n_queries=20, patch_size=patch, n_decoder_layers=6, return_intermediate=ubc,
                   use_binary_classifier=ubc)
    exp = state_shapes(20, patch, 6, ubc)
    sd = m.state_dict()
    assert list(sd.keys()) == list(exp.keys())
    assert all(tuple(v.shape) == exp[k] for k, v in sd.items())
    m.load_state_dict(synthetic_state_dict(0, "soft", patch_size=patch, use_binary_classifier=ubc), strict=True)
    # wrapped checkpoints ({'model': sd}) are what app.py:185-186 loads
    assert m.encoder.n_embs == 384 and m.encoder.n_heads == 6 and m.encoder.depth == 12 and m.encoder.patch_size == patch


def test_get_model_reads_reference_config_keys(tmp_path):
    from argparse import Namespace
    cfg = Namespace(n_queries=20, n_decoder_layers=6, learnable_pixel_decoder=False, lateral_connection=False,
                    loss_every_decoder_layer=True, scale_factor=2, abs_2d_pe_init=False, use_binary_classifier=True,
                    arch="vit_small", training_method="dino", patch_size=8)
    m = get_model("maskformer", configs=cfg)
    assert isinstance(m, MaskFormer) and m.use_binary_classifier and m.encoder.patch_size == 8
    with pytest.raises(ValueError):
        get_model("resnet50", training_method="swav")
    # both checkpoint wrappers
    from selfmask_amd import load_checkpoint
    sd = synthetic_state_dict(0, "soft", patch_size=8)
    torch.save(sd, tmp_path / "raw.pt")
    torch.save({"model": sd, "n_epochs": 12}, tmp_path / "wrapped.pt")
    load_checkpoint(m, str(tmp_path / "raw.pt"))
    load_checkpoint(m, str(tmp_path / "wrapped.pt"))


def test_no_cpu_fallback():
    m = MaskFormer(n_queries=20, patch_size=16, n_decoder_layers=6, return_intermediate=True, use_binary_classifier=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(1, 3, 224, 224))
    bs = BaseStructure(m, device=torch.device("cpu"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        bs._forward({"x": torch.zeros(1, 3, 32, 32)}, device=torch.device("cpu"))
