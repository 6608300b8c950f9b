"""The three-backbone pseudo-mask generator (selfmask_amd/mask_generator.py: ``backbones={"mocov2" | "swav": ResNet50}``): the
constructor's contract and the planner on the CPU; on the device 9 candidates per feature type in ``feature_types`` order, the ResNet
ones against the oracle chain fed with the device's own ``resnet_features``, all 27 in one vote."""
import types

import numpy as np
import pytest
import torch

from selfmask_amd import _native as N
from selfmask_amd.mask_generator import MaskGenerator

gpu = pytest.mark.gpu
DEV = "cuda:0"
TYPES3 = ["mocov2", "swav", "dino"]


def fake_network(patch=16):
    """what the planner reads of a MaskFormer: the patch size, and the weight table the encoder's workspace size is asked with"""
    w = N.Weights()
    w.patch, w.n_dec_layers, w.n_queries, w.pos_grid = patch, 6, 20, 14
    return types.SimpleNamespace(encoder=types.SimpleNamespace(patch_size=patch), _weights=lambda: w)


# ---- CPU ------------------------------------------------------------------------------------------------------------------------
def test_constructor_contract_with_backbones():
    r = object()
    with pytest.raises(NotImplementedError, match="swav"):  # a ResNet type without its backbone: named, before `network` is looked at
        MaskGenerator(feature_types=TYPES3, backbones={"mocov2": r})
    with pytest.raises(NotImplementedError, match="mocov2"):
        MaskGenerator(feature_types=TYPES3, network=object())
    with pytest.raises(NotImplementedError, match="byol"):  # not a type the reference knows
        MaskGenerator(feature_types=["byol", "dino"], network=object(), backbones={"byol": r})
    with pytest.raises(ValueError, match="network"):
        MaskGenerator(feature_types=TYPES3, backbones={"mocov2": r, "swav": r})
    g = MaskGenerator(feature_types=TYPES3, network=object(), backbones={"mocov2": r, "swav": r, "unused": r}, device="cpu")
    assert g.feature_types == TYPES3 and g.resnet_types == ["mocov2", "swav"] and sorted(g.backbones) == ["mocov2", "swav"]
    g = MaskGenerator(feature_types=["swav"], backbones={"swav": r}, device="cpu")  # no "dino": no `network` needed
    assert g.resnet_types == ["swav"] and g._bucket_stride() == 8
    assert MaskGenerator(network=object(), device="cpu").resnet_types == []


def test_vote_takes_at_most_64_planes():
    r = object()
    MaskGenerator(cluster_sizes=(2, 3, 4, 5, 6), feature_types=TYPES3, network=object(), backbones={"mocov2": r, "swav": r})  # 60 planes
    with pytest.raises(ValueError, match="66"):
        MaskGenerator(cluster_sizes=(2, 4, 5, 5, 6), feature_types=TYPES3, network=object(), backbones={"mocov2": r, "swav": r})
    with pytest.raises(ValueError, match="65"):
        MaskGenerator(cluster_sizes=(5,) * 13, network=object())


@pytest.mark.parametrize("cluster_type", ["k-means", "kmeans"])
def test_kmeans_with_a_resnet_type_is_refused(cluster_type):
    with pytest.raises(NotImplementedError, match="k-means"):
        MaskGenerator(cluster_type=cluster_type, feature_types=["mocov2", "dino"], network=object(), backbones={"mocov2": object()})
    from selfmask_amd import voting as VT
    with pytest.raises(NotImplementedError, match="k-means"):
        VT.extract_candidate_masks_resnet(object(), torch.zeros(1, 3, 64, 64), cluster_type=cluster_type)


def test_bucket_plan_follows_the_stride_8_grid(tmp_path):
    """100 x 130 and 110 x 130 pad to one 16-grid (112 x 144) but to different 8-grids (104 / 112 x 136): one batch for "dino" alone,
    two once a ResNet type is asked for - the size of its own padded grid enters that type's align_corners up-sample"""
    from PIL import Image
    paths = []
    for i, (h, w) in enumerate([(100, 130), (110, 130), (104, 136), (97, 129)]):
        p = str(tmp_path / f"p{i}.png")
        Image.new("RGB", (w, h)).save(p)
        paths.append(p)
    dino = MaskGenerator(network=fake_network(), device="cpu")
    assert sorted(sorted(b) for b in dino._plan(paths)[2]) == [[0, 1, 2, 3]]
    both = MaskGenerator(feature_types=["mocov2", "dino"], network=fake_network(), backbones={"mocov2": object()}, device="cpu")
    assert sorted(sorted(b) for b in both._plan(paths)[2]) == [[0, 2, 3], [1]]
    assert both._points((100, 130)) == 4 * 7 * 9 and both._points_resnet((100, 130)) == 4 * 13 * 17
    # every size counts against the budget once a ResNet type is there; "dino" alone keeps batch_size below 8192 points
    tight = MaskGenerator(feature_types=["mocov2", "dino"], network=fake_network(), backbones={"mocov2": object()}, device="cpu",
                          batch_size=128, max_stream_bytes=1)
    assert tight._batch_cap((300, 400)) == 1
    lib = N.load()
    per = (lib.sm_resnet50_workspace_bytes(1, 304, 400, 1) + 7600 * 2048 * 4 + lib.sm_spectral_workspace_bytes_dim(1, 7600, 2048, 10, 4)
           + lib.sm_spectral_workspace_bytes(1, 1900, 10, 4) + lib.sm_forward_workspace_bytes(fake_network()._weights(), 1, 304, 400))
    assert per > 7600 * 7600 * 4  # the Gram matrix of the ResNet type's 7600 points is in there
    roomy = MaskGenerator(feature_types=["mocov2", "dino"], network=fake_network(), backbones={"mocov2": object()}, device="cpu",
                          batch_size=128, max_stream_bytes=5 * per + 1)
    assert roomy._batch_cap((300, 400)) == 5
    assert MaskGenerator(network=fake_network(), device="cpu", max_stream_bytes=1)._batch_cap((300, 400)) == 128
    # a file whose ResNet grid is out of the clusterer's range is named before anything runs (the DINO count would pass: 4 * 64 * 128)
    big = str(tmp_path / "big.png")
    Image.new("RGB", (2048, 1024)).save(big)
    assert dino._plan([big])[1] == [(1024, 2048)]
    with pytest.raises(ValueError, match="big.png"):
        both._plan([paths[0], big])


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
SIZES = [(64, 64), (64, 72), (61, 70), (96, 64)]


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """models, files and the three-type candidates, made once"""
    from PIL import Image
    import _resnet_cases as RC
    from selfmask_amd import MaskFormer, ResNet50, synthetic_state_dict
    m = MaskFormer(n_queries=20, patch_size=16, n_decoder_layers=6, return_intermediate=True, use_binary_classifier=True)
    m.load_state_dict(synthetic_state_dict(31, "soft", patch_size=16), strict=True)
    m = m.to(DEV)
    backbones = {}
    for name, seed in (("mocov2", 11), ("swav", 12)):
        r = ResNet50(use_dilated_resnet=True)
        r.load_state_dict(RC.synthetic_resnet_state_dict(seed, True), strict=True)
        backbones[name] = r.to(DEV).eval()
    d = tmp_path_factory.mktemp("backbones")
    # Pixel noise, not a smooth scene: at these sizes every cell of a random-weight ResNet's 8 x 8 map sees the zero padding, and on a
    # smooth image that border signature outweighs the content - the k-NN graph falls into the image's quadrants (fp64 restatement,
    # tests/_resnet_ref.py: 3 components at 64 x 64, 2 at 61 x 70).  Eigenvalue 0 is then multiple, ANY basis of its space is a
    # valid answer and a comparison of labels with the oracle is not defined.  Noise gives one component at all four sizes for both
    # weight seeds; test_resnet_candidates_against_the_oracle_chain asserts that on the oracle's graph before it compares.
    rng = np.random.Generator(np.random.PCG64(1))
    paths = []
    for i, (h, w) in enumerate(SIZES):
        p = str(d / f"im{i}.png")
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(p)
        paths.append(p)
    gen = MaskGenerator(feature_types=TYPES3, network=m, backbones=backbones, device=DEV, batch_size=2)
    cands = gen.extract_candidate_masks(paths)
    torch.cuda.synchronize()
    return types.SimpleNamespace(model=m, backbones=backbones, paths=paths, gen=gen, cands=cands)


@gpu
def test_candidates_per_type_in_order(world):
    two = MaskGenerator(feature_types=["swav", "dino"], network=world.model, backbones=world.backbones, device=DEV).extract_candidate_masks(world.paths)
    dino = MaskGenerator(network=world.model, device=DEV).extract_candidate_masks(world.paths)
    for p, (h, w) in zip(world.paths, SIZES):
        name = p.split("/")[-1]
        c = world.cands[name]
        assert c.shape == (27, h, w) and c.dtype == torch.uint8
        for t in range(3):
            for k0, k in ((0, 2), (2, 3), (5, 4)):  # every group of k planes is a partition of the image
                assert torch.equal(c[9 * t + k0:9 * t + k0 + k].sum(0).cpu(), torch.ones(h, w, dtype=torch.uint8)), (name, t, k)
        assert torch.equal(c[18:], dino[name])  # the DINO nine: what "dino" alone gives
        assert two[name].shape == (18, h, w) and torch.equal(two[name][:9], c[9:18]) and torch.equal(two[name][9:], c[18:])


@gpu
def test_resnet_candidates_against_the_oracle_chain(world):
    from scipy.sparse.csgraph import connected_components
    from oracle import cluster_oracle as CO
    from selfmask_amd import resnet_features
    for p, (h, w) in zip(world.paths, SIZES):
        name = p.split("/")[-1]
        x = world.gen._load(p)[None].to(DEV)
        for t, f in enumerate(("mocov2", "swav")):
            feats, (gh, gw) = resnet_features(world.backbones[f], x)  # the DEVICE's features of the file alone
            assert (gh, gw) == (-(-h // 8), -(-w // 8)) and feats.shape == (1, 4 * gh * gw, 2048)
            ref_labels, ref_idx, _, _ = CO.spectral_cluster(feats[0].cpu().numpy(), (2, 3, 4), 10)
            assert connected_components(CO.affinity_from_knn(ref_idx))[0] == 1  # (the comparison's precondition: see `world`)
            ref = torch.cat([CO.to_one_hot_masks(torch.from_numpy(ref_labels[k]).reshape(2 * gh, 2 * gw), k, 4, h, w) for k in (2, 3, 4)])
            miss = (world.cands[name][9 * t:9 * t + 9].cpu() != ref).float().mean().item()
            print(f"{name} {f}: mismatch {miss:.3e} of the pixels")
            assert miss <= 5e-3, (name, f)


@gpu
def test_vote_over_all_planes_and_files_together_or_alone(world):
    from oracle import voting_oracle as V
    from selfmask_amd.mask_generator import rle_decode
    out = world.gen(world.paths)
    assert sorted(out) == sorted(p.split("/")[-1] for p in world.paths)
    for p, (h, w) in zip(world.paths, SIZES):
        name = p.split("/")[-1]
        c = world.cands[name].contiguous()
        best_mask, best, new_to_prev = world.gen.vote_mask(c)
        ref_mask, ref_best, ref_map, _, _ = V.vote_mask(c.cpu())
        assert best == ref_best and new_to_prev == ref_map and torch.equal(best_mask.cpu(), ref_mask)
        assert np.array_equal(rle_decode(out[name]), ref_mask.numpy())
        assert world.gen([p]) == {name: out[name]}  # alone or with the others: the same code
    raw = world.gen(world.paths[:2], encode=False)
    for name in raw:
        assert np.array_equal(raw[name], rle_decode(out[name]))
