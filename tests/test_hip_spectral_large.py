"""Spectral clustering above 8192 points (csrc/spectral.hip: streaming k-NN on the matrix cores, the O(n m) graph build, the
eigen-solver's one-column and gathering plans): every stage against its restatement on the device's own graph, separable features
as the true partition, the graph build's results pinned at small n, and - through the tuning build - the streaming k-NN and the
eigen-solver's plans at small n against the Gram-matrix path and the default plan."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import cluster_oracle as CO  # noqa: E402  (checker only)
from selfmask_amd import voting as VT  # noqa: E402
from test_oracle_spectral import agreement, blobs, scene  # noqa: E402

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TUNING = os.path.join(ROOT, "salient-object-detection_amd", "lib", "libselfmask_hip_tuning.so")


def run(x, sizes=(2, 3, 4), n_neighbors=10, **kw):
    labels, det = VT.spectral_cluster(torch.from_numpy(x)[None].to(DEV), sizes, n_neighbors, return_details=True, **kw)
    return labels[0].cpu().numpy(), {k: v[0].cpu().numpy() for k, v in det.items()}


def brute_knn(x, rows, m):
    """fp64 brute force for the sampled rows: (neighbour lists by (distance, index), gap between the m-th and the (m+1)-th)"""
    x64 = x.astype(np.float64)
    sq = (x64 * x64).sum(1)
    d = sq[rows, None] + sq[None, :] - 2.0 * (x64[rows] @ x64.T)
    d[np.arange(len(rows)), rows] = np.inf
    order = np.argsort(d, axis=1, kind="stable")
    s = np.take_along_axis(d, order[:, :m + 1], 1)
    return order[:, :m], s[:, m] - s[:, m - 1]


def laplacian(knn):
    import scipy.sparse as sp
    n, m = knn.shape
    c = sp.csr_matrix((np.ones(n * m), (np.repeat(np.arange(n), m), knn.reshape(-1))), shape=(n, n))
    c.data[:] = 1.0  # (a repeated index counts once, as in the device's graph)
    w = (c + c.T) * 0.5
    d = np.asarray(w.sum(1)).ravel()
    s = sp.diags(1.0 / np.sqrt(d))
    return sp.identity(n) - s @ w @ s, d


@pytest.mark.parametrize("n,k", [(9216, 3), (16384, 4), (32768, 2)])
def test_separable_features_come_back_as_the_true_partition(n, k):
    x, truth = blobs(n, k, seed=n + k)
    labels, det = run(x, (k,))
    assert agreement(truth, labels[0], k) == 1.0
    assert det["info"][2] == 1 and det["residuals"].max() <= 1e-8, det["info"]
    assert np.abs(det["eigenvalues"]).max() <= 1e-9


@pytest.mark.parametrize("g,k,seed", [(96, 3, 5), (128, 4, 6), (180, 3, 7)])
def test_every_stage_against_its_restatement(g, k, seed):
    import scipy.sparse.linalg as sla
    x, truth = scene(g, k, seed)
    n = g * g
    labels, det = run(x)
    knn = det["knn"]
    m = knn.shape[1]
    assert knn.min() >= 0 and knn.max() < n and all(i not in knn[i] for i in range(0, n, 97))
    rows = np.random.Generator(np.random.PCG64(seed)).choice(n, 512, replace=False)
    ref, gap = brute_knn(x, rows, m)
    bad = [r for r in range(len(rows)) if set(knn[rows[r]]) != set(ref[r])]
    assert all(gap[r] <= 2e-3 for r in bad) and len(bad) <= len(rows) // 200, (len(bad), [gap[r] for r in bad][:5])
    assert (knn[rows] == ref).mean() >= 0.995  # nearest first
    # eigenpairs on the device's own graph (sparse)
    lap, d = laplacian(knn)
    assert det["info"][2] == 1, det["info"]
    v = det["embedding"] * np.sqrt(d)[:, None]
    lam = det["eigenvalues"]
    assert np.abs(lap @ v - v * lam[None]).max() <= 1e-8
    assert np.abs(v.T @ v - np.eye(v.shape[1])).max() <= 1e-10
    want = np.sort(sla.eigsh(lap.tocsc(), k=4, sigma=-1e-3, which="LM", return_eigenvectors=False))
    assert np.abs(lam - want).max() <= 1e-10, (lam, want)
    for i, kk in enumerate((2, 3, 4)):
        assert np.array_equal(labels[i], CO.kmeans_embedding(det["embedding"][:, :kk], kk))
    assert agreement(truth, labels[(2, 3, 4).index(k)], k) >= 0.9


def test_batched_deterministic_and_limits():
    xs = np.stack([scene(128, 3, s)[0] for s in (21, 22)])
    lab, det = VT.spectral_cluster(torch.from_numpy(xs).to(DEV), (2, 3), return_details=True)
    assert lab.shape == (2, 2, 16384) and det["embedding"].shape == (2, 16384, 3) and det["knn"].shape == (2, 16384, 9)
    for i in range(2):
        one, od = VT.spectral_cluster(torch.from_numpy(xs[i:i + 1]).to(DEV), (2, 3), return_details=True)
        assert torch.equal(one[0], lab[i])
        for key in ("knn", "eigenvalues", "embedding", "residuals"):
            assert torch.equal(od[key][0], det[key][i]), key
    again, ad = VT.spectral_cluster(torch.from_numpy(xs).to(DEV), (2, 3), return_details=True)
    assert torch.equal(again, lab) and torch.equal(ad["embedding"], det["embedding"])
    with pytest.raises(ValueError, match="32768"):
        VT.spectral_cluster(torch.zeros(1, 32772, 384, device=DEV), (2,))


def test_non_finite_features_do_not_fault():
    x = scene(111, 2, 3)[0][:12288].copy()
    x[5] = np.nan
    x[77, 3] = np.inf
    x[4000:4010] = np.inf
    lab, det = VT.spectral_cluster(torch.from_numpy(x)[None].to(DEV), (2, 3, 4), return_details=True)
    torch.cuda.synchronize()
    knn = det["knn"][0].cpu().numpy()
    assert lab.shape == (1, 3, 12288) and int(lab.min()) >= 0 and int(lab.max()) <= 3
    assert knn.min() >= 0 and knn.max() < 12288 and all(i not in knn[i] for i in (5, 77, 4003))


def tuning_run(code, env):
    if not os.path.exists(TUNING):
        pytest.skip("tuning library not built (salient-object-detection_amd/build.py --tuning)")
    r = subprocess.run([sys.executable, "-c", code, ROOT], env={**os.environ, "SM_HIP_LIB": TUNING, **env}, capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def result_hashes(grids):
    """SHA-1 of labels, eigenvalues, embedding, residuals and iteration counts of a batch of two scenes per g x g grid"""
    import hashlib
    out = {}
    for g in grids:
        x = torch.from_numpy(np.stack([scene(g, 3, 60 + s)[0] for s in range(2)])).to(DEV)
        labels, det = VT.spectral_cluster(x, (2, 3, 4), return_details=True)
        h = hashlib.sha1()
        for t in (labels, det["eigenvalues"], det["embedding"], det["residuals"], det["info"][:, :3]):
            h.update(t.cpu().numpy().tobytes())
        out[str(g)] = h.hexdigest()
    return out


HASHES = r"""
import json, os, sys
sys.path[:0] = [os.path.join(sys.argv[1], "salient-object-detection_amd"), sys.argv[1], os.path.join(sys.argv[1], "tests")]
from test_hip_spectral_large import result_hashes
print("RESULT " + json.dumps(result_hashes((28, 44, 56))))
"""

# result_hashes of the library whose graph had a second builder (an n x n bitmap at n <= 8192), on an MI355X: n = 16 (too small for
# that library's list build to run), 100, 784, 1936 and 3136
PINNED_HASHES = {"4": "d8669297eece5e9f0eb4aedc5f1f9d59f7825e82", "10": "36c7e00310d71b075b4e6e35beb99d739df2500e",
                 "28": "ec4a7dec049cb86974961a1adb1a25a9582734c9", "44": "1bb626eb05cf67785e6d79cadd27a93c91e32066",
                 "56": "ab432744c71f25f24315e39b7eb82c06491fe963"}


def test_list_graph_build_gives_the_same_bits():
    """the O(n m) list build (in-degree count, scan, scatter, sorted reverse segments) at n <= 8192: the same lists as the bitmap
    build it replaced, so the same labels, eigenvalues, embedding and residuals bit for bit"""
    assert result_hashes((4, 10, 28, 44, 56)) == PINNED_HASHES


@pytest.mark.parametrize("plan", ["cg1", "gather"])
def test_new_eigen_solver_plans_give_the_same_bits(plan):
    """the one-staged-column plan and the gathering plan forced at small n against the default plan"""
    assert tuning_run(HASHES, {"SM_SPECTRAL_PLAN": plan}) == tuning_run(HASHES, {})


def test_streaming_knn_matches_the_gram_path():
    code = r"""
import json, os, sys
import numpy as np, torch
sys.path[:0] = [os.path.join(sys.argv[1], "salient-object-detection_amd"), sys.argv[1], os.path.join(sys.argv[1], "tests")]
from selfmask_amd import voting as VT
from test_oracle_spectral import scene
out = {}
for g in (28, 56, 91):
    x = scene(g, 3, 70 + g)[0][:min(g * g, 8192)]
    _, det = VT.spectral_cluster(torch.from_numpy(x)[None].cuda(), (2, 3), return_details=True)
    out[str(g)] = det["knn"][0].cpu().numpy().tolist()
print("RESULT " + json.dumps(out))
"""
    gram = tuning_run(code, {})
    stream = tuning_run(code, {"SM_SPECTRAL_KNN": "stream"})
    for g in (28, 56, 91):
        x = scene(g, 3, 70 + g)[0][:min(g * g, 8192)]
        a, b = np.asarray(gram[str(g)]), np.asarray(stream[str(g)])
        n, m = a.shape
        assert n in (784, 3136, 8192) and b.min() >= 0 and b.max() < n
        diff = np.flatnonzero((a != b).any(1))
        if len(diff):
            _, gap = brute_knn(x, diff, m)
            assert (gap <= 2e-3).all() and len(diff) <= n // 200, (len(diff), gap.max())


def test_mask_generator_on_large_images(tmp_path):
    from PIL import Image
    from selfmask_amd import MaskFormer, synthetic_state_dict
    from selfmask_amd.datasets import MEAN, STD, synthetic_scene
    from selfmask_amd.mask_generator import MaskGenerator, rle_decode
    patch = 16
    m = MaskFormer(n_queries=20, patch_size=patch, n_decoder_layers=6, return_intermediate=True, use_binary_classifier=True)
    m.load_state_dict(synthetic_state_dict(31, "soft", patch_size=patch), strict=True)
    m = m.to(DEV)
    rng = np.random.Generator(np.random.PCG64(9))
    paths = []
    for i, (h, w) in enumerate([(720, 1280), (1080, 1920), (300, 400)]):
        img, _ = synthetic_scene(rng, h, w)
        p = str(tmp_path / f"img_{i}.png")
        Image.fromarray(img).save(p)
        paths.append(p)
    gen = MaskGenerator(network=m, device=DEV, batch_size=4)
    out = gen(paths)
    for p, (h, w) in zip(paths, [(720, 1280), (1080, 1920), (300, 400)]):
        assert rle_decode(out[p.split("/")[-1]]).shape == (h, w)
    assert out["img_2.png"] == MaskGenerator(network=m, device=DEV, batch_size=4)(paths[2:])["img_2.png"]
    # the 1080p winner, restated on the device: encoder -> spectral_cluster -> labels_to_masks_batch -> vote_mask
    rgb = np.asarray(Image.open(paths[1]).convert("RGB"), np.float32) / np.float32(255.0)
    x = torch.from_numpy(np.ascontiguousarray(((rgb - np.asarray(MEAN, np.float32)) / np.asarray(STD, np.float32)).transpose(2, 0, 1)))[None]
    H, W = x.shape[-2:]
    Hp, Wp = -(-H // patch) * patch, -(-W // patch) * patch
    xp = torch.zeros((1, 3, Hp, Wp))
    xp[:, :, :H, :W] = x
    with torch.no_grad():
        tok = m(xp.to(DEV), encoder_only=True)["patch_tokens"]
        gh, gw = tok.shape[1:3]
        feats = VT.upsample_tokens_aligned(tok.reshape(1, gh * gw, 384), gh, gw, 2).reshape(1, 4 * gh * gw, 384)
        lab = VT.spectral_cluster(feats, (2, 3, 4))
        cands = VT.labels_to_masks_batch(lab, (2, 3, 4), 2 * gh, 2 * gw, patch // 2, H, W)
        want = VT.vote_mask(cands[0])[0].cpu().numpy()
    assert np.array_equal(rle_decode(out["img_1.png"]), want)
