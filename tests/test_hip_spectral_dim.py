"""The spectral clusterer on the 2048-d points of a ResNet feature type (csrc/spectral.hip through ``sm_spectral_cluster_dim_f32``):
only the neighbour lists depend on the width, so every stage is held to what tests/test_hip_spectral.py holds the 384-d clusterer to -
the lists against the fp64 restatement (allowance scaled by the norms, tests/test_hip_knn_dim.py), the eigenpairs against a dense
``eigh`` of the device's own graph, the k-means of the device's embedding exactly, scikit-learn as the third-party witness."""
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import cluster_oracle as CO  # noqa: E402  (checker only)
from selfmask_amd import voting as VT  # noqa: E402
from test_oracle_spectral import agreement, blobs, scene  # noqa: E402

DEV = "cuda:0"
DIM = 2048


def run(x, sizes=(2, 3, 4), n_neighbors=10):
    labels, det = VT.spectral_cluster(torch.from_numpy(x)[None].to(DEV), sizes, n_neighbors, return_details=True)
    return labels[0].cpu().numpy(), {k: v[0].cpu().numpy() for k, v in det.items()}


@pytest.mark.parametrize("k,seed", [(3, 2), (2, 1)])
def test_every_stage_against_its_restatement(k, seed):
    g, nn = 28, 10
    x, truth = scene(g, k, seed, dim=DIM)
    n = g * g
    labels, det = run(x, (2, 3, 4), nn)
    # stage 2: the neighbour lists
    ref_idx = CO.knn_indices(x, nn)
    gap = CO.knn_boundary_gap(x, nn)
    allowance = 2e-3 * float((x.astype(np.float64) ** 2).sum(1).max()) / 853.5
    bad = [i for i in range(n) if set(det["knn"][i]) != set(ref_idx[i])]
    print(f"k={k} seed={seed}: {len(bad)} differing rows, gaps {[float(gap[i]) for i in bad][:5]} (allowance {allowance:.3e}), "
          f"order agreement {(det['knn'] == ref_idx).mean():.4f}")
    assert all(gap[i] <= allowance for i in bad) and len(bad) <= n // 200
    assert (det["knn"] == ref_idx).mean() >= 0.995
    assert all(i not in det["knn"][i] for i in range(n))
    # stage 4: eigenpairs of the DEVICE's graph against a dense eigh of the same graph
    w = CO.affinity_from_knn(det["knn"])
    vals, vecs, emb = CO.spectral_embedding(w, 4)
    assert det["info"][2] == 1 and det["info"][3] == 0, det["info"]
    assert np.abs(det["eigenvalues"] - vals).max() <= 1e-10
    assert det["residuals"].max() <= 1e-8
    d = w.sum(1)
    lap = np.eye(n) - w / np.sqrt(d)[:, None] / np.sqrt(d)[None, :]
    v = det["embedding"] * np.sqrt(d)[:, None]
    assert np.abs(lap @ v - v * det["eigenvalues"][None]).max() <= 1e-8
    assert np.abs(v.T @ v - np.eye(4)).max() <= 1e-10
    for j in range(4):  # distinct eigenvalues: vectors equal up to sign
        if min(abs(vals[j] - vals[i]) for i in range(4) if i != j) > 1e-6:
            s = np.sign(v[:, j] @ vecs[:, j])
            assert np.abs(v[:, j] * s - vecs[:, j]).max() <= 1e-6
    # stage 5: k-means of the DEVICE's embedding, exactly; and the whole chain through the restatement
    for i, kk in enumerate((2, 3, 4)):
        assert np.array_equal(labels[i], CO.kmeans_embedding(det["embedding"][:, :kk], kk))
        assert (labels[i] == CO.kmeans_embedding(emb[:, :kk], kk)).mean() >= 0.999
    assert agreement(truth, labels[(2, 3, 4).index(k)], k) >= 0.9
    # third-party witness on the same graph
    from sklearn.cluster import SpectralClustering
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sk = SpectralClustering(n_clusters=k, affinity="precomputed", assign_labels="kmeans", random_state=0).fit(w)
    assert agreement(sk.labels_, labels[(2, 3, 4).index(k)], k) >= 0.99


def test_separable_features_come_back_as_the_true_partition():
    x, truth = blobs(784, 3, seed=787, dim=DIM)
    labels, det = run(x, (3,))
    assert agreement(truth, labels[0], 3) == 1.0
    assert det["info"][2] == 1 and det["residuals"].max() <= 1e-8
    assert np.abs(det["eigenvalues"]).max() <= 1e-9  # three components: eigenvalue 0, three times


def test_batched_and_deterministic():
    xs = torch.from_numpy(np.stack([scene(28, 3, s, dim=DIM)[0] for s in (11, 12, 13)])).to(DEV)
    lab = VT.spectral_cluster(xs, (2, 3))
    assert lab.shape == (3, 2, 784) and lab.dtype == torch.int32
    for i in range(3):
        assert torch.equal(VT.spectral_cluster(xs[i:i + 1], (2, 3))[0], lab[i])
    assert torch.equal(VT.spectral_cluster(xs, (2, 3)), lab)
