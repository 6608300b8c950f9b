"""The neighbour lists as an operation of their own (``selfmask_amd.voting.knn`` = ``sm_knn_f32``, csrc/spectral.hip) at both feature
widths the spectral clusterer takes - 384 (DINO tokens) and 2048 (the ResNet maps) - and by both methods: a Gram matrix on the matrix
cores, and the streaming kernels that never form one (at 2048 dimensions: products accumulated over chunks of 64 features).  The
checker is the fp64 restatement ``oracle.cluster_oracle.knn_indices``; the rule is stage 2 of
tests/test_hip_spectral.py::test_every_stage_against_its_restatement, with the allowance scaled by the norms: the products carry
22 bits of |f|^2, and the 2e-3 of that test was set on ``scene(28, 3, 2)``, whose largest |f|^2 is 853.5."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import cluster_oracle as CO  # noqa: E402  (checker only)
from selfmask_amd import _native as N  # noqa: E402
from selfmask_amd import voting as VT  # noqa: E402
from test_oracle_spectral import scene  # noqa: E402

gpu = pytest.mark.gpu
DEV = "cuda:0"

# name -> (grids / seeds of the images, k, n_neighbors)
CASES = {
    "n100_b2": (((10, 5), (10, 6)), 3, 10),   # tails in the 64-row block and in the 32- / 64-column tiles; two images
    "n784_nn10": (((28, 2),), 3, 10),         # CAP 16
    "n784_nn20": (((28, 2),), 3, 20),         # CAP 32
    "n16_nn33": (((4, 7),), 2, 33),           # m clipped to n - 1 = 15
}


@functools.lru_cache(maxsize=None)
def case(name, dim):
    """-> (features (B, n, dim) float32, reference lists [(n, m)], sorted fp64 distances to the others [(n, n - 1)], allowance [B])"""
    imgs, k, nn = CASES[name]
    xs = np.stack([scene(g, k, seed, dim=dim)[0] for g, seed in imgs])
    refs, dists, allow = [], [], []
    for x in xs:
        refs.append(CO.knn_indices(x, nn))
        x64 = x.astype(np.float64)
        sq = (x64 * x64).sum(1)
        d = sq[:, None] + sq[None, :] - 2.0 * (x64 @ x64.T)
        d[np.arange(len(x)), np.arange(len(x))] = -np.inf
        dists.append(np.sort(d, axis=1)[:, 1:])
        allow.append(2e-3 * float(sq.max()) / 853.5)
    for a in (xs, *refs, *dists):
        a.setflags(write=False)
    return xs, refs, dists, allow


def row_gap(dist_row, m):
    """the smallest gap between consecutive distances among a row's m nearest and the first one left out: a list may legitimately
    differ from the fp64 one only where two of these are closer than the products resolve"""
    d = dist_row[:m + 1]
    return float(np.diff(d).min()) if len(d) > 1 else np.inf


def device_knn(xs, nn, method):
    out = VT.knn(torch.from_numpy(xs).to(DEV), nn, method)
    torch.cuda.synchronize()
    assert out.dtype == torch.int32
    return out.cpu().numpy()


@gpu
@pytest.mark.parametrize("method", ["gram", "stream"])
@pytest.mark.parametrize("dim", [384, 2048])
@pytest.mark.parametrize("name", sorted(CASES))
def test_neighbour_lists_against_the_restatement(name, dim, method):
    xs, refs, dists, allow = case(name, dim)
    nn = CASES[name][2]
    B, n = xs.shape[:2]
    m = min(nn - 1, n - 1)
    got = device_knn(xs, nn, method)
    assert got.shape == (B, n, m)
    for b in range(B):
        g, ref = got[b], refs[b]
        assert g.min() >= 0 and g.max() < n
        assert all(i not in g[i] for i in range(n))
        gap = CO.knn_boundary_gap(xs[b], nn)
        bad = [i for i in range(n) if set(g[i]) != set(ref[i])]
        order = float((g == ref).mean())
        print(f"{name} D={dim} {method} image {b}: {len(bad)} differing rows (cap {n // 200}), gaps {[float(gap[i]) for i in bad][:5]} "
              f"(allowance {allow[b]:.3e}), order agreement {order:.4f}")
        assert len(bad) <= n // 200 and all(gap[i] <= allow[b] for i in bad)
        assert order >= 0.995


@gpu
def test_width_384_keeps_the_clusterers_lists_and_the_old_entry_point_its_labels():
    xs, _, _, _ = case("n784_nn10", 384)
    f = torch.from_numpy(xs).to(DEV)
    labels, det = VT.spectral_cluster(f, (2, 3, 4), 10, return_details=True)
    for method in ("gram", "auto"):
        assert torch.equal(VT.knn(f, 10, method), det["knn"]), method
    # the entry point without a width is the 384 call of the new one
    lib = N.load()
    nbytes = lib.sm_spectral_workspace_bytes(1, 784, 10, 4)
    assert nbytes == lib.sm_spectral_workspace_bytes_dim(1, 784, 384, 10, 4) > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    old = torch.empty((1, 3, 784), dtype=torch.int32, device=DEV)
    a = N.SpectralArgs()
    sizes = (C.c_int32 * 3)(2, 3, 4)
    a.features, a.labels, a.cluster_sizes = f.data_ptr(), old.data_ptr(), C.cast(sizes, C.POINTER(C.c_int32))
    a.workspace, a.workspace_bytes, a.tol = ws.data_ptr(), nbytes, 1e-9
    a.B, a.n, a.n_sizes, a.n_neighbors, a.degree, a.max_outer = 1, 784, 3, 10, 24, 60
    torch.cuda.synchronize()
    N.check(lib.sm_spectral_cluster_f32(C.byref(a), torch.cuda.current_stream().cuda_stream), "sm_spectral_cluster_f32")
    torch.cuda.synchronize()
    assert torch.equal(old, labels)


@gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_width_2048_gram_and_stream_differ_only_within_the_allowance(name):
    xs, _, dists, allow = case(name, 2048)
    nn = CASES[name][2]
    a, b = device_knn(xs, nn, "gram"), device_knn(xs, nn, "stream")
    m = a.shape[2]
    for img in range(xs.shape[0]):
        rows = np.flatnonzero((a[img] != b[img]).any(1))
        gaps = [row_gap(dists[img][i], m) for i in rows]
        print(f"{name} image {img}: {len(rows)} rows differ between gram and stream, gaps {gaps[:5]} (allowance {allow[img]:.3e})")
        assert all(g <= allow[img] for g in gaps)
    assert np.array_equal(device_knn(xs, nn, "stream"), b)  # and a repeat gives the same bits


@gpu
def test_above_8192_points_slabs_and_stream_agree_and_sampled_rows_match_the_restatement():
    """8448 points (the smallest multiple of 64 above 8192 that leaves a partial last slab: 4 x 2048 + 256 rows): "gram" forms the matrix
    in slabs, "stream" never forms it.  All rows: the two differ only within the allowance.  64 sampled rows (the slab borders, the
    last row, 57 random ones) against fp64 distances: the stage-2 rule at the sample's size (at most ceil(64 / 200) = 1 row)."""
    n, nn, m = 8448, 10, 9
    x = scene(92, 3, 4, dim=2048)[0][:n]
    a, b = device_knn(x[None], nn, "gram")[0], device_knn(x[None], nn, "stream")[0]
    auto = device_knn(x[None], nn, "auto")[0]
    assert np.array_equal(auto, a) or np.array_equal(auto, b)  # whichever the clusterer takes at this width
    x64 = x.astype(np.float64)
    sq = (x64 * x64).sum(1)
    allowance = 2e-3 * float(sq.max()) / 853.5

    def others(i):  # sorted fp64 distances of row i to the other points, and their indices
        d = sq[i] + sq - 2.0 * (x64 @ x64[i])
        d[i] = -np.inf
        o = np.argsort(d, kind="stable")[1:]
        return d[o], o

    rows = np.flatnonzero((a != b).any(1))
    gaps = [row_gap(others(i)[0], m) for i in rows]
    print(f"n={n}: {len(rows)} rows differ between slabs and stream, gaps {gaps[:5]} (allowance {allowance:.3e})")
    assert len(rows) <= n // 200 and all(g <= allowance for g in gaps)
    sample = sorted({0, 1, 2047, 2048, 4095, 4096, 8191, 8192, 8447} | set(np.random.Generator(np.random.PCG64(3)).integers(0, n, 55).tolist()))
    for got in (a, b):
        assert got.min() >= 0 and got.max() < n and all(i not in got[i] for i in sample)
        bad = []
        for i in sample:
            d, o = others(i)
            if set(got[i]) != set(o[:m]):
                bad.append(float(d[m] - d[m - 1]))
        assert len(bad) <= 1 and all(g <= allowance for g in bad), bad


@gpu
@pytest.mark.parametrize("method", ["gram", "stream"])
@pytest.mark.parametrize("dim", [384, 2048])
def test_non_finite_rows_do_not_fault(dim, method):
    x = case("n784_nn10", dim)[0].copy()
    x[0, 5] = np.nan
    x[0, 77, 3] = np.inf
    got = device_knn(x, 10, method)
    assert got.shape == (1, 784, 9) and got.min() >= 0 and got.max() < 784


@gpu
def test_python_argument_checks():
    with pytest.raises(ValueError, match="knn"):
        VT.knn(torch.zeros(1, 64, 512, device=DEV))
    with pytest.raises(ValueError, match="knn"):
        VT.knn(torch.zeros(1, 8, 384, device=DEV))
    with pytest.raises(ValueError, match="knn"):
        VT.knn(torch.zeros(1, 64, 384, device=DEV), method="faiss")
    with pytest.raises(ValueError, match="spectral_cluster"):
        VT.spectral_cluster(torch.zeros(1, 64, 512, device=DEV), (2,))
    with pytest.raises(RuntimeError, match="HIP device"):
        VT.knn(torch.zeros(1, 64, 384))


def test_c_argument_checks_run_before_any_launch():
    """every check of sm_knn_f32 / sm_spectral_cluster_dim_f32 is host arithmetic: callable without a GPU (the pointers are never followed)"""
    lib = N.load()
    p = 1 << 20  # non-null, 256-B aligned, never dereferenced
    ok = lib.sm_knn_workspace_bytes(2, 100, 2048, 10, 2)
    assert ok > 0 and lib.sm_knn_workspace_bytes(2, 100, 2048, 10, 1) > ok  # the Gram matrix
    assert lib.sm_knn_workspace_bytes(1, 100, 384, 10, 0) == lib.sm_knn_workspace_bytes(1, 100, 384, 10, 1)
    # above 8192 points: streaming holds no matrix, "gram" one slab of 2048 rows; the workspace stays linear in n
    stream, slabs = lib.sm_knn_workspace_bytes(1, 16384, 2048, 10, 2), lib.sm_knn_workspace_bytes(1, 16384, 2048, 10, 1)
    assert 0 < stream < slabs == stream + 2048 * 16384 * 4
    assert lib.sm_knn_workspace_bytes(1, 16384, 384, 10, 0) == lib.sm_knn_workspace_bytes(1, 16384, 384, 10, 2)  # 384-d: streaming, as before
    assert lib.sm_knn_workspace_bytes(1, 16384, 2048, 10, 0) in (stream, slabs)
    for B, n, D, nn, method, word in ((1, 100, 512, 10, 0, b"features per point"), (1, 8, 384, 10, 0, b"points"), (1, 102, 384, 10, 0, b"points"),
                                      (1, 100, 384, 40, 0, b"n_neighbors"), (1, 32772, 384, 10, 2, b"points"), (1, 100, 384, 10, 3, b"method")):
        assert lib.sm_knn_workspace_bytes(B, n, D, nn, method) == 0
        assert lib.sm_knn_f32(p, B, n, D, nn, method, p, p, 1 << 40, None) == -1
        assert word in lib.sm_last_error(), lib.sm_last_error()
    assert lib.sm_knn_f32(p, 2, 100, 2048, 10, 2, p, p, ok - 1, None) == -1 and b"workspace" in lib.sm_last_error()
    assert lib.sm_knn_f32(None, 2, 100, 2048, 10, 2, p, p, ok, None) == -1 and b"null pointer" in lib.sm_last_error()
    # the clusterer at a width
    assert lib.sm_spectral_workspace_bytes_dim(1, 784, 512, 10, 4) == 0
    assert lib.sm_spectral_workspace_bytes_dim(1, 784, 2048, 10, 4) > lib.sm_spectral_workspace_bytes_dim(1, 784, 384, 10, 4) > 0
    a = N.SpectralArgs()
    sizes = (C.c_int32 * 1)(2)
    a.features = a.labels = a.workspace = p
    a.cluster_sizes = C.cast(sizes, C.POINTER(C.c_int32))
    a.workspace_bytes, a.B, a.n, a.n_sizes, a.n_neighbors = 1 << 40, 1, 784, 1, 10
    assert lib.sm_spectral_cluster_dim_f32(C.byref(a), 512, None) == -1 and b"features per point" in lib.sm_last_error()
    a.workspace_bytes = 256
    assert lib.sm_spectral_cluster_dim_f32(C.byref(a), 2048, None) == -1 and b"workspace" in lib.sm_last_error()
