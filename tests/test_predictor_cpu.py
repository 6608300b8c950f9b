"""Host half of the bulk predictor (selfmask_amd/predictor.py, csrc/predict.hip): the restatement the GPU tests compare against, the
C ABI of the fused finish, its host-side validation, the planner's refusals and the multi-rank branch.  The device half runs in
tests/test_hip_predict.py and tests/test_hip_predictor.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import _predict_ref as R
from selfmask_amd import MaskFormer, _native as N
from selfmask_amd.distributed import shard_indices
from selfmask_amd.mask_generator import rle_decode, rle_encode
from selfmask_amd.predictor import SaliencyPredictor, build_parser


# ---- the restatement's known answers ------------------------------------------------------------------------------------------
def test_restatement_known_answers():
    nq, size = 3, (10, 14)
    obj = np.array([0.1, 0.9, 0.9], np.float32)  # a tie for the top: the first wins
    masks = torch.zeros((nq, 5, 7))
    masks[2] = 1.0
    r = R.finish_one(masks, obj, size, 2.0)
    assert r["best"] == 1 and r["rle"] == {"size": [10, 14], "counts": [140]} and not r["soft"].any()
    masks[1] = 1.0
    r = R.finish_one(masks, obj, size, 2.0)
    assert r["rle"]["counts"] == [0, 140] and (r["soft"] == 255).all()
    one = np.zeros(size, np.uint8)
    one[0, 0] = 1
    assert rle_encode(one)["counts"] == [0, 1, 139]
    masks[1] = 0.0
    masks[1, 0, 0] = 1.0  # the x2 up-sample leaves pixel (0, 0) at 1.0 (clamped taps) and (1, 1) at 0.5625
    r = R.finish_one(masks, obj, size, 2.0)
    assert r["binary"][0, 0] == 1 and r["rle"]["counts"][0] == 0
    # a pixel outside the up-sampled plane is 0
    r = R.finish_one(torch.ones((1, 2, 2)), [1.0], (6, 3), 2.0)
    assert r["binary"][:4].all() and not r["binary"][4:].any()


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_rle_round_trip_mixed_sizes(seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    for h, w in [(1, 1), (1, 9), (7, 1), (17, 23), (250, 333)]:
        m = (rng.random((h, w)) > 0.6).astype(np.uint8)
        assert np.array_equal(rle_decode(rle_encode(m)), m)


# ---- C ABI (its layout: tests/test_abi_cpu.py) ----------------------------------------------------------------------------------
def _err(lib):
    return (lib.sm_last_error() or b"").decode()


def test_validation_without_gpu():
    """every refusal happens on the host before any launch"""
    lib = N.load()
    table = (N.BilateralImage * 1)()
    table[0].H, table[0].W = 4, 4
    a = N.PredictArgs()
    assert lib.sm_predict_masks_f32(a, C.addressof(table), None) == -1 and "null pointer" in _err(lib)
    a.masks, a.objectness, a.images, a.best = 256, 256, 256, 256  # never dereferenced: the shape is refused first
    a.B, a.nq, a.mh, a.mw, a.max_pixels = 0, 20, 4, 4, 16
    assert lib.sm_predict_masks_f32(a, C.addressof(table), None) == -1 and "B=0" in _err(lib)
    a.B, a.nq = 1, 961
    assert lib.sm_predict_masks_f32(a, C.addressof(table), None) == -1 and "nq=961" in _err(lib)
    a.nq = 20
    assert lib.sm_predict_masks_f32(a, None, None) == -1 and "null pointer" in _err(lib)
    table[0].H = 5  # 20 pixels > max_pixels
    assert lib.sm_predict_masks_f32(a, C.addressof(table), None) == -1 and "max_pixels" in _err(lib)
    table[0].H = 4
    a.starts = 256  # starts without info
    assert lib.sm_predict_masks_f32(a, C.addressof(table), None) == -1 and "starts and info" in _err(lib)
    assert lib.sm_rle_runs_packed_u8(None, None, None, 1, None, 16, None, None, 0, None) == -1 and "null pointer" in _err(lib)
    assert lib.sm_rle_runs_packed_u8(256, 256, C.addressof(table), 0, 256, 16, 256, 256, 0, None) == -1


def test_padded_runs_validation_without_gpu():
    """sm_rle_runs_u8 walks with the predictor's workspace: a missing, misaligned or short one and a plane the walk does not take are
    refused on the host, with a message"""
    lib = N.load()
    need = lib.sm_predict_workspace_bytes(2, 64 * 80)

    def call(H, W, ws, nbytes):  # the pointers are never dereferenced: every case is refused first
        return lib.sm_rle_runs_u8(256, 2, H, W, None, 256, 16, 256, ws, nbytes, None)

    assert call(64, 80, None, need) == -1 and "null pointer" in _err(lib)
    assert call(64, 80, 256 + 64, need) == -1 and "misaligned" in _err(lib)
    assert call(64, 80, 256, need - 1) == -1 and "too small" in _err(lib)
    assert call(1, (1 << 22) + 1, 256, 1 << 30) == -1 and "4194304 pixels" in _err(lib)
    assert call(2049, 2048, 256, 1 << 30) == -1 and "4194304 pixels" in _err(lib)
    assert lib.sm_rle_runs_u8(256, 65536, 4, 4, None, 256, 16, 256, 256, 1 << 30, None) == -1 and "65535 masks" in _err(lib)


def test_workspace_bytes_positive_and_monotone():
    lib = N.load()
    prev_b = 0
    for B in (1, 2, 7, 64, 128):
        prev_p = 0
        for px in (1, 4096, 4097, 120000, 1080 * 1920, 1 << 22):
            n = lib.sm_predict_workspace_bytes(B, px)
            assert n > 0 and n % 256 == 0 and n >= prev_p
            prev_p = n
        assert prev_p >= prev_b
        prev_b = prev_p
    assert lib.sm_predict_workspace_bytes(0, 100) == 0 and lib.sm_predict_workspace_bytes(1, 0) == 0
    assert lib.sm_predict_workspace_bytes(1, (1 << 22) + 1) == 0


# ---- planner ----------------------------------------------------------------------------------------------------------------------
class _Net:
    """a network as far as the planner looks at it; any forward would fail"""
    use_binary_classifier = True

    class encoder:
        patch_size = 16

    def __call__(self, *a, **k):
        raise AssertionError("the planner must refuse before anything runs")


def _png(path, h, w):
    from PIL import Image
    Image.fromarray(np.zeros((h, w, 3), np.uint8)).save(path)
    return str(path)


def test_planner_refuses_before_any_device_call(tmp_path, monkeypatch):
    p = SaliencyPredictor(_Net())
    monkeypatch.setattr(p, "_run", lambda *a, **k: pytest.fail("queued work although the plan is invalid"))
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    one, two = _png(tmp_path / "a" / "x.png", 20, 30), _png(tmp_path / "b" / "x.png", 20, 30)
    with pytest.raises(ValueError, match="x.png"):
        p([one, two])
    with pytest.raises(FileNotFoundError, match="missing.jpg"):
        p([one, str(tmp_path / "missing.jpg")])
    bad = tmp_path / "broken.png"
    bad.write_bytes(b"not an image")
    with pytest.raises(ValueError, match="broken.png"):
        p([one, str(bad)])
    with pytest.raises(ValueError, match="soft"):
        p([one], output="soft", refine="bilateral")
    with pytest.raises(ValueError, match="output"):
        p([one], output="png")
    with pytest.raises(ValueError, match="refine"):
        p([one], refine="crf")
    # native buckets by token grid; plain slices when resized
    files = [_png(tmp_path / f"{i}.png", h, w) for i, (h, w) in enumerate([(20, 30), (40, 30), (17, 31), (33, 20)])]
    assert p._plan(files, None, ("rle",), None)[3] == [[0, 2], [1, 3]]
    p.batch_size = 3
    assert p._plan(files, 224, ("rle",), None)[3] == [[0, 1, 2], [3]]


def test_no_cpu_fallback():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SaliencyPredictor(_Net(), device="cpu")
    m = MaskFormer(n_queries=20, patch_size=16, n_decoder_layers=6, return_intermediate=True, use_binary_classifier=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SaliencyPredictor(m)
    net = _Net()
    net.use_binary_classifier = False
    with pytest.raises(RuntimeError, match="use_binary_classifier"):
        SaliencyPredictor(net)


# ---- multi-rank branch ------------------------------------------------------------------------------------------------------------
class _FakeComm:
    """one of two ranks run one after the other in this process: gather_bytes (patched below) keeps a board of payloads"""

    def __init__(self, rank, world, board):
        self.rank, self.world_size, self.board, self.calls = rank, world, board, 0


def test_multi_rank_branch_shards_and_merges_in_list_order(tmp_path, monkeypatch):
    files = [_png(tmp_path / f"im{i}.png", 16 + i, 20) for i in range(5)]
    names = [f.split("/")[-1] for f in files]
    board = {}
    took = {}

    def gather_bytes(payload, comm, device="cpu"):
        slot = board.setdefault(comm.calls, {})
        slot[comm.rank] = payload
        comm.calls += 1
        return [slot.get(r, b"") for r in range(comm.world_size)]

    monkeypatch.setattr("selfmask_amd.distributed.gather_bytes", gather_bytes)
    out = {}
    for rnd in range(2):  # the first round fills the board with every rank's payload, the second reads the complete board
        for rank in range(2):
            p = SaliencyPredictor(_Net())

            def run(paths, img_size, scale_factor, outputs, refine, plan=None, p=p, rank=rank):
                took[rank] = [q.split("/")[-1] for q in paths]
                assert plan is not None and plan[0] == list(paths) and plan[2] == [(16 + int(n[2]), 20) for n in took[rank]]  # no second probe
                p.last_best = {n: int(n[2]) for n in took[rank]}
                return {"rle": {n: {"size": [1, 1], "counts": [int(n[2]) + 1]} for n in took[rank]}}

            monkeypatch.setattr(p, "_run", run)
            comm = _FakeComm(rank, 2, board)
            if rnd == 0:
                try:
                    p(files, comm=comm)
                except KeyError:  # the other rank's shard is not on the board yet
                    pass
            else:
                out[rank] = (p(files, comm=comm), p.last_best)
    assert took[0] == [names[i] for i in shard_indices(5, 0, 2)] and took[1] == [names[i] for i in shard_indices(5, 1, 2)]
    for rank in range(2):
        res, best = out[rank]
        assert list(res) == names and list(best) == names
        assert [res[n]["counts"][0] for n in names] == [1, 2, 3, 4, 5] and [best[n] for n in names] == [0, 1, 2, 3, 4]
    with pytest.raises(AssertionError, match="run-length"):
        SaliencyPredictor(_Net())(files, output="binary", comm=_FakeComm(0, 2, {}))


# ---- CLI --------------------------------------------------------------------------------------------------------------------------
def test_cli_help_and_defaults():
    with pytest.raises(SystemExit) as e:
        build_parser().parse_args(["--help"])
    assert e.value.code == 0
    a = build_parser().parse_args(["--config", "c.yaml", "--p_state_dict", "w.pt", "--images", "dir", "--out", "o.json"])
    assert a.img_size is None and a.batch_size == 64 and a.refine is None and a.png_dir is None
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--config", "c", "--p_state_dict", "w", "--images", "d", "--out", "o", "--refine", "crf"])
