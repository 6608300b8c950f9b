"""Inputs and the byte comparison shared by the tests of the selected query's up-sampled planes (test_hip_sod_metrics.py,
test_hip_selected_planes.py)."""
import numpy as np


def _masks(seed, B, nq, mh, mw, spread=1.0):
    """spread 1: probabilities in (0, 1), no up-sampled value is clipped; above 1: some values outside [0, 1] on either side"""
    rng = np.random.Generator(np.random.PCG64(seed))
    masks = (spread * (rng.random((B, nq, mh, mw)) - 0.5) + 0.5).astype(np.float32)
    obj = rng.random((B, nq)).astype(np.float32)
    rows = np.zeros((B, 16), np.float32)
    rows[:, 14], rows[:, 15] = obj.argmax(1), rng.integers(0, nq, B)
    return masks, obj, rows


def _u8_of_f64(x):
    """(clip(x) 255).astype(uint8) of the fp64 up-sample, and where x 255 lies within 1e-4 of an integer"""
    v = np.clip(x, 0.0, 1.0) * 255.0
    return v.astype(np.uint8), np.abs(v - np.rint(v)) <= 1e-4


def _compare_planes(got, x64, label):
    want, near = _u8_of_f64(x64)
    share = float(near.mean())
    diff = got.astype(np.int64) - want.astype(np.int64)
    print(f"\n{label}: {int((diff != 0).sum())} of {diff.size} bytes differ, share within 1e-4 of an integer {share:.2e}")
    assert share < 1e-3, label  # holds for the fp64 path itself: the inputs are fit for the comparison
    assert np.abs(diff).max() <= 1 and not (diff != 0)[~near].any(), label
