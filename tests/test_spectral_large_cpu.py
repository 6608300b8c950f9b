"""The clusterer's streaming path (8192 < n <= 32768) as the host sees it, no GPU: workspace sizes linear in n, the sizes of the
Gram-matrix path unchanged, and the pseudo-mask generator refusing an oversized file before it runs anything."""
import types

import pytest

from selfmask_amd import _native as N


def ws(B, n, nn=10, kw=4):
    return N.load().sm_spectral_workspace_bytes(B, n, nn, kw)


@pytest.mark.parametrize("n", [8196, 12288, 16384, 32768])
def test_workspace_exists_above_8192_points(n):
    assert ws(1, n) > 0


def test_workspace_is_linear_in_points_and_images():
    assert ws(1, 32768) < 128 << 20
    assert ws(1, 32768) / ws(1, 16384) < 2.2
    assert 1.9 <= ws(2, 32768) / ws(1, 32768) <= 2.1
    assert 1.9 <= ws(2, 12288) / ws(1, 12288) <= 2.1
    assert ws(1, 32772) == 0
    assert ws(1, 40000) == 0


def test_gram_path_sizes_are_unchanged():
    # read from the library before the streaming path existed
    assert ws(1, 784) == 3983872
    assert ws(128, 1900) == 2354192896
    assert ws(1, 8192) == 291897856


def test_oversized_file_is_refused_up_front(tmp_path):
    from PIL import Image
    from selfmask_amd.mask_generator import MaskGenerator
    small = tmp_path / "small.png"
    big = tmp_path / "big.png"
    Image.new("RGB", (64, 48)).save(small)
    Image.new("RGB", (3000, 3000)).save(big)  # 188 x 188 patches at P = 16: 141 376 points
    net = types.SimpleNamespace(encoder=types.SimpleNamespace(patch_size=16))  # only the patch size is read before the check
    gen = MaskGenerator(network=net, device="cpu")
    with pytest.raises(ValueError, match="big.png"):
        gen([str(small), str(big)])
    with pytest.raises(ValueError, match="big.png"):
        list(gen._batches([str(big)]))
    tiny = tmp_path / "tiny.png"
    Image.new("RGB", (8, 8)).save(tiny)  # one patch: 4 points
    with pytest.raises(ValueError, match="tiny.png"):
        gen([str(tiny)])


def test_batch_cap_only_above_8192_points():
    from selfmask_amd.mask_generator import MaskGenerator
    net = types.SimpleNamespace(encoder=types.SimpleNamespace(patch_size=16))
    gen = MaskGenerator(network=net, device="cpu", batch_size=128, max_stream_bytes=1)
    assert gen._points((1080, 1920)) == 4 * 68 * 120
    assert gen._batch_cap((224, 224)) == 128  # 784 points: batch_size, whatever the budget
    assert gen._batch_cap((512, 1024)) == 128  # 32 x 64 patches, 8192 points: still the Gram path
