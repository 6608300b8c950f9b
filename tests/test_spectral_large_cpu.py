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


# sm_spectral_workspace_bytes(B, n, n_neighbors, kw) as the library returned it when the graph had two builders (a bitmap at
# n <= 8192): (B, n) -> the values for n_neighbors in (2, 10, 33), each for kw in (1, 4, 6).  MaskGenerator's batch caps rest on them.
WORKSPACE_BYTES = {
    (1, 16): (29952, 30208, 30464, 31488, 31744, 32000, 32512, 32768, 33024),
    (1, 20): (37632, 38144, 38400, 39424, 39936, 40192, 41728, 42240, 42496),
    (1, 64): (127488, 129024, 130048, 133632, 135168, 136192, 151296, 152832, 153856),
    (1, 784): (3889920, 3908608, 3921152, 3965184, 3983872, 3996416, 4181504, 4200192, 4212736),
    (1, 1900): (18165248, 18210816, 18241280, 18347776, 18393344, 18423808, 18872064, 18917632, 18948096),
    (1, 8192): (290914816, 291111424, 291242496, 291701248, 291897856, 292028928, 293962240, 294158848, 294289920),
    (1, 8196): (14328576, 14525184, 14656256, 15639808, 15836416, 15967488, 19409920, 19606528, 19737600),
    (1, 16384): (28640000, 29033216, 29295360, 31261440, 31654656, 31916800, 38798080, 39191296, 39453440),
    (1, 32768): (57279232, 58065664, 58589952, 62522112, 63308544, 63832832, 77595392, 78381824, 78906112),
    (3, 16): (87040, 88064, 88832, 91648, 92672, 93440, 95232, 96256, 97024),
    (3, 20): (109312, 110848, 111872, 115200, 116736, 117760, 122112, 123648, 124672),
    (3, 64): (381696, 386304, 389376, 400128, 404736, 407808, 453120, 457728, 460800),
    (3, 784): (11666944, 11723264, 11760896, 11892736, 11949056, 11986688, 12541952, 12598272, 12635904),
    (3, 1900): (54493952, 54630656, 54721792, 55041024, 55177728, 55268864, 56614144, 56750848, 56841984),
    (3, 8192): (872743680, 873333504, 873726720, 875102976, 875692800, 876086016, 881885952, 882475776, 882868992),
    (3, 8196): (42982144, 43572224, 43965696, 46916096, 47506176, 47899648, 58226688, 58816768, 59210240),
    (3, 16384): (85918976, 87098624, 87885056, 93783296, 94962944, 95749376, 116393216, 117572864, 118359296),
    (3, 32768): (171836672, 174195968, 175768832, 187565312, 189924608, 191497472, 232785152, 235144448, 236717312),
    (128, 16): (3686912, 3736064, 3768832, 3883520, 3932672, 3965440, 4030976, 4080128, 4112896),
    (128, 20): (4645376, 4706816, 4747776, 4891136, 4952576, 4993536, 5198336, 5259776, 5300736),
    (128, 64): (16269824, 16466432, 16597504, 17056256, 17252864, 17383936, 19317248, 19513856, 19644928),
    (128, 784): (497762816, 500171264, 501776896, 507396608, 509805056, 511410688, 535093760, 537502208, 539107840),
    (128, 1900): (2325008896, 2330845696, 2334736896, 2348356096, 2354192896, 2358084096, 2415479296, 2421316096, 2425207296),
    (128, 8192): (37237047808, 37262213632, 37278990848, 37337711104, 37362876928, 37379654144, 37627118080, 37652283904, 37669061120),
    (128, 8196): (1833839104, 1859017216, 1875802624, 2001693184, 2026871296, 2043656704, 2484273664, 2509451776, 2526237184),
    (128, 16384): (3665854976, 3716186624, 3749741056, 4001399296, 4051730944, 4085285376, 4966089216, 5016420864, 5049975296),
    (128, 32768): (7331676672, 7432339968, 7499448832, 8002765312, 8103428608, 8170537472, 9932145152, 10032808448, 10099917312),
}


@pytest.mark.parametrize("B,n", sorted(WORKSPACE_BYTES))
def test_workspace_sizes_are_pinned(B, n):
    assert [ws(B, n, nn, kw) for nn in (2, 10, 33) for kw in (1, 4, 6)] == list(WORKSPACE_BYTES[B, n])


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
