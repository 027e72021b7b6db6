"""CPU: tests/compress_helper.py (the restatement the GPU tests hold the kernels against) pinned to what the reference's PngCompression wrote
and read back (tests/golden/compress_a/, recorded by tools/gen_golden_compress.py), and the argument checks of the package's compression
module, which must raise before any GPU call."""
import json
import os

import numpy as np
import pytest
import torch

import compress_helper as H

REF = os.path.join(H.GOLDEN, "ref")


@pytest.fixture(scope="module")
def golden():
    inputs = {k: torch.from_numpy(v) for k, v in np.load(os.path.join(H.GOLDEN, "inputs.npz")).items()}
    meta = json.load(open(os.path.join(REF, "meta.json")))
    dec = dict(np.load(os.path.join(H.GOLDEN, "ref_decompressed.npz")))
    return inputs, meta, dec


def test_golden_is_the_cropped_scene(golden):
    inputs, meta, _ = golden
    assert inputs["means"].shape == (1000, 3) and meta["means"]["shape"] == [961, 3]
    assert sorted(os.listdir(REF)) == ["extra.npz", "means_l.png", "means_u.png", "meta.json", "opacities.png", "quats.png", "scales.png", "sh0.png"]
    assert list(meta) == ["means", "scales", "quats", "opacities", "sh0", "extra"]
    assert len(torch.unique(inputs["opacities"])) == 1000      # distinct: the reference's unstable argsort has one answer


def test_helper_planes_match_the_reference_files(golden):
    """scales, opacities, sh0: equal codes.  means (16 bit) and quats: log1p and the normalisation run in front of the quantiser and may
    differ by an ulp between implementations; one ulp of a value in [0, 1] is 2^-24 * 65535 = 0.004 codes, so a difference can only be a
    flip at a rounding boundary: within +-1 code.  The share of differing codes is counted, not bounded."""
    inputs, meta, _ = golden
    mine, pre, n = H.planes_of(inputs)
    ref = H.reference_planes(REF, n)
    assert n == 31
    for k in ("scales", "opacities", "sh0"):
        assert np.array_equal(mine[k][0], ref[k]), k
    for k in ("means", "quats"):
        diff = np.abs(mine[k][0].astype(np.int64) - ref[k].astype(np.int64))
        print(f"{k}: {int((diff > 0).sum())} of {diff.size} codes differ from the reference's")
        assert diff.max() <= 1, k
    for k in H.PNG_FIELDS:
        lim = 0 if k in ("scales", "opacities", "sh0") else 2.0 ** -22
        assert np.all(np.abs(mine[k][1] - np.float32(meta[k]["mins"])) <= lim * np.abs(mine[k][1])), k
        assert np.all(np.abs(mine[k][2] - np.float32(meta[k]["maxs"])) <= lim * np.abs(mine[k][2])), k
    extra = np.load(os.path.join(REF, "extra.npz"))["arr"]
    assert np.array_equal(extra, pre["extra"].numpy())      # the crop keeps the reference's rows in the reference's order


def test_helper_decoders_are_bit_equal_to_the_reference(golden):
    _, meta, dec = golden
    ref = H.reference_planes(REF, 31)
    for k in ("scales", "quats", "opacities", "sh0"):
        got = H.dequantise(ref[k].reshape(961, -1), meta[k]["mins"], meta[k]["maxs"], 8).reshape(meta[k]["shape"])
        assert np.array_equal(got, dec[k]), k
    logm = H.dequantise(ref["means"].reshape(961, 3), meta["means"]["mins"], meta["means"]["maxs"], 16)
    means = H.inverse_log_transform(torch.from_numpy(logm)).numpy()
    assert np.all(np.abs(means - dec["means"]) <= 4 * 2.0 ** -24 * np.abs(dec["means"]))      # expm1 may differ by an ulp or two


def test_helper_kmeans_decoder_is_bit_equal_to_the_reference():
    d = os.path.join(H.GOLDEN, "kmeans")
    meta = json.load(open(os.path.join(d, "meta.json")))["shN"]
    z = np.load(os.path.join(d, "shN.npz"))
    assert z["centroids"].shape == (300, 24) and z["centroids"].dtype == np.uint8 and z["labels"].shape == (961,) and z["labels"].dtype == np.uint16
    got = H.dequantise_kmeans(z["centroids"], z["labels"], meta["mins"], meta["maxs"], meta["quantization"]).reshape(meta["shape"])
    want = np.load(os.path.join(H.GOLDEN, "kmeans_decompressed.npz"))["shN"]
    assert np.array_equal(got, want)


def test_helper_quantiser_constant_channel_and_half_to_even():
    x = torch.tensor([[0.0, 7.0], [1.0, 7.0], [2.0, 7.0]])      # 0.5 * 255 = 127.5 -> 128 (even); the second channel is constant
    codes, mins, maxs = H.quantise(x, 8)
    assert codes[:, 0].tolist() == [0, 128, 255] and codes[:, 1].tolist() == [0, 0, 0]
    assert np.array_equal(H.dequantise(codes, mins, maxs, 8)[:, 1], np.float32([7, 7, 7]))


def test_helper_kmeans_empty_centroid_keeps_its_value():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(50, 9, generator=g)
    x[7] = x[3]
    labels, cent, errors, last = H.kmeans_l1_ref(x, 4, torch.tensor([3, 7, 20, 30]), max_iter=1, tol=0.0)
    assert not (last == 1).any()      # the lower index wins the tie, so in iteration 0 centroid 1 has no members ...
    assert torch.equal(cent[1], x[7].double()) and torch.isfinite(cent).all()      # ... and keeps its value
    assert labels[3] == 1 and labels[7] == 1      # centroid 0 has moved; the final assignment finds the two rows at distance 0 of centroid 1
    assert len(errors) == 1


def test_helper_grid_perm_fills_every_cell_once():
    for n in (1, 2, 31, 64):
        g = torch.Generator().manual_seed(n)
        perm = H.grid_perm(torch.randn(n * n, 3, generator=g))
        assert sorted(perm.tolist()) == list(range(n * n))


def test_argument_checks_raise_before_any_gpu_call(monkeypatch, tmp_path):
    from hunyuanworld_mirror_amd import PngCompression, _lib, kmeans_l1, sort_splats

    def no_library():
        raise AssertionError("the library was asked for before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", no_library)
    monkeypatch.setattr(torch.Tensor, "cuda", lambda *a, **k: (_ for _ in ()).throw(AssertionError("a tensor was moved to the GPU")))
    s = H.scene(16, degree=1, with_row=False)
    comp = PngCompression(verbose=False)
    with pytest.raises(RuntimeError):      # host tensors
        comp.compress(str(tmp_path / "a"), s)
    with pytest.raises(RuntimeError):
        sort_splats(s, verbose=False)
    with pytest.raises(RuntimeError):
        kmeans_l1(torch.randn(20, 9), 4)
    with pytest.raises(RuntimeError):
        kmeans_l1(np.zeros((20, 9), np.float32), 4)
    with pytest.raises(ValueError):        # no splats
        comp.compress(str(tmp_path / "b"), {k: v[:0] for k, v in s.items()})
    bad = dict(s)
    bad["scales"] = s["scales"][:15]
    with pytest.raises(ValueError):        # first dimensions differ
        comp.compress(str(tmp_path / "c"), bad)
    with pytest.raises(ValueError):
        sort_splats(bad, verbose=False)
    with pytest.raises(ValueError):
        kmeans_l1(torch.randn(20, 10), 4)      # D outside 9, 24, 45
    with pytest.raises(ValueError):
        kmeans_l1(torch.randn(0, 9), 4)
    with pytest.raises(ValueError):
        PngCompression(quantization=9)
    assert not os.path.exists(tmp_path / "a") and not os.path.exists(tmp_path / "b") and not os.path.exists(tmp_path / "c")


def test_public_names_are_exported():
    import hunyuanworld_mirror_amd as pkg
    c = pkg.PngCompression()
    assert c.use_sort is True and c.verbose is True and c.n_clusters == 65536 and c.quantization == 6 and c.max_iter == 15 and c.tol == 1e-4
    assert callable(pkg.kmeans_l1) and callable(pkg.sort_splats)
