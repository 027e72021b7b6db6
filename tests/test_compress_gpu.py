"""GPU: hunyuanworld_mirror_amd.compression (csrc/compress.hip) against the reference's recorded files (tests/golden/compress_a/) and against
tests/compress_helper.py, which tests/test_compress_cpu.py pins to those files.  The shapes are the smallest that take each path of the
kernels: N = 1, 2, 3 (a 1 x 1 grid, every channel constant), N = 1000 (a crop), N = 1024 (no crop), N = 66049 = 257^2 (more than 256
level-1 rows per block, a one-row tail, the second reduction level), K and N that are no multiple of the 256-lane block, K = N = 65536.

k-means is checked by property, not by label equality: two centroids can lie within rounding of each other for a row and either is then
correct.  Counts measured on MI355X (printed by the tests, copied to profiles/r23_png_compression.md): see that file."""
import json
import math
import os
import shutil

import numpy as np
import pytest
import torch

import compress_helper as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REF = os.path.join(H.GOLDEN, "ref")


def dev(s):
    return {k: v.to(DEV) for k, v in s.items()}


def comp(**kw):
    from hunyuanworld_mirror_amd import PngCompression
    kw.setdefault("verbose", False)
    if "generator" not in kw:
        kw["generator"] = torch.Generator(device=DEV).manual_seed(11)
    return PngCompression(**kw)


def png_bytes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d) if f.endswith(".png"))


def check_planes(got_dir, splats_cpu, what):
    """the written planes against the helper's: equal for scales / opacities / sh0, within one code for means and quats"""
    mine, pre, n = H.planes_of(splats_cpu)
    got = H.reference_planes(got_dir, n)
    meta = json.load(open(os.path.join(got_dir, "meta.json")))
    for k in mine:
        diff = np.abs(mine[k][0].astype(np.int64) - got[k].astype(np.int64))
        if k in ("means", "quats"):
            print(f"{what} {k}: {int((diff > 0).sum())} of {diff.size} codes differ from the helper's")
            assert diff.max() <= 1, k
        else:
            assert diff.max() == 0, k
            assert np.array_equal(np.float32(meta[k]["mins"]), mine[k][1]) and np.array_equal(np.float32(meta[k]["maxs"]), mine[k][2]), k
    return pre, n, meta


@pytest.fixture(scope="module")
def golden_inputs():
    return {k: torch.from_numpy(v) for k, v in np.load(os.path.join(H.GOLDEN, "inputs.npz")).items()}


# ---------------------------------------------------------------- quantise and decode
def test_golden_scene_planes_and_meta(golden_inputs, tmp_path):
    d = str(tmp_path / "g")
    comp(use_sort=False).compress(d, dev(golden_inputs))
    assert sorted(os.listdir(d)) == sorted(os.listdir(REF))
    ref, got = H.reference_planes(REF, 31), H.reference_planes(d, 31)
    for k in ("scales", "opacities", "sh0"):
        assert np.array_equal(ref[k], got[k]), k
    for k in ("means", "quats"):
        diff = np.abs(ref[k].astype(np.int64) - got[k].astype(np.int64))
        print(f"golden {k}: {int((diff > 0).sum())} of {diff.size} codes differ from the reference's")
        assert diff.max() <= 1, k
    rmeta, gmeta = json.load(open(os.path.join(REF, "meta.json"))), json.load(open(os.path.join(d, "meta.json")))
    assert list(rmeta) == list(gmeta)
    for k in rmeta:
        assert list(rmeta[k]) == list(gmeta[k]), k      # exactly the reference's keys, in its order
        assert rmeta[k]["shape"] == gmeta[k]["shape"] and rmeta[k]["dtype"] == gmeta[k]["dtype"], k
    for k in ("scales", "opacities", "sh0"):
        assert rmeta[k]["mins"] == gmeta[k]["mins"] and rmeta[k]["maxs"] == gmeta[k]["maxs"], k
    assert np.array_equal(np.load(os.path.join(REF, "extra.npz"))["arr"], np.load(os.path.join(d, "extra.npz"))["arr"])


def test_decompress_of_the_reference_files_is_bit_equal():
    want = dict(np.load(os.path.join(H.GOLDEN, "ref_decompressed.npz")))
    got = comp().decompress(REF, device=DEV)
    assert list(got) == ["means", "scales", "quats", "opacities", "sh0", "extra"]
    for k in ("scales", "quats", "opacities", "sh0", "extra"):
        assert got[k].device.type == "cuda" and np.array_equal(got[k].cpu().numpy(), want[k]), k
    m = got["means"].cpu().numpy()
    assert np.all(np.abs(m - want["means"]) <= 4 * 2.0 ** -24 * np.abs(want["means"]))


def test_decompress_of_the_reference_kmeans_file_is_bit_equal(tmp_path):
    d = str(tmp_path / "k")
    shutil.copytree(REF, d)
    shutil.copy(os.path.join(H.GOLDEN, "kmeans", "shN.npz"), d)
    meta = json.load(open(os.path.join(d, "meta.json")))
    meta["shN"] = json.load(open(os.path.join(H.GOLDEN, "kmeans", "meta.json")))["shN"]
    json.dump(meta, open(os.path.join(d, "meta.json"), "w"))
    got = comp().decompress(d, device=DEV)["shN"]
    want = np.load(os.path.join(H.GOLDEN, "kmeans_decompressed.npz"))["shN"]
    assert got.dtype == torch.float32 and np.array_equal(got.cpu().numpy(), want)


def test_square_count_is_not_cropped_and_keeps_its_order(tmp_path):
    s = H.scene(1024, degree=None, seed=1)
    d = str(tmp_path / "s")
    comp(use_sort=False).compress(d, dev(s))
    check_planes(d, s, "N=1024")
    assert np.array_equal(np.load(os.path.join(d, "row.npz"))["arr"], np.arange(1024, dtype=np.int32))


@pytest.mark.parametrize("N", [1, 2, 3])
def test_one_cell_grid_every_channel_constant(N, tmp_path):
    s = H.scene(N, degree=None, seed=N)
    d = str(tmp_path / "s")
    c = comp(use_sort=True)
    c.compress(d, dev(s))
    planes = H.reference_planes(d, 1)
    assert all(int(p.max()) == 0 for p in planes.values())
    top = int(torch.argmax(s["opacities"]))
    got = c.decompress(d, device=DEV)
    assert int(got["row"][0]) == top and got["row"].shape == (1,)
    for k in ("scales", "opacities", "sh0"):
        assert torch.equal(got[k].cpu(), s[k][top:top + 1]), k      # code 0 decodes to the minimum, the value itself
    assert torch.allclose(got["means"].cpu(), s["means"][top:top + 1], rtol=8 * 2.0 ** -24, atol=0)
    assert torch.allclose(got["quats"].cpu(), torch.nn.functional.normalize(s["quats"][top:top + 1], dim=-1), rtol=4 * 2.0 ** -24, atol=0)


def test_257_squared_crosses_blocks_and_the_second_reduction_level(tmp_path):
    s = H.scene(257 * 257, degree=None, seed=4)
    d = str(tmp_path / "s")
    comp(use_sort=False).compress(d, dev(s))
    check_planes(d, s, "N=66049")


def test_one_constant_channel_among_varying_ones(tmp_path):
    s = H.scene(64, degree=None, seed=5)
    s["scales"][:, 1] = -3.25
    d = str(tmp_path / "s")
    c = comp(use_sort=False)
    c.compress(d, dev(s))
    check_planes(d, s, "constant channel")
    assert int(H.reference_planes(d, 8)["scales"][:, :, 1].max()) == 0
    got = c.decompress(d, device=DEV)["scales"].cpu()
    assert torch.equal(got[:, 1], torch.full((64,), -3.25)) and torch.isfinite(got).all()


def test_nan_in_a_quantised_field_raises(tmp_path):
    s = H.scene(100, degree=None, seed=6)
    s["scales"][37, 2] = float("nan")
    d = str(tmp_path / "s")
    with pytest.raises(ValueError):
        comp().compress(d, dev(s))
    assert not [f for f in os.listdir(d) if f.endswith(".png") or f == "meta.json"]


def test_degree_zero_shn_writes_no_file_and_decodes_to_zeros(tmp_path):
    s = H.scene(100, degree=0, seed=7)
    assert s["shN"].shape == (100, 0, 3)
    d = str(tmp_path / "s")
    c = comp()
    c.compress(d, dev(s))
    assert not os.path.exists(os.path.join(d, "shN.npz"))
    assert json.load(open(os.path.join(d, "meta.json")))["shN"] == {"shape": [100, 0, 3], "dtype": "float32"}
    got = c.decompress(d, device=DEV)["shN"]
    assert got.shape == (100, 0, 3) and got.dtype == torch.float32


def test_round_trip_error_is_half_a_code(tmp_path):
    """every field comes back within 0.5 (max - min) / (2^b - 1) plus four fp32 roundings of the value (the means in the log domain); shN
    comes back as exactly the dequantised centroid of its label.  N = 1000: cropped to 961 and sorted; the rows are matched through ``row``."""
    s = H.scene(1000, degree=1, seed=8)
    d = str(tmp_path / "s")
    c = comp(n_clusters=64)
    c.compress(d, dev(s))
    got = {k: v.cpu() for k, v in c.decompress(d, device=DEV).items()}
    meta = json.load(open(os.path.join(d, "meta.json")))
    rows = got["row"].long()
    assert rows.shape == (961,) and len(set(rows.tolist())) == 961
    assert set(rows.tolist()) == set(H.crop_indices(s["opacities"]).tolist())
    want = {"means": H.log_transform(s["means"].double()), "scales": s["scales"].double(), "quats": torch.nn.functional.normalize(s["quats"].double(), dim=-1),
            "opacities": s["opacities"].double(), "sh0": s["sh0"].double()}
    for k, w in want.items():
        g = H.log_transform(got[k].double()) if k == "means" else got[k].double()
        mins, maxs = torch.tensor(meta[k]["mins"], dtype=torch.float64), torch.tensor(meta[k]["maxs"], dtype=torch.float64)
        bound = 0.5 * (maxs - mins) / (2 ** (16 if k == "means" else 8) - 1) + 4 * 2.0 ** -24 * torch.maximum(mins.abs(), maxs.abs())
        err = (g - w[rows]).abs().reshape(961, -1)
        print(f"round trip {k}: max error / bound = {float((err / bound).max()):.4f}")
        assert (err <= bound).all(), k
    z = np.load(os.path.join(d, "shN.npz"))
    assert z["centroids"].dtype == np.uint8 and z["centroids"].shape == (64, 9) and z["labels"].dtype == np.uint16 and int(z["centroids"].max()) <= 63
    table = H.dequantise_kmeans(z["centroids"], z["labels"], meta["shN"]["mins"], meta["shN"]["maxs"], 6)
    assert np.array_equal(got["shN"].numpy(), table.reshape(961, 3, 3))
    assert meta["shN"]["quantization"] == 6 and list(meta["shN"]) == ["shape", "dtype", "mins", "maxs", "quantization"]


# ---------------------------------------------------------------- k-means
def clustered(N, D, seed):
    g = torch.Generator().manual_seed(seed)
    proto = torch.randn(37, D, generator=g)
    return proto[torch.randint(0, 37, (N,), generator=g)] + 0.2 * torch.randn(N, D, generator=g)


@pytest.mark.parametrize("D,N,K", [(9, 1000, 300), (24, 961, 64), (45, 4097, 257)])
def test_kmeans_properties_against_the_fp64_helper(D, N, K):
    from hunyuanworld_mirror_amd.compression import _kmeans_l1
    x = clustered(N, D, seed=D)
    init = torch.randperm(N, generator=torch.Generator().manual_seed(N))[:K]
    labels, cent, errors, last = (t.cpu() for t in _kmeans_l1(x.to(DEV), K, init=init.to(DEV)))
    rl, rc, re, rlast = H.kmeans_l1_ref(x, K, init)
    assert labels.dtype == torch.int64 and cent.dtype == torch.float32 and errors.dtype == torch.float64 and cent.shape == (K, D)
    x64 = x.double()
    # near-optimal assignment: the fp32 rounding of a D-term sum of non-negative terms, doubled
    d64 = H.l1_distances(x64, cent.double())
    assigned = d64[torch.arange(N), labels]
    assert (assigned <= (1 + 4 * D * 2.0 ** -24) * d64.min(dim=1).values).all()
    # the centroids are the member means of the last iteration's assignment
    cnt = torch.bincount(last, minlength=K)
    mean = torch.zeros(K, D, dtype=torch.float64).index_add_(0, last, x64) / cnt.clamp(min=1).unsqueeze(1)
    has = cnt > 0
    assert ((cent.double() - mean).abs()[has] <= 2.0 ** -23 * mean.abs()[has] + 1e-38).all()
    print(f"k-means D={D} N={N} K={K}: {int((last != rlast).sum())} rows assigned otherwise than by the fp64 helper (tie margin), "
          f"{int((~has).sum())} empty centroids, {len(errors)} iterations")
    # the error history
    assert len(errors) == len(re), (errors, re)      # the stop rule fired where the helper's did
    assert ((errors - re).abs() <= D * 2.0 ** -23 * re).all(), (errors, re)
    assert (errors[1:] <= errors[:-1]).all(), errors


def test_kmeans_every_row_its_own_centroid():
    """K = N = 65536: distance exactly 0, the labels reach 65535 and survive the uint16 file"""
    from hunyuanworld_mirror_amd import kmeans_l1
    N = 65536
    x = torch.randn(N, 9, generator=torch.Generator().manual_seed(12))
    assert len(torch.unique(x[:, 0])) > N - 64      # rows are distinct: a duplicate pair in nine columns does not happen
    init = torch.randperm(N, generator=torch.Generator().manual_seed(13))
    labels, cent, errors = kmeans_l1(x.to(DEV), N, init=init.to(DEV))
    labels, cent, errors = labels.cpu(), cent.cpu(), errors.cpu()
    inv = torch.empty(N, dtype=torch.int64)
    inv[init] = torch.arange(N)
    assert torch.equal(labels, inv) and int(labels.max()) == 65535
    assert torch.equal(cent, x[init])
    assert errors.tolist() == [0.0, 0.0]      # |0 - 0| <= tol * 0 at t = 1
    assert np.array_equal(labels.numpy().astype(np.uint16).astype(np.int64), labels.numpy())


def test_kmeans_centroid_without_members_keeps_its_value():
    from hunyuanworld_mirror_amd.compression import _kmeans_l1
    x = torch.randn(50, 9, generator=torch.Generator().manual_seed(3))
    x[7] = x[3]
    init = torch.tensor([3, 7, 20, 30])
    labels, cent, errors, last = (t.cpu() for t in _kmeans_l1(x.to(DEV), 4, init=init.to(DEV), max_iter=1, tol=0.0))
    assert not (last == 1).any()      # the lowest index wins the tie
    assert torch.equal(cent[1], x[7]) and torch.isfinite(cent).all()
    assert len(errors) == 1 and math.isfinite(float(errors[0]))


def test_kmeans_clamps_k_and_runs_one_iteration():
    from hunyuanworld_mirror_amd import kmeans_l1
    x = clustered(50, 24, seed=2).to(DEV)
    labels, cent, errors = kmeans_l1(x, 100, max_iter=1, generator=torch.Generator(device=DEV).manual_seed(1))
    assert cent.shape == (50, 24) and labels.shape == (50,) and errors.shape == (1,) and float(errors[0]) == 0.0
    with pytest.raises(ValueError):
        kmeans_l1(x, 4, init=torch.tensor([0, 1, 2, 50], device=DEV))      # a row outside the input


def test_kmeans_is_deterministic():
    from hunyuanworld_mirror_amd.compression import _kmeans_l1
    x = clustered(4097, 45, seed=9).to(DEV)
    init = torch.randperm(4097, generator=torch.Generator().manual_seed(9))[:257].to(DEV)
    a = _kmeans_l1(x, 257, init=init)
    b = _kmeans_l1(x, 257, init=init)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    from hunyuanworld_mirror_amd.compression import _assign
    labels, dist = _assign(x, a[1])      # the assignment on its own gives the returned labels again
    assert torch.equal(labels.long(), a[0])
    d64 = H.l1_distances(x.cpu().double(), a[1].cpu().double())[torch.arange(4097), a[0].cpu()]
    assert ((dist.cpu().double() - d64).abs() <= 45 * 2.0 ** -24 * d64).all()


# ---------------------------------------------------------------- sort
def test_sort_is_an_aligned_permutation_and_fills_every_cell():
    """n = 31, not a power of two: every cell is filled exactly once; the fields stay aligned row by row"""
    from hunyuanworld_mirror_amd import sort_splats
    s = H.scene(961, degree=1, seed=10)
    sd = dev(s)
    before = {k: v.clone() for k, v in sd.items()}
    out = {k: v.cpu() for k, v in sort_splats(sd, verbose=False).items()}
    assert all(torch.equal(sd[k], before[k]) for k in sd)
    rows = out["row"].long()
    assert sorted(rows.tolist()) == list(range(961))
    for k in s:
        assert out[k].dtype == s[k].dtype and torch.equal(out[k], s[k][rows]), k
    assert torch.equal(rows, H.grid_perm(s["means"]))
    with pytest.raises(ValueError):
        sort_splats(dev(H.scene(960, degree=None)), verbose=False)


def test_sorting_makes_the_pngs_smaller(tmp_path):
    s = dev(H.coherent_scene(64, seed=14))
    a, b = str(tmp_path / "sorted"), str(tmp_path / "unsorted")
    comp(use_sort=True).compress(a, s)
    comp(use_sort=False).compress(b, s)
    print(f"PNG bytes sorted / unsorted = {png_bytes(a)} / {png_bytes(b)} = {png_bytes(a) / png_bytes(b):.4f}")
    assert png_bytes(a) < png_bytes(b)


# ---------------------------------------------------------------- end to end
def test_end_to_end_degree_three(tmp_path):
    s = H.scene(961, degree=3, seed=15)
    params = torch.nn.ParameterDict({k: torch.nn.Parameter(v.to(DEV), requires_grad=v.is_floating_point()) for k, v in s.items()})
    before = {k: v.detach().clone() for k, v in params.items()}
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    comp(n_clusters=128).compress(a, params)
    assert all(torch.equal(params[k].detach(), before[k]) for k in before) and list(params.keys()) == list(before)
    assert sorted(os.listdir(a)) == ["means_l.png", "means_u.png", "meta.json", "opacities.png", "quats.png", "row.npz", "scales.png", "sh0.png", "shN.npz"]
    comp(n_clusters=128).compress(b, params)
    for f in sorted(os.listdir(a)):
        if f.endswith(".png"):
            assert open(os.path.join(a, f), "rb").read() == open(os.path.join(b, f), "rb").read(), f
    za, zb = np.load(os.path.join(a, "shN.npz")), np.load(os.path.join(b, "shN.npz"))
    assert np.array_equal(za["centroids"], zb["centroids"]) and np.array_equal(za["labels"], zb["labels"])
    assert za["centroids"].shape == (128, 45)
    got = comp().decompress(a, device=DEV)
    assert list(got) == list(params.keys())      # the order the caller's container gives its fields in
    for k in s:
        assert got[k].shape == s[k].shape and got[k].dtype == s[k].dtype and got[k].device.type == "cuda", k
    rows = got["row"].long().cpu()
    err = (got["shN"].cpu() - s["shN"][rows]).abs().mean()
    print(f"end to end: mean |shN error| {float(err):.4f} with 128 centroids at 6 bits")
    assert float(err) < 0.1      # the clusters of the scene are 0.03 wide and a 6-bit step of the table is about 0.03
