"""CPU: the torch restatement tests/export_helper.py against the reference's own bytes (tests/golden/export_{a,b,c}.npz, written by
tools/gen_golden_export.py from gsplat's export_splats), the headers hunyuanworld_mirror_amd.exporter writes, its PLY reader, and the
argument checks of the C ABI entries, which come before any launch and so answer without a GPU.

Scene c's tied Morton codes: the reference sorts with an unstable torch.argsort, which on the CPU returns tied rows in no defined
order; the goldens of scene c are the reference's bytes with that one call made stable (row order inside a tie, the order this
project defines; see the generator)."""
import ctypes as C

import numpy as np
import pytest
import torch

import export_helper as EH
from hunyuanworld_mirror_amd import _lib, exporter

WM_OK, WM_ERR_INVALID = 0, 1
SCENES = {"a": (700, 15), "b": (300, 0), "c": (600, 3)}


@pytest.mark.parametrize("fmt", EH.FORMATS)
@pytest.mark.parametrize("name", sorted(SCENES))
def test_helper_reproduces_the_reference_bytes(name, fmt):
    z = EH.load_golden(name)
    t = EH.scene_tensors(z)
    assert (t[0].shape[0], t[5].shape[1]) == SCENES[name]
    got, n = EH.export_splats(*t, format=fmt)
    r = EH.compare(got, z[fmt].tobytes(), fmt, SCENES[name][1])
    print(f"{name} {fmt}: {n} kept, {r['flips']} fields off by one (cap {EH.flip_cap(n)}), exp(scale) max {r['max_ulp']} ulp; "
          f"identical: {got == z[fmt].tobytes()}")
    assert r["n"] == n


def test_golden_scenes_are_what_they_are_meant_to_be():
    kept = {}
    for name in SCENES:
        z = EH.load_golden(name)
        t = EH.scene_tensors(z)
        kept[name] = {fmt: int(EH.keep_mask(*t, fmt).sum()) for fmt in EH.FORMATS}
        assert bool(torch.isfinite(t[3]).all())                    # no non-finite opacity: the reference would drop every row
    assert kept["a"] == {"ply": 700, "splat": 700, "ply_compressed": 700}          # two full chunks and a part chunk
    assert kept["b"]["ply"] == 291 and kept["b"]["ply_compressed"] == 278          # non-finite rows, rows under the opacity threshold
    assert kept["c"]["ply"] == 597                                                   # the three rows with a non-finite shN
    t = EH.scene_tensors(EH.load_golden("c"))
    m = t[0][EH.keep_mask(*t, "splat")]
    _, cnt = torch.unique(EH.morton_codes(m), return_counts=True)
    assert int(cnt[cnt > 1].sum()) >= 100                          # many tied Morton codes
    for name in SCENES:                                            # no chunk with a zero range: the reference's 0 / 0 is not in the goldens
        ch = EH.split(EH.load_golden(name)["ply_compressed"].tobytes(), "ply_compressed", SCENES[name][1])[2]["chunks"]
        ch = ch.view("<f4").reshape(-1, 3, 2, 3)
        assert (ch[:, :, 0, :] != ch[:, :, 1, :]).all()


@pytest.mark.parametrize("K", [0, 3, 8, 15])
def test_headers(K):
    for n in (0, 1, 256, 257, 70000):
        assert exporter.ply_header(n, K) == EH.header("ply", n, K)
        assert exporter.ply_compressed_header(n, K) == EH.header("ply_compressed", n, K)
    assert exporter.float_ply_header(5, exporter.GS_PLY_ATTRIBUTES) == EH.float_header(5, EH.GS_PLY_PROPS)
    assert list(exporter.GS_PLY_ATTRIBUTES) == ["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2", "opacity", "scale_0", "scale_1",
                                                "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"]


@pytest.mark.parametrize("name", sorted(SCENES))
def test_headers_match_the_reference_files(name):
    z = EH.load_golden(name)
    K = SCENES[name][1]
    for fmt, fn in (("ply", exporter.ply_header), ("ply_compressed", exporter.ply_compressed_header)):
        data = z[fmt].tobytes()
        head, n, _ = EH.split(data, fmt, K)
        assert fn(n, K) == head and data.startswith(head)


def _scene(n=40, seed=5):
    g = torch.Generator().manual_seed(seed)
    return dict(means=torch.randn(n, 3, generator=g), scales=torch.rand(n, 3, generator=g) * 0.1 + 0.01, quats=torch.randn(n, 4, generator=g),
                rgbs=torch.randn(n, 3, generator=g), opacities=torch.rand(n, generator=g))


def test_load_gaussian_ply_reads_both_writers_and_a_permuted_file(tmp_path):
    # the layout of export_splats(format="ply"): golden a (K = 15), rows as the reference wrote them
    z = EH.load_golden("a")
    p = tmp_path / "a.ply"
    p.write_bytes(z["ply"].tobytes())
    pos, sh, op, sc, rot = exporter.load_gaussian_ply(p)
    for got, want in ((pos, z["means"]), (sh, z["sh0"][:, 0]), (op, z["opacities"]), (sc, z["scales"]), (rot, z["quats"])):
        assert got.dtype == torch.float32 and got.device.type == "cpu" and np.array_equal(got.numpy(), want)
    # the layout of save_gs_ply
    s = _scene()
    data, n = EH.save_gs_ply(s["means"], s["scales"], s["quats"], s["rgbs"], s["opacities"])
    p = tmp_path / "gs.ply"
    p.write_bytes(data)
    keep = s["scales"].max(-1)[0] <= torch.quantile(s["scales"].max(-1)[0], 0.95)
    pos, sh, op, sc, rot = exporter.load_gaussian_ply(str(p))
    assert pos.shape == (n, 3) and n == int(keep.sum()) and n < 40
    assert torch.equal(pos, s["means"][keep]) and torch.equal(sh, s["rgbs"][keep]) and torch.equal(op, s["opacities"][keep])
    assert torch.equal(sc, s["scales"][keep].log()) and torch.equal(rot, s["quats"][keep])
    # columns in another order, two columns nobody asks for, a comment line
    names = ["rot_3", "extra_a", "scale_2", "x", "f_dc_1", "opacity", "z", "rot_0", "scale_0", "y", "f_dc_2", "rot_1", "extra_b", "f_dc_0", "scale_1",
             "rot_2"]
    cols = {"x": s["means"][:, 0], "y": s["means"][:, 1], "z": s["means"][:, 2], "opacity": s["opacities"], "extra_a": torch.full((40,), 7.0),
            "extra_b": torch.arange(40.0)}
    for j in range(3):
        cols[f"f_dc_{j}"], cols[f"scale_{j}"] = s["rgbs"][:, j], s["scales"][:, j]
    for j in range(4):
        cols[f"rot_{j}"] = s["quats"][:, j]
    head = "ply\nformat binary_little_endian 1.0\ncomment made by a test\nelement vertex 40\n" + "".join(f"property float {n}\n" for n in names)
    p = tmp_path / "perm.ply"
    p.write_bytes((head + "end_header\n").encode() + torch.stack([cols[n] for n in names], dim=1).numpy().astype("<f4").tobytes())
    pos, sh, op, sc, rot = exporter.load_gaussian_ply(p)
    assert torch.equal(pos, s["means"]) and torch.equal(sh, s["rgbs"]) and torch.equal(op, s["opacities"])
    assert torch.equal(sc, s["scales"]) and torch.equal(rot, s["quats"])
    # what the reader refuses
    bad = tmp_path / "bad.ply"
    bad.write_bytes(b"ply\nformat binary_little_endian 1.0\nelement vertex 1\nproperty uchar x\nend_header\n\0")
    with pytest.raises(ValueError):
        exporter.load_gaussian_ply(bad)
    bad.write_bytes(b"ply\nformat ascii 1.0\nelement vertex 0\nproperty float x\nend_header\n")
    with pytest.raises(ValueError):
        exporter.load_gaussian_ply(bad)
    bad.write_bytes((head + "end_header\n").encode() + b"\0" * 100)          # a truncated body
    with pytest.raises(ValueError):
        exporter.load_gaussian_ply(bad)


def test_splats_from_ply_is_the_trainers_ffgs_branch(tmp_path):
    s = _scene()
    data, n = EH.save_gs_ply(s["means"], s["scales"], s["quats"], s["rgbs"], s["opacities"])
    p = tmp_path / "gs.ply"
    p.write_bytes(data)
    keep = s["scales"].max(-1)[0] <= torch.quantile(s["scales"].max(-1)[0], 0.95)
    out = exporter.splats_from_ply(p, sh_degree=2, device="cpu")
    assert {k: tuple(v.shape) for k, v in out.items()} == {"means": (n, 3), "scales": (n, 3), "quats": (n, 4), "opacities": (n,), "sh0": (n, 1, 3),
                                                          "shN": (n, 8, 3)}
    assert torch.equal(out["opacities"], torch.logit(torch.clamp(s["opacities"][keep], 1e-6, 1 - 1e-6)))
    assert torch.equal(out["sh0"][:, 0], s["rgbs"][keep]) and not out["shN"].any()
    assert torch.equal(out["scales"], s["scales"][keep].log())
    raw = exporter.splats_from_ply(p, opacity="logit", device="cpu")
    assert torch.equal(raw["opacities"], s["opacities"][keep]) and raw["shN"].shape == (n, 0, 3)
    with pytest.raises(ValueError):
        exporter.splats_from_ply(p, opacity="sigmoid", device="cpu")


def test_cpu_tensors_raise_and_the_unbuilt_writer_says_so(tmp_path):
    t = EH.scene_tensors(EH.load_golden("b"))
    for fmt in EH.FORMATS:
        with pytest.raises(RuntimeError):
            exporter.export_splats(*t, format=fmt)
    with pytest.raises(ValueError):
        exporter.export_splats(*t, format="obj")
    with pytest.raises(AssertionError):
        exporter.export_splats(t[0], t[1], t[2], t[3], t[4][:, 0], t[5])          # gsplat's shape checks: sh0 must be [N,1,3]
    s = _scene()
    with pytest.raises(RuntimeError):
        exporter.save_gs_ply(tmp_path / "x.ply", s["means"], s["scales"], s["quats"], s["rgbs"], s["opacities"])
    with pytest.raises(NotImplementedError):
        exporter.process_ply_to_splat(tmp_path / "x.ply")


def test_size_rules():
    L = _lib.lib()
    for n, K in ((0, 0), (1, 0), (256, 3), (257, 15), (70000, 0)):
        assert L.wm_export_splats_payload_bytes(n, K, 0) == n * (14 + 3 * K) * 4
        assert L.wm_export_splats_payload_bytes(n, K, 1) == n * 32
        assert L.wm_export_splats_payload_bytes(n, K, 2) == ((n + 255) // 256) * 72 + n * 16 + n * 3 * K
        for fmt in (0, 1, 2):
            assert L.wm_export_splats_workspace_bytes(n, K, fmt) >= 20 * n + (1 << 20)
        assert L.wm_export_splats_workspace_bytes(n, K, 1) == L.wm_export_splats_workspace_bytes(n, K, 2) > L.wm_export_splats_workspace_bytes(n, K, 0)
        assert L.wm_pack_rows_workspace_bytes(n) == L.wm_export_splats_workspace_bytes(n, K, 0)
    for bad in ((-1, 0, 0), (1 << 31, 0, 0), (10, 16, 0), (10, -1, 0), (10, 0, 3), (10, 0, -1)):
        assert L.wm_export_splats_workspace_bytes(*bad) == 0 and L.wm_export_splats_payload_bytes(*bad) == 0
    assert L.wm_pack_rows_workspace_bytes(-1) == 0 and L.wm_pack_rows_workspace_bytes(1 << 31) == 0


def test_c_abi_argument_checks_come_before_any_launch():
    """Every refused call returns WM_ERR_INVALID without touching a device: the pointers below are host buffers (or made up), and this
    test runs on a machine without a GPU."""
    L = _lib.lib()
    buf = (C.c_char * 4096)()
    fake = C.cast(buf, C.c_void_p)
    n_kept = C.c_int(-7)
    N, K = 10, 3
    ws_need, out_need = L.wm_export_splats_workspace_bytes(N, K, 2), L.wm_export_splats_payload_bytes(N, K, 2)

    def call(means=fake, scales=fake, quats=fake, opac=fake, sh0=fake, shN=fake, n=N, k=K, fmt=2, ws=fake, ws_bytes=None, out=fake, out_bytes=None,
             nk=C.byref(n_kept)):
        return L.wm_export_splats(means, scales, quats, opac, sh0, shN, n, k, fmt, 1 / 255, ws, ws_need if ws_bytes is None else ws_bytes, out,
                                  out_need if out_bytes is None else out_bytes, nk, None)

    for kw in (dict(means=None), dict(scales=None), dict(quats=None), dict(opac=None), dict(sh0=None), dict(shN=None), dict(ws=None), dict(out=None),
               dict(nk=None), dict(n=-1), dict(n=1 << 31), dict(n=(1 << 31) + 5), dict(k=-1), dict(k=16), dict(fmt=3), dict(fmt=-1),
               dict(ws_bytes=ws_need - 1), dict(ws_bytes=0), dict(out_bytes=out_need - 1)):
        assert call(**kw) == WM_ERR_INVALID, kw
    assert n_kept.value == -7                                        # a refused call writes nothing
    # N = 0 is a legal call that launches nothing: null tensors and a null output
    assert call(means=None, scales=None, quats=None, opac=None, sh0=None, shN=None, out=None, n=0, ws_bytes=L.wm_export_splats_workspace_bytes(0, K, 2),
                out_bytes=0) == WM_OK and n_kept.value == 0

    ptrs, strides, xfs = (C.c_void_p * 3)(fake, None, fake), (C.c_int * 3)(3, 0, 1), (C.c_int * 3)(0, 0, 1)
    pw = L.wm_pack_rows_workspace_bytes(N)
    n_kept.value = -7

    def pack(p=ptrs, s=strides, x=xfs, nc=3, keep=None, n=N, ws=fake, ws_bytes=pw, out=fake, out_bytes=N * 3 * 4, nk=C.byref(n_kept)):
        return L.wm_pack_rows(p, s, x, nc, keep, n, ws, ws_bytes, out, out_bytes, nk, None)

    for kw in (dict(p=None), dict(s=None), dict(x=None), dict(nc=0), dict(nc=65), dict(n=-1), dict(n=1 << 31), dict(ws=None), dict(ws_bytes=pw - 1),
               dict(out=None), dict(out_bytes=N * 3 * 4 - 1), dict(nk=None), dict(s=(C.c_int * 3)(3, -1, 1)), dict(x=(C.c_int * 3)(0, 2, 1)),
               dict(x=(C.c_int * 3)(-1, 0, 1))):
        assert pack(**kw) == WM_ERR_INVALID, kw
    assert n_kept.value == -7
    assert pack(n=0, out=None, out_bytes=0, ws_bytes=L.wm_pack_rows_workspace_bytes(0)) == WM_OK and n_kept.value == 0
