"""Writes tests/golden/export_{a,b,c}.npz: the inputs of three small splat sets and the REFERENCE's own bytes for them in the three
formats of gsplat's export_splats, run on the CPU.  Data only.

    python tools/gen_golden_export.py <reference gsplat package dir (the one that holds exporter.py)>

exporter.py is loaded by file path (it imports only math, struct, io, numpy and torch: no CUDA extension is touched).

Scenes
  a   N = 700, K = 15: every row kept, two full chunks of 256 plus a part chunk of 188; shN wide enough that some sh bytes clamp.
  b   N = 300, K = 0: what the forward pass itself produces.  Rows with NaN / +-Inf in means, scales, quats and sh0 (none in the
      opacities: the reference would drop every row), and rows whose sigmoid(opacity) is under 1 / 255.  (With K = 0 shN is empty and
      cannot hold a NaN; scene c carries those rows.)
  c   N = 600, K = 3: means snapped to a lattice of 6 values per axis, so that many Morton codes tie; rows with NaN / Inf in shN.
Asserted of every scene, for the rows each format keeps, so that the goldens pin what they are meant to pin:
  * no chunk of ply_compressed has max == min in any of its nine quantities (the reference's 0 / 0)
  * argmax |q / |q|| is unique per row (the two largest magnitudes differ)
  * |sigmoid(opacity) - 1 / 255| > 1e-4
  * a, b: torch.argsort(codes) equals torch.argsort(codes, stable=True) for the reference's own Morton codes (no two rows tie)
  * c: at least 100 rows share their Morton code with another row.  The reference calls torch.argsort WITHOUT stable=True, and on the
    CPU that sort does move equal codes (measured here: with any tie among ~600 rows it never returned them in row order, presorted
    input included), so the order of tied records in the reference's own output is whatever the sort leaves.  This project defines
    it: equal codes stay in row order.  For scene c alone the reference therefore runs with torch.argsort forced to stable=True
    (stable_argsort below; nothing else of it changes), and the tool asserts that the untouched reference gives the same "ply" bytes
    and, for "splat", the same multiset of records with the same sequence of means-derived codes: it differs in the order inside
    tie groups and in nothing else.
and the restatement tests/export_helper.py reproduces all nine byte strings exactly."""
import contextlib
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import export_helper as EH  # noqa: E402


def load_reference(pkg_dir):
    spec = importlib.util.spec_from_file_location("reference_exporter", os.path.join(pkg_dir, "exporter.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@contextlib.contextmanager
def stable_argsort():
    """torch.argsort with stable=True for the duration: the tie order this project defines (see the module text, scene c)"""
    orig = torch.argsort
    torch.argsort = lambda x, *a, **k: orig(x, *a, **{**k, "stable": True})
    try:
        yield
    finally:
        torch.argsort = orig


def _base(g, N, K, sh_std):
    return dict(means=torch.randn(N, 3, generator=g) * torch.tensor([2.0, 1.0, 3.0]),
                scales=torch.randn(N, 3, generator=g) * 1.2 - 3.0,
                quats=torch.randn(N, 4, generator=g),
                opacities=torch.rand(N, generator=g) * 8.0 - 4.0,
                sh0=torch.randn(N, 1, 3, generator=g) * 1.5,
                shN=torch.randn(N, K, 3, generator=g) * sh_std)


def scene_a():
    g = torch.Generator().manual_seed(101)
    s = _base(g, 700, 15, 2.5)
    s["scales"][5, 1] = -25.0          # past the +-20 clamp of the chunk bounds
    s["scales"][300, 2] = 21.5
    return s


def scene_b():
    g = torch.Generator().manual_seed(102)
    s = _base(g, 300, 0, 1.0)
    bad = [float("nan"), float("inf"), float("-inf")]
    for j, (name, row) in enumerate([("means", 3), ("means", 150), ("scales", 17), ("scales", 299), ("quats", 0), ("quats", 77), ("sh0", 42),
                                     ("sh0", 201), ("means", 202)]):
        t = s[name].reshape(300, -1)
        t[row, j % t.shape[1]] = bad[j % 3]
    s["opacities"][torch.arange(10, 300, 23)] = -8.0 - torch.rand(13, generator=g)          # sigmoid < 1 / 255
    return s


def scene_c():
    g = torch.Generator().manual_seed(103)
    s = _base(g, 600, 3, 2.0)
    s["means"] = torch.randint(0, 6, (600, 3), generator=g).float() * torch.tensor([0.5, 0.25, 1.5]) - 1.0
    s["shN"][11, 2, 1] = float("nan")
    s["shN"][400, 0, 0] = float("inf")
    s["shN"][599, 1, 2] = float("-inf")
    return s


def check_scene(ref, name, s, outs):
    K = s["shN"].shape[1]
    for fmt in ("splat", "ply_compressed"):
        keep = EH.keep_mask(*[s[k] for k in EH.NAMES], fmt)
        m, q, o = s["means"][keep], s["quats"][keep], s["opacities"][keep]
        codes = ref.encode_morton3_vec(*ref_scaled(ref, m))
        u, cnt = torch.unique(codes, return_counts=True)
        if name != "c":
            assert int(cnt.max()) == 1 and torch.equal(torch.argsort(codes), torch.argsort(codes, stable=True)), (name, fmt, "a tie")
            assert torch.equal(ref.sort_centers(m, torch.arange(m.shape[0])), torch.argsort(codes, stable=True))
        else:
            with stable_argsort():
                assert torch.equal(ref.sort_centers(m, torch.arange(m.shape[0])), torch.argsort(codes, stable=True))
        assert torch.equal(codes.to(torch.int64), EH.morton_codes(m)), (name, "helper codes")
        qa = (q / torch.linalg.norm(q, dim=-1, keepdim=True)).abs().sort(dim=1, descending=True).values
        assert bool((qa[:, 0] > qa[:, 1]).all()), (name, "argmax |q| not unique")
        assert float((torch.sigmoid(s["opacities"][torch.isfinite(s["opacities"])]) - 1 / 255).abs().min()) > 1e-4
        if name == "c":
            assert int(cnt[cnt > 1].sum()) >= 100, int(cnt[cnt > 1].sum())
    _, n, sec = EH.split(outs["ply_compressed"], "ply_compressed", K)
    ch = sec["chunks"].view("<f4").reshape(-1, 3, 2, 3)
    assert (ch[:, :, 0, :] != ch[:, :, 1, :]).all(), (name, "a chunk with a zero range")
    return n


def ref_scaled(ref, centers):
    """the reference's quantised coordinates, by the lines of its sort_centers"""
    mn, _ = torch.min(centers, dim=0)
    mx, _ = torch.max(centers, dim=0)
    ln = mx - mn
    ln[ln == 0] = 1
    sc = ((centers - mn) / ln * 1024).floor().to(torch.int32)
    return sc[:, 0], sc[:, 1], sc[:, 2]


def main(pkg_dir):
    ref = load_reference(pkg_dir)
    gold = os.path.join(ROOT, "tests", "golden")
    expect = {"a": (700, 15), "b": (300, 0), "c": (600, 3)}
    for name, s in (("a", scene_a()), ("b", scene_b()), ("c", scene_c())):
        assert (s["means"].shape[0], s["shN"].shape[1]) == expect[name]
        assert bool(torch.isfinite(s["opacities"]).all())
        run = lambda: {fmt: ref.export_splats(*[s[k].clone() for k in EH.NAMES], format=fmt) for fmt in EH.FORMATS}  # noqa: E731
        if name == "c":
            with stable_argsort():
                outs = run()
            raw = run()
            rec = lambda b: np.frombuffer(b, np.uint8).reshape(-1, 32)  # noqa: E731
            assert raw["ply"] == outs["ply"] and len(raw["ply_compressed"]) == len(outs["ply_compressed"])
            assert sorted(map(bytes, rec(raw["splat"]))) == sorted(map(bytes, rec(outs["splat"])))
            code_of = lambda b: EH.morton_codes(torch.from_numpy(rec(b)[:, :12].copy().view("<f4").reshape(-1, 3)))  # noqa: E731
            assert torch.equal(code_of(raw["splat"]), code_of(outs["splat"]))
            print("c: the untouched reference orders", int((rec(raw["splat"]) != rec(outs["splat"])).any(axis=1).sum()), "of", len(rec(raw["splat"])),
                  "splat records differently inside tie groups")
        else:
            outs = run()
        n_c = check_scene(ref, name, s, outs)
        kept = {}
        for fmt in EH.FORMATS:
            mine, kept[fmt] = EH.export_splats(*[s[k] for k in EH.NAMES], format=fmt)
            assert mine == outs[fmt], (name, fmt, "tests/export_helper.py does not reproduce the reference's bytes")
        assert kept["ply_compressed"] == n_c
        if name == "a":
            assert kept["ply_compressed"] == 700
        if name == "b":
            assert kept["ply"] == 300 - 9 and kept["ply_compressed"] < kept["ply"] - 5
        if name == "c":
            assert kept["ply"] == 597
        path = os.path.join(gold, f"export_{name}.npz")
        np.savez_compressed(path, **{k: s[k].numpy() for k in EH.NAMES}, **{fmt: np.frombuffer(outs[fmt], np.uint8) for fmt in EH.FORMATS})
        print(name, "kept", kept, {fmt: len(outs[fmt]) for fmt in EH.FORMATS}, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
