"""bench.py's bookkeeping, checked without a GPU: every timing kind has algorithmic FLOPs, the per-kernel rows add up to their
classes, the totals are BASELINE.md's (42 TFLOP per 8-view forward at 518 x 518, 7.94 TFLOP per cross-view attention launch at
32 views), and the kinds named here are the kinds include/wm_hip.h documents."""
import importlib.util
import os
import re

from conftest import ROOT


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b


def test_flop_model_rows_add_up_to_their_classes():
    from hunyuanworld_mirror_amd import WMConfig
    b = _bench()
    cfg = WMConfig()
    for n_local, n_total in ((8, 8), (32, 32), (8, 64)):
        fl = b.flop_model(cfg, n_local, n_total, 518, 518)
        for name in b.KINDS.values():
            assert name in fl and fl[name] >= 0, name
        assert abs(sum(v for k, v in fl.items() if k.startswith("gemm_")) - fl["gemm"]) < 1e-6 * fl["gemm"]
        assert abs(sum(v for k, v in fl.items() if k.startswith("dpt_") and k != "dpt_conv") - fl["dpt_conv"]) < 1e-6 * fl["dpt_conv"]
        parts = fl["gemm"] + fl["dpt_conv"] + fl["global_attention"] + fl["frame_dino_attention"]
        assert parts <= fl["total"] <= parts * 1.01
    c2 = b.flop_model(cfg, 8, 8, 518, 518)
    assert abs(c2["total"] / 1e12 - 42.0) < 0.5
    c3 = b.flop_model(cfg, 32, 32, 518, 518)
    assert abs(c3["global_attention"] / 24 / 1e12 - 7.94) < 0.02     # per launch at 32 views
    c4 = b.flop_model(cfg, 8, 64, 518, 518)
    assert abs(c4["global_attention"] / c2["global_attention"] - 8.0) < 1e-9   # 8 x the keys per rank at 8 ranks


def test_timing_kinds_match_the_header():
    b = _bench()
    hdr = open(os.path.join(ROOT, "include", "wm_hip.h")).read()
    doc = hdr[hdr.index("/* kind:"):hdr.index("wm_status wm_profile_enable")]
    documented = {int(x) for x in re.findall(r"(\d+)(?: / (\d+))? =", doc) for x in x if x}
    assert set(b.KINDS) | {4} <= documented, (sorted(b.KINDS), sorted(documented))
    assert b.PEAK_TFLOPS == 2500.0


def test_two_pass_gather_decision_logic():
    """bench.two_pass_overlap (N > 1): both modes are timed, one forward of each is compared, and the overlapped mode is headlined only
    when it is faster AND agrees with the serial one within the bound; a disagreement or a non-finite output falls back to the serial
    gather whatever the timing says.  Pure host logic: fake forwards on the CPU."""
    import torch
    b = _bench()

    def run(ms0, ms1, delta, nan=False):
        state = {"mode": None, "set": []}
        base = {"pts3d": torch.arange(12.0).reshape(1, 1, 2, 2, 3) + 1, "depth": torch.ones(1, 1, 2, 2, 1), "camera_params": torch.ones(1, 1, 9)}

        def set_overlap(v):
            state["mode"] = v
            state["set"].append(v)

        def fwd():
            o = {k: v.clone() for k, v in base.items()}
            if state["mode"] == 1:
                o["pts3d"] = o["pts3d"] * (1.0 + delta)
                if nan:
                    o["depth"][0, 0, 0, 0, 0] = float("nan")
            return o
        pick, ms, info = b.two_pass_overlap(set_overlap, fwd, lambda: (ms0 if state["mode"] == 0 else ms1), lambda x: x)
        assert state["set"][:2] == [0, 1] and state["set"][-1] == pick      # serial first; the tuning is left at the choice
        assert ms == (ms0, ms1)[pick] and info["chosen_comm_overlap"] == pick
        return pick, info

    assert run(10.0, 9.0, 1e-4)[0] == 1                 # faster and within the bound
    assert run(10.0, 11.0, 1e-4)[0] == 0                # slower
    pick, info = run(10.0, 5.0, 1e-2)                   # faster but disagrees: not headlined
    assert pick == 0 and not info["comparison_passed"]
    pick, info = run(10.0, 5.0, 0.0, nan=True)          # non-finite output
    assert pick == 0 and not info["comparison_passed"]


def test_dump_outputs_budget_and_fixed_pixel_sample(tmp_path):
    """bench.dump_outputs (--dump-outputs): every output array is written as float32 .npy; over the byte budget the per-pixel arrays
    keep one and the same seeded pixel sample (so that the files of two builds compare element for element) while the small arrays
    stay whole, the total stays within the budget, and a container reachable under two keys is written once."""
    import numpy as np
    import torch
    b = _bench()
    n, H, W = 2, 20, 30
    n_pix = n * H * W
    g = torch.Generator().manual_seed(5)
    pix = torch.arange(n_pix, dtype=torch.float32)           # each pixel carries its own index in every per-pixel array
    raw = {"means": pix.reshape(1, n_pix, 1).repeat(1, 1, 3), "weights": pix.reshape(1, n_pix)}
    out = {"camera_params": torch.rand(1, n, 9, generator=g), "depth": pix.reshape(1, n, H, W, 1),
           "pts3d": pix.reshape(1, n, H, W, 1).repeat(1, 1, 1, 1, 3).double(), "splats_raw": raw, "splats": raw}
    keep = b.dump_outputs(out, str(tmp_path / "all"), n_pix)             # fits: everything whole
    assert keep == n_pix
    files = sorted(p.name for p in (tmp_path / "all").iterdir())
    assert files == ["camera_params.npy", "depth.npy", "pts3d.npy", "splats_raw.means.npy", "splats_raw.weights.npy"]
    d = np.load(tmp_path / "all" / "depth.npy")
    assert d.dtype == np.float32 and d.shape == (1, n, H, W, 1) and np.array_equal(d.ravel(), pix.numpy())
    assert np.load(tmp_path / "all" / "pts3d.npy").dtype == np.float64
    budget = 16 * 1024
    runs = []
    for r in range(2):
        path = tmp_path / f"s{r}"
        keep = b.dump_outputs(out, str(path), n_pix, budget=budget)
        assert 0 < keep < n_pix
        assert sum(p.stat().st_size for p in path.iterdir()) <= budget
        runs.append({p.name: np.load(p) for p in path.iterdir()})
    s = runs[0]
    assert np.array_equal(s["camera_params.npy"], out["camera_params"].numpy())
    idx = s["depth.npy"][:, 0]
    assert idx.shape == (keep,) and np.all(np.diff(idx) > 0)            # pixel order, no repeats
    assert np.array_equal(s["pts3d.npy"], np.repeat(idx[:, None], 3, 1))
    assert np.array_equal(s["splats_raw.means.npy"][:, 0], idx) and np.array_equal(s["splats_raw.weights.npy"], idx)
    assert all(np.array_equal(s[k], runs[1][k]) for k in s)             # the same sample on every run


def test_parallel_weight_draw_is_the_serial_one_bit_for_bit():
    """bench.synthetic_state_dict draws the synthetic weights on several threads; the benchmark's inputs must stay what
    WorldMirror.init_synthetic_weights() uploads: the same names in the same order, every tensor bit-identical."""
    import numpy as np
    from hunyuanworld_mirror_amd import WMConfig
    from hunyuanworld_mirror_amd.weights import iter_params
    b = _bench()
    cfg = WMConfig.tiny(enable_gs=True)
    got = b.synthetic_state_dict(cfg, 4)
    ref = dict(iter_params(cfg))
    assert list(got) == list(ref)
    for k, v in ref.items():
        assert got[k].dtype == np.float32 and got[k].shape == v.shape and got[k].tobytes() == v.tobytes(), k


def test_full_option_exists_and_is_off_by_default():
    """Everything beyond the headline (roofline step, north-star / parity legs, CPU baseline) sits behind --full: the option is in the
    command line, and the options that drop single legs of a --full run are still accepted."""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    for opt in ("--full", "--gpus", "--steps", "--warmup", "--dump-outputs", "--no-cpu-baseline", "--no-north-star", "--no-parity"):
        assert opt in r.stdout, opt
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert re.search(r'add_argument\("--full", action="store_true"', src)
