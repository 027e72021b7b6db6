"""CPU: tests/mcmc_helper.py (the torch restatement the GPU tests compare with) reproduces the REFERENCE's MCMCStrategy step on the
fixtures tests/golden/mcmc_*.npz (tools/gen_golden_mcmc.py: gsplat's own code, CPU, fp64; eq. 9 itself is the helper's literal form
there), eq. 9's closed forms and its collapsed form hold, and the new C ABI names are declared, bound and exported."""
import ctypes as C
import math
import os

import pytest
import torch

import mcmc_helper as MH
from conftest import ROOT

KEYS, SCENES = MH.KEYS, MH.SCENES
F64 = torch.float64


def relmax(a, b):
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("name", SCENES)
def test_golden_scene_properties(name):
    MH.check_scene_properties(name, MH.load_scene(name))


def _compare(got, want, computed_rows, key):
    """copied rows exact; computed rows (opacities and scales of sources and copies) within 1e-12"""
    assert got.shape == want.shape, key
    comp = torch.zeros(len(want), dtype=torch.bool)
    if key in ("opacities", "scales"):
        comp[computed_rows] = True
    assert torch.equal(got[~comp], want[~comp]), key
    if comp.any():
        assert relmax(got[comp], want[comp]) < 1e-12, key


@pytest.mark.parametrize("name", SCENES)
def test_helper_reproduces_the_reference(name):
    z = MH.load_scene(name)
    N, mo = int(z["N"]), float(z["min_opacity"])
    dead, alive, s_rel, s_add, c_rel, c_add = MH.scene_facts(z)
    p, m, v = MH.tensors(z, "in_", F64), MH.tensors(z, "in_m_", F64), MH.tensors(z, "in_v_", F64)
    assert torch.equal(MH.ratios_of(s_rel), (c_rel + 1).clamp(max=51))
    # relocation
    p1, m1, v1 = MH.relocate(p, m, v, s_rel, mo, F64)
    touched = torch.cat([s_rel, dead]).unique()
    for k in KEYS:
        _compare(p1[k], torch.from_numpy(z["rel_" + k]), touched, k)
        assert torch.equal(m1[k], torch.from_numpy(z["rel_m_" + k])) and torch.equal(v1[k], torch.from_numpy(z["rel_v_" + k])), k
        assert float(m1[k][s_rel].abs().max()) == 0.0 and torch.equal(m1[k][dead], m[k][dead])        # sources zeroed, dead rows kept
    assert float(torch.sigmoid(p1["opacities"]).min()) >= mo * (1 - 1e-12)
    # growth
    p2, m2, v2 = MH.sample_add(p1, m1, v1, s_add, mo, F64)
    touched = torch.cat([s_add, N + torch.arange(len(s_add))]).unique()
    want_means = torch.from_numpy(z["out_means"])
    for k in KEYS:
        if k != "means":
            _compare(p2[k], torch.from_numpy(z["out_" + k]), touched, k)
        assert torch.equal(m2[k], torch.from_numpy(z["out_m_" + k])) and torch.equal(v2[k], torch.from_numpy(z["out_v_" + k])), k
        assert float(m2[k][N:].abs().max()) == 0.0 and float(v2[k][N:].abs().max()) == 0.0
    assert len(p2["means"]) == min(int(z["cap_max"]), int(1.05 * N)) == len(want_means)
    # position noise: compare what is added (the means themselves are orders larger)
    d = MH.noise_displacement(p2["quats"], p2["scales"], p2["opacities"], torch.from_numpy(z["noise"]), float(z["lr"]) * float(z["noise_lr"]), F64)
    want_d = want_means - p2["means"]
    assert float(d.abs().max()) > 1e-6                       # the gate is not vanishing everywhere
    assert float((d - want_d).abs().max()) < 1e-12 * float(want_means.abs().max())      # the subtraction above rounds at the means' size
    assert relmax(p2["means"] + d, want_means) < 1e-12


def test_eq9_closed_forms():
    g = torch.Generator().manual_seed(3)
    o = 10 ** (-3.5 + 3.49 * torch.rand(200, generator=g, dtype=F64))
    s = torch.rand(200, 3, generator=g, dtype=F64) + 0.1
    for form in (MH.relocation_literal, MH.relocation_collapsed):
        x, ns = form(o, s, torch.ones(200, dtype=torch.int64), F64)                      # ratio 1: nothing changes
        assert relmax(x, o) < 1e-12 and relmax(ns, s) < 1e-12
        x, ns = form(o, s, torch.full((200,), 2), F64)                                   # ratio 2: denom = 2x - x^2 / sqrt(2)
        assert relmax(x, 1 - torch.sqrt(1 - o)) < 1e-12
        assert relmax(ns, (o / (2 * x - x * x / math.sqrt(2)))[:, None] * s) < 1e-12


def test_eq9_hockey_stick_form_equals_the_literal_form():
    g = torch.Generator().manual_seed(4)
    n = 8
    o = torch.cat([10 ** (-3.5 + 3.49 * torch.rand(n - 2, generator=g, dtype=F64)), torch.tensor([0.99, 1 - 1e-6], dtype=F64)])
    s = torch.ones(n, 3, dtype=F64)
    eps = 2.0 ** -52
    worst = 0.0
    for ratio in range(1, MH.N_MAX + 1):
        r = torch.full((n,), ratio)
        (xl, sl), (xc, sc) = MH.relocation_literal(o, s, r, F64), MH.relocation_collapsed(o, s, r, F64)
        assert torch.equal(xl, xc)
        # the alternating sum's condition number: sum of |terms| over |sum|.  Either form rounds each of its terms a few times (a power,
        # a product, a quotient, an addition): 8 eps per term of size <= the largest, 51 terms -> 400 eps times the condition number
        terms = torch.stack([math.comb(ratio, k + 1) / math.sqrt(k + 1) * xc ** (k + 1) for k in range(ratio)])
        cond = terms.sum(0) / (o / sc[:, 0])
        err = (sc - sl).abs().max(-1).values / sl.abs().max(-1).values
        assert bool((err <= 400 * eps * cond).all()), (ratio, err, cond)
        worst = max(worst, float((err / cond).max()))
    print(f"collapsed vs literal, ratios 1..51: worst difference {worst / eps:.1f} eps times the condition number")


NEW_EXPORTS = ["wm_mcmc_inject_noise", "wm_mcmc_partition_workspace_bytes", "wm_mcmc_partition", "wm_mcmc_relocation", "wm_mcmc_scatter",
               "wm_mcmc_zero_rows"]


def test_new_exports_and_strategy_surface():
    from hunyuanworld_mirror_amd import _lib, strategy_mcmc
    import hunyuanworld_mirror_amd as wm
    lib = os.path.join(ROOT, "hunyuanworld-mirror_amd", "libwm_hip.so")
    if not os.path.exists(lib):
        import __graft_entry__ as g
        g.build()
    L = C.CDLL(lib)
    hdr = open(os.path.join(ROOT, "include", "wm_hip.h")).read()
    for n in NEW_EXPORTS:
        assert n in _lib.EXPORTS and hasattr(L, n) and (n + "(") in hdr, n
    L.wm_mcmc_partition_workspace_bytes.restype = C.c_size_t
    L.wm_mcmc_partition_workspace_bytes.argtypes = [C.c_size_t]
    assert L.wm_mcmc_partition_workspace_bytes(1000) >= 2 * 1001 * 4
    assert wm.MCMCStrategy is strategy_mcmc.MCMCStrategy
    s = wm.MCMCStrategy()
    assert (s.cap_max, s.noise_lr, s.refine_start_iter, s.refine_stop_iter, s.refine_every, s.min_opacity, s.verbose) == \
        (1_000_000, 5e5, 500, 25_000, 100, 0.005, False)                                 # gsplat/strategy/mcmc.py:49-55
    assert s.initialize_state() == {}
    for f in ("relocate", "sample_add", "inject_noise_to_position"):
        assert callable(getattr(strategy_mcmc, f))
    with pytest.raises(NotImplementedError):
        strategy_mcmc._multinomial_sample(torch.empty(2 ** 24 + 1, device="meta"), 3, None)
    p = {k: torch.nn.Parameter(torch.zeros(3, 3)) for k in ("means", "scales", "quats")}
    with pytest.raises(AssertionError):
        s.check_sanity(p, {k: torch.optim.Adam([v]) for k, v in p.items()})              # opacities missing
    p["opacities"] = torch.nn.Parameter(torch.zeros(3))
    with pytest.raises(RuntimeError):                                                    # no CPU fallback
        s.step_post_backward(p, {k: torch.optim.Adam([v]) for k, v in p.items()}, {}, 1, {}, lr=1e-3)
