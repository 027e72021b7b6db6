"""MCMC relocation, growth and position noise on the GPU (wm_mcmc_* through hunyuanworld_mirror_amd.strategy_mcmc) against
tests/mcmc_helper.py and the reference's own results in tests/golden/mcmc_*.npz, and MCMCStrategy in a short optimisation loop.
The criterion for computed values, with e32 the fp32 restatement's relative L2 error against fp64 and e64 the GPU's:
e32 > 0 and e64 <= 4 e32.  Indices, ratios, copied rows and zeroed moments are compared exactly."""
import numpy as np
import pytest
import torch

import mcmc_helper as MH
from conftest import rel_l2
from mcmc_helper import KEYS, SCENES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64


def _criterion(what, h32, gpu, want):
    e32, e64 = rel_l2(h32.double().numpy(), want.numpy()), rel_l2(gpu.double().cpu().numpy(), want.numpy())
    print(f"{what}: e32 {e32:.3e} e64 {e64:.3e}")
    assert e32 > 0 and e64 <= 4 * e32, (what, e32, e64)     # e32 = 0: a seed at which the fp32 restatement is exact, change the seed


def _random_splats(N, seed):
    """opacities log-uniform from 10^-3.5 to 10^-0.5: the gate of the noise is open for some and the dead test splits them"""
    g = torch.Generator().manual_seed(seed)
    u = lambda *s: torch.rand(*s, generator=g)
    return {"means": torch.randn(N, 3, generator=g), "quats": torch.randn(N, 4, generator=g), "scales": torch.log(10 ** (-2.2 + 1.4 * u(N, 3))),
            "opacities": torch.logit(10 ** (-3.5 + 3.0 * u(N))), "noise": torch.randn(N, 3, generator=g)}


@pytest.mark.parametrize("N", [1, 257, 1500])
def test_gpu_inject_noise(N):
    from hunyuanworld_mirror_amd import strategy_mcmc as S
    t, scaler = _random_splats(N, 40 + N), 80.0                       # the trainer's lr * noise_lr = 1.6e-4 * 5e5
    g = {k: v.to(DEV) for k, v in t.items()}
    want = MH.noise_displacement(t["quats"], t["scales"], t["opacities"], t["noise"], scaler, F64)
    h32 = MH.noise_displacement(t["quats"], t["scales"], t["opacities"], t["noise"], scaler, F32)
    assert float(want.abs().max()) > 1e-6                             # the gate is open somewhere
    # from zero means the result IS the displacement (from the real means, the addition would round it at the means' size)
    zero = torch.zeros(N, 3, device=DEV)
    S.mcmc_inject_noise(zero, g["quats"], g["scales"], g["opacities"], g["noise"], scaler)
    _criterion(f"noise displacement N {N}", h32, zero, want)
    before = g["means"].clone()
    S.inject_noise_to_position({k: g[k] for k in ("means", "quats", "scales", "opacities")}, {}, {}, scaler, noise=g["noise"])
    assert torch.equal(g["means"], before + zero)                     # in place, one fp32 addition
    for k in ("quats", "scales", "opacities", "noise"):
        assert torch.equal(g[k].cpu(), t[k]), k                       # read only


@pytest.mark.parametrize("N", [1, 257, 1500])
def test_gpu_partition(N):
    from hunyuanworld_mirror_amd import strategy_mcmc as S
    op = _random_splats(N, 50 + N)["opacities"]
    assert MH.margins(op.double(), 0.005) > 1e-4
    dead, alive = MH.dead_alive(op.double(), 0.005)
    gd, ga = S.mcmc_partition(op.to(DEV), 0.005)
    assert gd.dtype == torch.int32 and torch.equal(gd.cpu().long(), dead) and torch.equal(ga.cpu().long(), alive)
    assert N == 1 or (len(dead) > 0 and len(alive) > 0)
    mask = torch.rand(N, generator=torch.Generator().manual_seed(N)) < 0.3
    gd, ga = S.mcmc_partition(op.to(DEV), 0.005, mask.to(DEV))
    assert torch.equal(gd.cpu().long(), mask.nonzero()[:, 0]) and torch.equal(ga.cpu().long(), (~mask).nonzero()[:, 0])


def _gpu_objects(z, prefix="in_"):
    """parameters and Adam optimisers on the GPU, with the fixture's moments and step = 1"""
    params = torch.nn.ParameterDict({k: torch.nn.Parameter(torch.from_numpy(z[prefix + k]).to(DEV)) for k in KEYS})
    opts = {}
    for k in KEYS:
        opts[k] = torch.optim.Adam([params[k]], lr=1e-3)
        opts[k].state[params[k]] = {"step": torch.tensor(1.0), "exp_avg": torch.from_numpy(z["in_m_" + k]).to(DEV),
                                    "exp_avg_sq": torch.from_numpy(z["in_v_" + k]).to(DEV)}
    return params, opts


def _check_objects(params, opts, n):
    for k in params:
        assert len(params[k]) == n and isinstance(params[k], torch.nn.Parameter) and params[k].requires_grad
        assert opts[k].param_groups[0]["params"][0] is params[k] and list(opts[k].state.keys()) == [params[k]]
        st = opts[k].state[params[k]]
        assert st["exp_avg"].shape == params[k].shape == st["exp_avg_sq"].shape and float(st["step"]) == 1.0


def _compare_stage(name, stage, params, opts, z, prefix, h32, computed_rows):
    for k in KEYS:
        want, got = torch.from_numpy(z[prefix + k]), params[k].detach().cpu()
        assert got.shape == want.shape, k
        comp = torch.zeros(len(want), dtype=torch.bool)
        if k in ("opacities", "scales"):
            comp[computed_rows] = True
        if k != "means" or stage == "relocate":                       # the final means carry the noise: compared apart
            assert torch.equal(got[~comp].double(), want[~comp]), (stage, k)    # copied rows: exact
        if comp.any():
            _criterion(f"{name} {stage} {k}", h32[k][comp], got[comp], want[comp])
        for key, mk in (("exp_avg", "m_"), ("exp_avg_sq", "v_")):
            assert torch.equal(opts[k].state[params[k]][key].cpu().double(), torch.from_numpy(z[prefix + mk + k])), (stage, k, key)


@pytest.mark.parametrize("name", SCENES)
def test_gpu_step_matches_the_reference(name):
    """relocate -> sample_add -> inject_noise_to_position with the reference's draws, against the reference's fp64 results."""
    from hunyuanworld_mirror_amd import strategy_mcmc as S
    z = MH.load_scene(name)
    MH.check_scene_properties(name, z)
    N, mo = int(z["N"]), float(z["min_opacity"])
    dead, alive, s_rel, s_add, c_rel, c_add = MH.scene_facts(z)
    p32, m32, v32 = MH.tensors(z, "in_"), MH.tensors(z, "in_m_"), MH.tensors(z, "in_v_")
    params, opts = _gpu_objects(z)
    # the entries on their own: index lists and ratios exact
    gd, ga = S.mcmc_partition(params["opacities"], mo)
    assert torch.equal(gd.cpu().long(), dead) and torch.equal(ga.cpu().long(), alive)
    _, _, hist = S.mcmc_relocation(params["opacities"], params["scales"], s_rel.to(DEV).int(), mo, return_counts=True)
    assert torch.equal(hist.cpu().long(), torch.bincount(s_rel, minlength=N))
    assert torch.equal((hist.cpu().long()[s_rel] + 1).clamp(1, 51), MH.ratios_of(s_rel))
    # relocation
    storage = {k: params[k].data_ptr() for k in KEYS}
    assert S.relocate(params, opts, {}, None, mo, sampled_idxs=s_rel.to(DEV)) == len(dead)
    torch.cuda.synchronize()
    _check_objects(params, opts, N)
    assert all(params[k].data_ptr() == storage[k] for k in KEYS)                       # the same storage
    h1 = MH.relocate(p32, m32, v32, s_rel, mo, F32)
    touched = torch.cat([s_rel, dead]).unique()
    _compare_stage(name, "relocate", params, opts, z, "rel_", h1[0], touched)
    for k in KEYS:
        m = opts[k].state[params[k]]["exp_avg"].cpu()
        assert float(m[s_rel].abs().max()) == 0.0 and torch.equal(m[dead], m32[k][dead])  # sources zeroed, dead rows as they were
    # growth
    assert S.sample_add(params, opts, {}, len(s_add), mo, sampled_idxs=s_add.to(DEV)) == len(s_add)
    torch.cuda.synchronize()
    n = N + len(s_add)
    _check_objects(params, opts, n)
    h2 = MH.sample_add(*h1, s_add, mo, F32)
    touched = torch.cat([touched, s_add, N + torch.arange(len(s_add))]).unique()       # the relocation's values are fp32 roundings too
    _compare_stage(name, "add", params, opts, z, "out_", h2[0], touched)
    means = params["means"].detach().cpu()
    assert torch.equal(means[:N].double(), torch.from_numpy(z["rel_means"])) and torch.equal(means[N:], means[s_add])
    for k in KEYS:
        for key in ("exp_avg", "exp_avg_sq"):
            assert float(opts[k].state[params[k]][key][N:].abs().max()) == 0.0          # new rows' moments: exactly zero
    # position noise: the displacement, from zero means (the golden's: its final means minus the fp64 means before the noise)
    p64 = MH.sample_add(*MH.relocate(MH.tensors(z, "in_", F64), m32, v32, s_rel, mo, F64), s_add, mo, F64)[0]
    want_d = torch.from_numpy(z["out_means"]) - p64["means"]
    noise, scaler = torch.from_numpy(z["noise"]), float(z["lr"]) * float(z["noise_lr"])
    h32_d = MH.noise_displacement(h2[0]["quats"], h2[0]["scales"], h2[0]["opacities"], noise, scaler, F32)
    zero = torch.zeros(n, 3, device=DEV)
    S.mcmc_inject_noise(zero, params["quats"].detach(), params["scales"].detach(), params["opacities"].detach(), noise.to(DEV), scaler)
    _criterion(f"{name} noise displacement", h32_d, zero, want_d)
    before = params["means"].detach().clone()
    S.inject_noise_to_position(params, opts, {}, scaler, noise=noise.to(DEV))
    assert torch.equal(params["means"].detach(), before + zero)


def _small(opac, seed=0):
    N = len(opac)
    g = torch.Generator().manual_seed(seed)
    p = {"means": torch.randn(N, 3, generator=g), "scales": torch.log(0.02 + 0.1 * torch.rand(N, 3, generator=g)), "quats": torch.randn(N, 4, generator=g),
         "opacities": torch.logit(torch.tensor(opac))}
    params = {k: torch.nn.Parameter(t.float().contiguous().to(DEV)) for k, t in p.items()}
    opts = {k: torch.optim.Adam([params[k]], lr=1e-3) for k in params}
    for k in params:
        opts[k].state[params[k]] = {"step": torch.tensor(3.0), "exp_avg": torch.ones_like(params[k]), "exp_avg_sq": torch.ones_like(params[k])}
    return {k: t.float() for k, t in p.items()}, params, opts


def _one_ulp(got, want):
    """an fp64 evaluation rounded once is within half an ulp of fp32; one ulp leaves room for the fp64 functions' own error"""
    return bool(((got.double().cpu() - want).abs() <= 2.0 ** -23 * want.abs()).all())


def test_gpu_edge_cases():
    import hunyuanworld_mirror_amd as wm
    from hunyuanworld_mirror_amd import strategy_mcmc as S
    ones = lambda p: {k: torch.ones_like(t) for k, t in p.items()}
    strat = wm.MCMCStrategy()
    # no dead Gaussian: every object untouched
    p, params, opts = _small([0.5, 0.1, 0.3, 0.2, 0.9])
    before, values = dict(params), {k: t.detach().clone() for k, t in params.items()}
    assert strat._relocate_gs(params, opts) == 0
    assert all(params[k] is before[k] and torch.equal(params[k], values[k]) and opts[k].param_groups[0]["params"][0] is before[k] for k in params)
    # N < 20: int(1.05 N) == N, and cap_max == N: no growth, every object untouched
    assert strat._add_new_gs(params, opts) == 0
    p20, params20, opts20 = _small([0.5] * 40)
    before20 = dict(params20)
    assert wm.MCMCStrategy(cap_max=40)._add_new_gs(params20, opts20) == 0 and wm.MCMCStrategy(cap_max=30)._add_new_gs(params20, opts20) == 0
    assert all(params[k] is before[k] for k in params) and all(params20[k] is before20[k] for k in params20)
    assert wm.MCMCStrategy(cap_max=41)._add_new_gs(params20, opts20) == 1 and len(params20["means"]) == 41 == len(opts20["means"].state[params20["means"]]["exp_avg"])
    # one alive, all others dead: all become the one (ratio 6)
    p, params, opts = _small([1e-3, 2e-3, 0.7, 1e-4, 3e-3, 4e-3])
    assert strat._relocate_gs(params, opts, torch.Generator(device=DEV).manual_seed(0)) == 5
    sampled = torch.full((5,), 2)
    want, wm_, _ = MH.relocate(p, ones(p), ones(p), sampled, 0.005, F64)
    for k in params:
        assert torch.equal(params[k].detach()[[0, 1, 3, 4, 5]], params[k].detach()[[2] * 5]), k
        assert _one_ulp(params[k].detach(), want[k]), k
        assert torch.equal(opts[k].state[params[k]]["exp_avg"].cpu().double(), wm_[k]) and float(opts[k].state[params[k]]["step"]) == 3.0
        assert opts[k].param_groups[0]["params"][0] is params[k]
    # all dead
    p, params, opts = _small([1e-3, 2e-3, 1e-4])
    with pytest.raises(RuntimeError, match="all 3 Gaussians are dead"):
        strat._relocate_gs(params, opts)
    # a dead source, a wrong length, an index out of range
    p, params, opts = _small([1e-3, 0.5, 0.4, 0.3])
    for bad in ([0], [1, 2], [7]):
        with pytest.raises(ValueError):
            S.relocate(params, opts, {}, None, sampled_idxs=torch.tensor(bad))
    # repeated entries in sampled_idxs: growth
    p, params, opts = _small([0.6, 0.2, 0.5, 0.05])
    sampled = torch.tensor([2, 2, 0, 2])
    state = {"seen": torch.ones(4, device=DEV)}
    assert S.sample_add(params, opts, state, 4, sampled_idxs=sampled) == 4
    want, wm_, _ = MH.sample_add(p, ones(p), ones(p), sampled, 0.005, F64)
    for k in params:
        assert params[k].shape == want[k].shape and _one_ulp(params[k].detach(), want[k]), k
        assert torch.equal(opts[k].state[params[k]]["exp_avg"].cpu().double(), wm_[k])
    assert state["seen"].tolist() == [1.0] * 4 + [0.0] * 4
    assert torch.equal(params["opacities"].detach()[[4, 5, 7]], params["opacities"].detach()[[2, 2, 2]])
    # a caller's mask in place of the opacity test
    p, params, opts = _small([0.6, 0.2, 0.5, 0.05])
    assert S.relocate(params, opts, {}, torch.tensor([False, True, False, False], device=DEV), sampled_idxs=torch.tensor([3])) == 1
    assert torch.equal(params["means"].detach()[1], params["means"].detach()[3])


def _opt_scene():
    """the 150-Gaussian, 2-view, 64 x 48 scene of tests/test_densify_gpu.py's loop test"""
    g = torch.Generator().manual_seed(21)
    N, W, H = 150, 64, 48
    u = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    means = torch.cat([(u(N, 2) - 0.5) * torch.tensor([2.4, 1.8]), 2.0 + 1.5 * u(N, 1)], 1)
    quats = torch.randn(N, 4, generator=g, dtype=torch.float64)
    scales = torch.exp(-2.6 + 1.2 * u(N, 3))
    opac = 0.2 + 0.6 * u(N)
    colors = u(N, 3)
    vm = torch.eye(4, dtype=torch.float64).repeat(2, 1, 1)
    vm[1, :3, :3] = torch.tensor([[np.cos(0.15), 0, np.sin(0.15)], [0, 1, 0], [-np.sin(0.15), 0, np.cos(0.15)]])
    vm[1, :3, 3] = torch.tensor([0.2, -0.05, 0.1])
    K = torch.tensor([[50.0, 0, W / 2], [0, 50.0, H / 2], [0, 0, 1]], dtype=torch.float64).repeat(2, 1, 1)
    true = dict(means=means, quats=quats, scales=scales, opacities=opac, colors=colors)
    start = dict(means=means + 0.03 * torch.randn(N, 3, generator=g, dtype=torch.float64), quats=quats + 0.05 * torch.randn(N, 4, generator=g, dtype=torch.float64),
                 scales=scales * torch.exp(0.1 * torch.randn(N, 3, generator=g, dtype=torch.float64)), opacities=(opac + 0.1 * (u(N) - 0.5)).clamp(0.05, 0.95),
                 colors=(colors + 0.1 * (u(N, 3) - 0.5)).clamp(0, 1))
    return true, start, vm, K, W, H


# The loop test's learning rate and noise_lr.  lr = 2e-2 is the Adam rate at which test_densify_gpu.py's loop recovers within the ten
# steps between refinements on this scene (its LOOP comment); it is also what step_post_backward receives as the rate of the means.
# The trainer's product lr * noise_lr is 1.6e-4 * 5e5 = 80; noise_lr = 4e3 gives the same 80 at lr = 2e-2, so a Gaussian of a given
# opacity is shaken here as it is there.  (With the default 5e5 the product is 1e4: a source halved by eq. 9 to opacity 0.1 has a gate of
# 4.5e-5 and would move by 0.45 times its covariance every step.)
LOOP = dict(lr=2e-2, noise_lr=4e3)


def test_gpu_strategy_in_the_optimisation_loop():
    """40 steps on the 150-Gaussian scene.  N follows min(cap_max, int(1.05 N)) at steps 10 / 20 / 30 and not after refine_stop_iter;
    parameters, gradients and optimiser states agree in length after every step, "step" survives and the param group holds the live
    Parameter; the loss stays finite and ends below its start."""
    import hunyuanworld_mirror_amd as wm
    true, start, vm, K, W, H = _opt_scene()
    c2w, Kg = torch.linalg.inv(vm).float().to(DEV), K.float().to(DEV)
    rz = wm.Rasterizer()
    with torch.no_grad():
        f = lambda d, k: d[k].float().to(DEV)
        target = rz.rasterize_splats(f(true, "means"), f(true, "quats"), f(true, "scales"), f(true, "opacities"), f(true, "colors"), c2w, Kg, W, H)[0]
    sh0 = ((start["colors"] - 0.5) / 0.28209479177387814).float()[:, None, :]
    params = torch.nn.ParameterDict({"means": start["means"].float(), "scales": torch.log(start["scales"]).float(), "quats": start["quats"].float(),
                                     "opacities": torch.logit(start["opacities"]).float(), "sh0": sh0}).to(DEV)
    opts = {k: torch.optim.Adam([params[k]], lr=LOOP["lr"]) for k in params}
    strat = wm.MCMCStrategy(refine_start_iter=0, refine_every=10, refine_stop_iter=31, cap_max=170, noise_lr=LOOP["noise_lr"])
    strat.check_sanity(params, opts)
    state = strat.initialize_state()
    gen = torch.Generator(device=DEV).manual_seed(1)
    sizes, losses, expect = [], [], 150
    for step in range(40):
        rgb, _, _, info = rz.rasterize_splats(params["means"], params["quats"], torch.exp(params["scales"]), torch.sigmoid(params["opacities"]),
                                              params["sh0"], c2w, Kg, W, H, sh_degree=0, return_info=True)
        loss = wm.photometric_loss(rgb, target, 0.2, "valid")[0]
        for o in opts.values():
            o.zero_grad()
        loss.backward()                                         # at steps 11 / 21 / 31: into the Parameters the refinement created
        for k in params:
            assert params[k].grad is not None and params[k].grad.shape == params[k].shape, (step, k)
        for o in opts.values():
            o.step()
        strat.step_post_backward(params, opts, state, step, info, lr=LOOP["lr"], generator=gen)
        if step in (10, 20, 30):
            expect = min(170, int(1.05 * expect))
        n = len(params["means"])
        assert n == expect, (step, n, expect)
        sizes.append(n)
        losses.append(float(loss.detach()))
        for k in params:
            assert params[k].grad is None or params[k].grad.shape == params[k].shape, (step, k)
            assert len(params[k]) == n and isinstance(params[k], torch.nn.Parameter) and params[k].requires_grad
            assert opts[k].param_groups[0]["params"][0] is params[k] and list(opts[k].state.keys()) == [params[k]]
            st = opts[k].state[params[k]]
            assert st["exp_avg"].shape == params[k].shape == st["exp_avg_sq"].shape and float(st["step"]) == step + 1
    print("N per step", sizes, "loss", [f"{x:.4f}" for x in losses])
    assert sizes[9:11] == [150, 157] and sizes[19:21] == [157, 164] and sizes[29:31] == [164, 170] and sizes[-1] == 170
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
