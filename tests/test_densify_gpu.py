"""Splat densification on the GPU (wm_densify_accumulate / wm_densify_plan / wm_densify_gather through
hunyuanworld_mirror_amd.strategy) against tests/densify_helper.py and the reference's own results in tests/golden/densify_*.npz,
and DefaultStrategy in a short optimisation loop."""
import numpy as np
import pytest
import torch

import densify_helper as DH
from conftest import rel_l2
from densify_helper import KEYS, SCENES, helper_state, load_scene

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _accumulate_case(N, C_, W, H, with_radii, seed):
    from hunyuanworld_mirror_amd import strategy as S
    g = torch.Generator().manual_seed(seed)
    grads = torch.randn(2, C_, N, 2, generator=g) * 1e-4
    radii = torch.randint(0, 9, (2, C_, N, 2), generator=g, dtype=torch.int32)       # 0 = culled, in some cameras only
    st = {d: [torch.zeros(N, dtype=d), torch.zeros(N, dtype=d), torch.zeros(N, dtype=d) if with_radii else None] for d in (torch.float32, torch.float64)}
    gpu = [torch.zeros(N, device=DEV), torch.zeros(N, device=DEV), torch.zeros(N, device=DEV) if with_radii else None]
    for i in range(2):                                                               # twice: the running sums
        for d in st:
            st[d] = list(DH.update_state(grads[i], radii[i], W, H, *st[d], d))
        S.densify_accumulate(grads[i].to(DEV), radii[i].to(DEV), W, H, *gpu)
    torch.cuda.synchronize()
    e32 = rel_l2(st[torch.float32][0].double().numpy(), st[torch.float64][0].numpy())
    e64 = rel_l2(gpu[0].double().cpu().numpy(), st[torch.float64][0].numpy())
    print(f"accumulate N {N} C {C_} radii {with_radii}: e32 {e32:.3e} e64 {e64:.3e}")
    assert e32 > 0 and e64 <= 4 * e32, (e32, e64)    # e32 = 0 would mean a seed at which the fp32 restatement is exact: change the seed
    assert torch.equal(gpu[1].cpu().double(), st[torch.float64][1])
    if with_radii:
        assert torch.equal(gpu[2].cpu(), st[torch.float32][2])
        assert rel_l2(gpu[2].double().cpu().numpy(), st[torch.float64][2].numpy()) < 1e-7


@pytest.mark.parametrize("N,C_,with_radii", [(1500, 3, True), (1500, 3, False), (1, 3, True), (257, 2, True)])
def test_gpu_accumulate(N, C_, with_radii):
    _accumulate_case(N, C_, 100, 70, with_radii, seed=N + C_)


def _gpu_refine(p, m, v, g2, cnt, rs, cfg, step, scene, noise):
    """-> plan, new params, new moments (all on the GPU)"""
    from hunyuanworld_mirror_amd import strategy as S
    plan = S.densify_plan(g2, cnt, rs, p["scales"], p["opacities"], grow_grad2d=cfg["grow_grad2d"], grow_scale3d=cfg["grow_scale3d"] * scene,
                          grow_scale2d=cfg["grow_scale2d"], prune_opa=cfg["prune_opa"], prune_scale3d=cfg["prune_scale3d"] * scene,
                          prune_scale2d=cfg["prune_scale2d"], use_scale2d=step < cfg["refine_scale2d_stop_iter"], prune_big=step > cfg["reset_every"],
                          revised_opacity=cfg["revised_opacity"])
    N = plan["n_in"]
    nz = torch.zeros(2, N, 3, device=DEV)
    if noise is not None:
        nz[:, :noise.shape[1]] = noise.to(DEV)
    out, mo, vo = {}, {}, {}
    for k in p:
        out[k] = S.densify_gather(p[k], plan, DH.gather_mode(k, cfg["revised_opacity"]), p["quats"], p["scales"], nz)
        mo[k], vo[k] = S.densify_gather(m[k], plan, "zero_new"), S.densify_gather(v[k], plan, "zero_new")
    torch.cuda.synchronize()
    return plan, out, mo, vo


@pytest.mark.parametrize("name", SCENES)
def test_gpu_refine_matches_the_reference(name):
    from hunyuanworld_mirror_amd import strategy as S
    z, cfg = load_scene(name)
    step, scene, N = int(z["step"]), float(z["scene_scale"]), int(z["N"])
    g2, cnt = torch.zeros(N, device=DEV), torch.zeros(N, device=DEV)
    rs = torch.zeros(N, device=DEV) if "state_radii" in z else None
    for i in range(2):
        S.densify_accumulate(torch.from_numpy(z["grads"][i]).to(DEV), torch.from_numpy(z["radii"][i]).to(DEV), int(z["width"]), int(z["height"]), g2, cnt, rs)
    h64 = helper_state(z, torch.float64)
    p64 = {k: torch.from_numpy(z["in_" + k]).double() for k in KEYS}
    mg = DH.margins(*h64, p64["scales"], p64["opacities"], cfg, step, scene)
    assert min(mg.values()) > 1e-4, mg
    src, kind, rank, counts = DH.plan(*h64, p64["scales"], p64["opacities"], cfg, step, scene)
    p = {k: torch.from_numpy(z["in_" + k]).to(DEV) for k in KEYS}
    m = {k: torch.from_numpy(z["in_m_" + k]).to(DEV) for k in KEYS}
    v = {k: torch.from_numpy(z["in_v_" + k]).to(DEV) for k in KEYS}
    noise = torch.from_numpy(z["noise"])
    plan, out, mo, vo = _gpu_refine(p, m, v, g2, cnt, rs, cfg, step, scene, noise)
    assert [plan["n_dupli"], plan["n_split"], plan["n_prune"], plan["n_out"]] == [int(x) for x in z["counts"]] == list(counts)
    assert torch.equal(plan["src"].cpu().long(), src) and torch.equal(plan["kind"].cpu().long(), kind)
    child = kind >= DH.SPLIT0
    assert torch.equal(plan["rank"].cpu().long()[child], rank[child])
    for k in KEYS:
        mode = DH.gather_mode(k, cfg["revised_opacity"])
        want = torch.from_numpy(z["out_" + k])                                      # the reference's result (fp64)
        got = out[k].cpu()
        assert got.shape == want.shape
        computed = child if mode != "copy" else torch.zeros_like(child)
        assert torch.equal(got[~computed].double(), want[~computed]), k             # copied rows: exact
        if computed.any():
            h32 = DH.gather(torch.from_numpy(z["in_" + k]), src, kind, rank, mode, torch.float32, torch.from_numpy(z["in_quats"]),
                            torch.from_numpy(z["in_scales"]), noise)
            e32 = rel_l2(h32[computed].double().numpy(), want[computed].numpy())
            e64 = rel_l2(got[computed].double().numpy(), want[computed].numpy())
            print(f"{name} {k} ({mode}): e32 {e32:.3e} e64 {e64:.3e}")
            assert e64 <= 4 * e32, (k, e32, e64)
        for gm, key in ((mo, "out_m_"), (vo, "out_v_")):
            assert torch.equal(gm[k].cpu().double(), torch.from_numpy(z[key + k])), (k, key)
            assert float(gm[k][plan["kind"] != 0].abs().max()) == 0.0                # new rows' moments: exactly zero


def _small(N, scales, opac, grad, radii_state=None):
    p = {"means": torch.randn(N, 3), "scales": torch.log(torch.tensor(scales).reshape(N, 1).repeat(1, 3)), "quats": torch.randn(N, 4),
         "opacities": torch.logit(torch.tensor(opac))}
    p = {k: t.float().contiguous().to(DEV) for k, t in p.items()}
    g2, cnt = torch.tensor(grad).float().to(DEV), torch.ones(N, device=DEV)
    rs = None if radii_state is None else torch.tensor(radii_state).float().to(DEV)
    return p, {k: torch.ones_like(t) for k, t in p.items()}, g2, cnt, rs


def test_gpu_refine_edge_cases():
    import hunyuanworld_mirror_amd as wm
    from hunyuanworld_mirror_amd import strategy as S
    cfg = dict(DH.DEFAULTS)
    torch.manual_seed(0)
    # nothing selected: tensors unchanged, nothing reallocated
    p, m, g2, cnt, rs = _small(5, [0.05] * 5, [0.5] * 5, [1e-5] * 5)
    plan, out, mo, _ = _gpu_refine(p, m, m, g2, cnt, rs, cfg, 600, 1.0, None)
    assert (plan["n_dupli"], plan["n_split"], plan["n_prune"], plan["n_out"]) == (0, 0, 0, 5)
    assert plan["src"].tolist() == list(range(5)) and all(torch.equal(out[k], p[k]) and torch.equal(mo[k], m[k]) for k in p)
    params = {k: torch.nn.Parameter(t.clone()) for k, t in p.items()}
    before = dict(params)
    opts = {k: torch.optim.Adam([params[k]], lr=1e-3) for k in params}
    state = {"grad2d": g2.clone(), "count": cnt.clone(), "scene_scale": 1.0}
    assert wm.DefaultStrategy()._refine(params, opts, state, 600) == (0, 0, 0)
    assert all(params[k] is before[k] for k in params) and float(state["grad2d"].abs().max()) == 0.0
    # everything pruned but one
    p, m, g2, cnt, rs = _small(6, [0.05] * 6, [1e-4, 1e-4, 0.7, 1e-4, 1e-4, 1e-4], [1e-5] * 6)
    plan, out, _, _ = _gpu_refine(p, m, m, g2, cnt, rs, cfg, 600, 1.0, None)
    assert (plan["n_prune"], plan["n_out"]) == (5, 1) and plan["src"].tolist() == [2] and torch.equal(out["means"], p["means"][2:3])
    # N = 1: split
    p, m, g2, cnt, rs = _small(1, [0.05], [0.5], [1e-2])
    noise = torch.randn(2, 1, 3)
    plan, out, mo, _ = _gpu_refine(p, m, m, g2, cnt, rs, cfg, 600, 1.0, noise)
    assert (plan["n_dupli"], plan["n_split"], plan["n_prune"], plan["n_out"]) == (0, 1, 0, 2) and plan["kind"].tolist() == [2, 3]
    want = DH.gather(p["means"].cpu(), torch.tensor([0, 0]), torch.tensor([2, 3]), torch.tensor([0, 0]), "means", torch.float64, p["quats"].cpu(),
                     p["scales"].cpu(), noise)
    assert rel_l2(out["means"].double().cpu().numpy(), want.numpy()) < 1e-6 and float(mo["means"].abs().max()) == 0.0
    # N = 1: everything pruned
    p, m, g2, cnt, rs = _small(1, [0.05], [1e-4], [1e-5])
    plan, out, _, _ = _gpu_refine(p, m, m, g2, cnt, rs, cfg, 600, 1.0, None)
    assert plan["n_out"] == 0 and out["means"].shape == (0, 3)
    # small, high gradient, large 2-D radius: duplicated AND split -> the copy, then its two children; its neighbour untouched
    cfg2 = dict(cfg, refine_scale2d_stop_iter=1000)
    p, m, g2, cnt, rs = _small(2, [0.005, 0.005], [0.5, 0.5], [1e-2, 1e-5], [0.1, 0.0])
    plan, out, mo, _ = _gpu_refine(p, m, m, g2, cnt, rs, cfg2, 600, 1.0, torch.randn(2, 1, 3))
    assert (plan["n_dupli"], plan["n_split"], plan["n_prune"], plan["n_out"]) == (1, 1, 0, 4)
    assert plan["src"].tolist() == [1, 0, 0, 0] and plan["kind"].tolist() == [0, 1, 2, 3]
    h = DH.plan(g2.cpu().double(), cnt.cpu().double(), rs.cpu().double(), p["scales"].cpu().double(), p["opacities"].cpu().double(), cfg2, 600, 1.0)
    assert h[0].tolist() == [1, 0, 0, 0] and h[1].tolist() == [0, 1, 2, 3]
    assert torch.equal(out["means"][1], p["means"][0]) and mo["means"][:, 0].tolist() == [1.0, 0.0, 0.0, 0.0]


def _opt_scene():
    """the 150-Gaussian, 2-view, 64 x 48 scene of test_gpu_optimises_like_the_fp64_restatement (tests/test_raster_backward_gpu.py)"""
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


# grow_grad2d and the learning rate of the loop test, per gradient kind.  The scene starts as a near-converged fit (loss 0.03), where
# every split costs loss (children move by a draw of their parent's own extent): the threshold lets a tenth of the splats grow per
# refinement, enough that both kinds occur at every setting nearby, and Adam at 2e-2 recovers within the ten steps between
# refinements (at 2e-3, the rate of the fixed-N tests, the loss is still above its start at step 40).  absgrad sums are larger.
LOOP = {False: dict(grow_grad2d=0.012, lr=2e-2), True: dict(grow_grad2d=0.03, lr=2e-2)}


def _run_loop(absgrad, grow_grad2d, lr, steps=40):
    """rasterize_splats(return_info=True) -> photometric_loss -> step_pre_backward -> backward -> Adam -> step_post_backward, with the
    structural checks after every step.  -> N per step, the refinements' (n_dupli, n_split, n_prune), the losses."""
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
    opts = {k: torch.optim.Adam([params[k]], lr=lr) for k in params}
    strat = wm.DefaultStrategy(refine_start_iter=0, refine_every=10, refine_stop_iter=31, grow_grad2d=grow_grad2d, absgrad=absgrad, verbose=False)
    strat.check_sanity(params, opts)
    state = strat.initialize_state(scene_scale=10.0)          # grow_scale3d * scene_scale = 0.1: the scene's scales (0.074 .. 0.25) straddle it
    gen = torch.Generator(device=DEV).manual_seed(1)
    sizes, losses, refinements = [], [], []
    refine = strat._refine
    strat._refine = lambda *a, **k: (refinements.append(refine(*a, **k)), refinements[-1])[1]
    for step in range(steps):
        rgb, _, _, info = rz.rasterize_splats(params["means"], params["quats"], torch.exp(params["scales"]), torch.sigmoid(params["opacities"]),
                                              params["sh0"], c2w, Kg, W, H, sh_degree=0, return_info=True, absgrad=absgrad)
        loss = wm.photometric_loss(rgb, target, 0.2, "valid")[0]
        strat.step_pre_backward(params, opts, state, step, info)
        for o in opts.values():
            o.zero_grad()
        loss.backward()                                         # at steps 11 / 21 / 31: into the Parameters the refinement created
        for k in params:
            assert params[k].grad is not None and params[k].grad.shape == params[k].shape, (step, k)
        for o in opts.values():
            o.step()
        strat.step_post_backward(params, opts, state, step, info, generator=gen)
        for k in params:
            assert params[k].grad is None or params[k].grad.shape == params[k].shape, (step, k)
        n = len(params["means"])
        sizes.append(n)
        losses.append(float(loss.detach()))
        for k in params:
            assert len(params[k]) == n and isinstance(params[k], torch.nn.Parameter) and params[k].requires_grad
            assert opts[k].param_groups[0]["params"][0] is params[k] and list(opts[k].state.keys()) == [params[k]]
            st = opts[k].state[params[k]]
            assert st["exp_avg"].shape == params[k].shape == st["exp_avg_sq"].shape and float(st["step"]) == step + 1
        assert len(state["grad2d"]) == n == len(state["count"])
    with pytest.raises(NotImplementedError):
        strat.step_post_backward(params, opts, state, 5, info, packed=True)
    return sizes, refinements, losses


@pytest.mark.parametrize("absgrad", [False, True])
def test_gpu_strategy_in_the_optimisation_loop(absgrad):
    """40 steps on the 150-Gaussian scene.  N changes at steps 10 / 20 / 30 and not after refine_stop_iter; parameters, gradients and
    optimiser states agree in length after every step and "step" survives (checked in _run_loop); both growth kinds occur; the
    loss stays finite and ends below its start."""
    sizes, refinements, losses = _run_loop(absgrad, **LOOP[absgrad])
    print("N per step", sizes, "refinements (n_dupli, n_split, n_prune)", refinements, "loss", [f"{x:.4f}" for x in losses])
    changes = [i for i in range(1, 40) if sizes[i] != sizes[i - 1]] + ([0] if sizes[0] != 150 else [])
    assert changes == [10, 20, 30], changes
    assert len(refinements) == 3 and sum(r[0] for r in refinements) > 0 and sum(r[1] for r in refinements) > 0      # both growth kinds
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
