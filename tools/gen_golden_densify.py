"""Writes tests/golden/densify_*.npz: inputs and the results of the REFERENCE's gsplat.strategy.DefaultStrategy on them (CPU, fp64),
and tests/golden/absgrad_24g_2c_33x18.npz: a small scene with its per-pixel absgrad reference.  Data only.

    python tools/gen_golden_densify.py <path to the reference's gsplat checkout (the directory that holds the gsplat package)>

Scenes (N <= 600): inputs are fp32 values; the reference runs on their fp64 casts, so its results are the exact-arithmetic answer
to the inputs a fp32 implementation receives.  The Adam moments come from one real fp32 optimiser step.  Two step_post_backward calls
per scene (the second one refines), so the running sums are exercised.  The split noise is the one random draw of a refinement:
torch.randn(2, n_split, 3) after re-seeding; it is drawn in fp32 (torch.randn is wrapped for the call) and recorded.
The reference runs with float64 as the default dtype (its state and new moments take it); the one dtype it spells out, the count
increments of default.py:252, follows (torch.ones_like is wrapped for the call).
The radii grow from camera to camera wherever a Gaussian is seen twice: the reference's indexed assignment
(default.py:256-260, "should be ideally using scatter max") keeps the LAST camera's value, the kernels keep the maximum.
Asserted here and again in the tests: n_dupli, n_split, n_prune and the survivors of each kind are > 0, and no compared quantity lies
within relative 1e-4 of a threshold (fp32 rounding cannot flip a decision).  If a scene violates that, change its seed."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import densify_helper as DH  # noqa: E402
import raster_grad_helper as RG  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
KEYS = ("means", "scales", "quats", "opacities", "sh0", "shN")

SCENES = {
    # every clause fires: revised opacity, screen-size clauses (step < refine_scale2d_stop_iter), too-big pruning (step > reset_every)
    "densify_a_500g_3c": dict(seed=11, N=500, C=3, W=97, H=70, step=120, scene_scale=1.5,
                              cfg=dict(revised_opacity=True, refine_scale2d_stop_iter=1000, reset_every=50, refine_every=20, refine_start_iter=10,
                                       grow_grad2d=0.0004)),
    "densify_b_600g_2c": dict(seed=12, N=600, C=2, W=80, H=56, step=600, scene_scale=1.0, cfg=dict()),
}


def make_inputs(sc):
    g = torch.Generator().manual_seed(sc["seed"])
    N, C, W, H = sc["N"], sc["C"], sc["W"], sc["H"]
    u = lambda *s: torch.rand(*s, generator=g)
    p = {"means": torch.randn(N, 3, generator=g), "scales": torch.log(10 ** (-3.2 + 2.6 * u(N, 3))), "quats": torch.randn(N, 4, generator=g),
         "opacities": torch.logit(10 ** (-3.5 + 3.45 * u(N))), "sh0": u(N, 1, 3), "shN": torch.randn(N, 3, 3, generator=g) * 0.1}
    grads = torch.randn(2, C, N, 2, generator=g) * (10 ** (-6.5 + 2.5 * u(1, 1, N, 1)))
    base = torch.randint(1, 5, (2, 1, N, 2), generator=g)
    radii = (base * (1 + torch.arange(C).reshape(1, C, 1, 1))).to(torch.int32)      # grows from camera to camera
    radii[1] = radii[1] + radii[0].max(dim=0, keepdim=True).values                  # and from the first step to the second
    seen = u(2, C, N) > 0.3
    radii = radii * seen[..., None].to(torch.int32)
    radii[:, :, : N // 10, :] = 0                                                   # some never seen at all
    radii[0, 0, N // 10: N // 5, 1] = 0                                             # one radius 0 = culled
    return p, grads, radii


def adam_moments(p, seed):
    g = torch.Generator().manual_seed(seed + 100)
    out, m, v = {}, {}, {}
    for k, t in p.items():
        q = torch.nn.Parameter(t.clone())
        opt = torch.optim.Adam([q], lr=1e-3)
        q.grad = torch.randn(t.shape, generator=g) * 0.01
        opt.step()
        out[k], m[k], v[k] = q.detach().clone(), opt.state[q]["exp_avg"].clone(), opt.state[q]["exp_avg_sq"].clone()
    return out, m, v


def run_reference(DefaultStrategy, sc, p, m, v, grads, radii):
    cfg = sc["cfg"]
    strat = DefaultStrategy(verbose=False, **cfg)
    params = torch.nn.ParameterDict({k: torch.nn.Parameter(t.double()) for k, t in p.items()})
    opts = {}
    for k in params:
        opts[k] = torch.optim.Adam([params[k]], lr=1e-3)
        opts[k].state[params[k]] = {"step": torch.tensor(1.0), "exp_avg": m[k].double(), "exp_avg_sq": v[k].double()}
    strat.check_sanity(params, opts)
    state = strat.initialize_state(scene_scale=sc["scene_scale"])
    state_only = strat.initialize_state(scene_scale=sc["scene_scale"])
    noise = []
    real_randn = torch.randn

    def randn32(*size, **kw):
        kw.pop("dtype", None)
        z = real_randn(*size, dtype=torch.float32, **kw)
        noise.append(z.clone())
        return z.double()

    real_ones_like = torch.ones_like

    def ones_like64(t, **kw):      # default.py:252 spells the count increments' dtype out as float32: follow the state's dtype instead
        if kw.get("dtype") == torch.float32:
            kw["dtype"] = torch.float64
        return real_ones_like(t, **kw)

    for i, step in enumerate((sc["step"] - 1, sc["step"])):
        m2 = torch.zeros(sc["C"], sc["N"], 2, dtype=torch.float64, requires_grad=True)
        m2.grad = grads[i].double()
        info = dict(means2d=m2, radii=radii[i], width=sc["W"], height=sc["H"], n_cameras=sc["C"], gaussian_ids=None)
        torch.manual_seed(sc["seed"])
        torch.ones_like = ones_like64
        torch.randn = randn32
        try:
            strat._update_state(params, state_only, info)
            strat.step_post_backward(params, opts, state, step, info)
        finally:
            torch.randn, torch.ones_like = real_randn, real_ones_like
    assert len(noise) == 1 and noise[0].shape[0] == 2, "the split noise is the only random draw"
    out = {k: params[k].detach() for k in params}
    mo = {k: opts[k].state[params[k]]["exp_avg"] for k in params}
    vo = {k: opts[k].state[params[k]]["exp_avg_sq"] for k in params}
    steps = {k: float(opts[k].state[params[k]]["step"]) for k in params}
    assert all(s == 1.0 for s in steps.values())
    return out, mo, vo, noise[0], state_only


def gen_scene(DefaultStrategy, name, sc):
    p0, grads, radii = make_inputs(sc)
    p, m, v = adam_moments(p0, sc["seed"])
    torch.set_default_dtype(torch.float64)      # the reference allocates its state and the new moments in the default dtype
    try:
        out, mo, vo, noise, st = run_reference(DefaultStrategy, sc, p, m, v, grads, radii)
    finally:
        torch.set_default_dtype(torch.float32)
    cfg = dict(DH.DEFAULTS, **sc["cfg"])
    mg = DH.margins(st["grad2d"], st["count"], st.get("radii"), p["scales"].double(), p["opacities"].double(), cfg, sc["step"], sc["scene_scale"])
    print(name, "margins", {k: f"{x:.2e}" for k, x in mg.items()})
    assert min(mg.values()) > 1e-4, mg
    src, kind, rank, counts = DH.plan(st["grad2d"], st["count"], st.get("radii"), p["scales"].double(), p["opacities"].double(), cfg, sc["step"],
                                      sc["scene_scale"])
    n_dupli, n_split, n_prune, n_out = counts
    assert noise.shape[1] == n_split and out["means"].shape[0] == n_out, (noise.shape, counts, out["means"].shape)
    survivors = [int((kind == k).sum()) for k in range(4)]
    print(name, "n_dupli, n_split, n_prune, n_out", counts, "survivors by kind", survivors)
    assert min(n_dupli, n_split, n_prune) > 0 and min(survivors) > 0
    z = dict(N=sc["N"], C=sc["C"], width=sc["W"], height=sc["H"], step=sc["step"], scene_scale=sc["scene_scale"], grads=grads.numpy(),
             radii=radii.numpy(), noise=noise.numpy(), counts=np.array(counts), state_grad2d=st["grad2d"].numpy(), state_count=st["count"].numpy(),
             cfg_keys=np.array(sorted(sc["cfg"])), cfg_vals=np.array([float(sc["cfg"][k]) for k in sorted(sc["cfg"])]))
    if "radii" in st:
        z["state_radii"] = st["radii"].numpy()
    for k in KEYS:
        z["in_" + k], z["in_m_" + k], z["in_v_" + k] = p[k].numpy(), m[k].numpy(), v[k].numpy()
        z["out_" + k], z["out_m_" + k], z["out_v_" + k] = out[k].numpy(), mo[k].numpy(), vo[k].numpy()
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **z)


def absgrad_scene():
    """24 Gaussians, 2 cameras, 33 x 18 (ragged tiles both ways), 8 of them an opaque stack that reaches the T <= 1e-4 stop."""
    g = torch.Generator().manual_seed(5)
    n, W, H = 24, 33, 18
    u = lambda *s: torch.rand(*s, generator=g)
    means = torch.cat([(u(n, 2) - 0.5) * torch.tensor([1.0, 0.55]), 1.6 + u(n, 1)], 1)
    means[:8] = torch.tensor([[0.05, -0.03, 1.2 + 0.1 * i] for i in range(8)])
    quats = torch.randn(n, 4, generator=g)
    scales = torch.exp(-2.6 + 1.0 * u(n, 3))
    scales[:8] = 0.25
    opac = 0.2 + 0.6 * u(n)
    opac[:8] = 0.99
    colors = u(n, 3)
    vm = torch.eye(4).repeat(2, 1, 1)
    vm[1, :3, 3] = torch.tensor([0.1, -0.03, 0.05])
    K = torch.tensor([[30.0, 0, W / 2], [0, 30.0, H / 2], [0, 0, 1]]).repeat(2, 1, 1)
    cot = [torch.randn(2, H, W, ch, generator=g) for ch in (3, 1, 1)]
    return dict(means=means, quats=quats, scales=scales, opacities=opac, colors=colors, viewmats=vm, Ks=K), cot, W, H


def absgrad_reference(inp, cot, W, H, dtype):
    """-> grad [C,N,2] and absgrad [C,N,2] = sum over pixels of |d (cotangent . outputs at that pixel) / d means2d|"""
    t = {k: v.to(dtype) for k, v in inp.items()}
    radii, m2, depths, conics, _ = RG.project(t["means"], t["quats"], t["scales"], t["viewmats"], t["Ks"], W, H)
    m2 = m2.detach().requires_grad_(True)
    outs = RG.composite(m2, conics.detach(), depths.detach(), t["opacities"], t["colors"], radii, W, H)
    per_pixel = sum((o * c.to(dtype)).sum(-1) for o, c in zip(outs, cot))       # [C,H,W]
    grad, absg = torch.zeros_like(m2), torch.zeros_like(m2)
    for c in range(per_pixel.shape[0]):
        for i in range(H):
            for j in range(W):
                (gi,) = torch.autograd.grad(per_pixel[c, i, j], m2, retain_graph=True)
                grad += gi
                absg += gi.abs()
    return grad, absg, radii, outs


def gen_absgrad():
    inp, cot, W, H = absgrad_scene()
    g64, a64, radii, outs = absgrad_reference(inp, cot, W, H, torch.float64)
    g32, a32, _, _ = absgrad_reference(inp, cot, W, H, torch.float32)
    stopped = float((1 - outs[2]).min())
    print("absgrad scene: min transmittance", stopped, "visible pairs", int((radii > 0).all(-1).sum()))
    assert stopped < 2e-4, "the opaque stack must reach the stop"
    z = {"in_" + k: v.numpy() for k, v in inp.items()}
    z.update(width=W, height=H, cot_rgb=cot[0].numpy(), cot_depth=cot[1].numpy(), cot_alpha=cot[2].numpy(), grad64=g64.numpy(), absgrad64=a64.numpy(),
             grad32=g32.numpy(), absgrad32=a32.numpy(), radii=radii.numpy())
    np.savez_compressed(os.path.join(GOLD, "absgrad_24g_2c_33x18.npz"), **z)


if __name__ == "__main__":
    sys.path.insert(0, sys.argv[1])
    from gsplat.strategy import DefaultStrategy
    for name, sc in SCENES.items():
        gen_scene(DefaultStrategy, name, sc)
    gen_absgrad()
