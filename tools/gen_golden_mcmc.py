"""Writes tests/golden/mcmc_*.npz: inputs and the results of the REFERENCE's gsplat.strategy.MCMCStrategy.step_post_backward on them
(CPU, fp64).  Data only.

    python tools/gen_golden_mcmc.py <path to the reference's gsplat checkout (the directory that holds the gsplat package)>

Scenes (N <= 600): inputs are fp32 values; the reference runs on their fp64 casts, so its results are the exact-arithmetic answer to
the inputs a fp32 implementation receives.  The Adam moments come from one real fp32 optimiser step.  One step_post_backward call per
scene, at a refinement step: relocate -> add -> noise.  For the call
  ops._multinomial_sample            is wrapped to record its draws (relocation: positions among the alive Gaussians; growth: indices),
  torch.randn_like                   is wrapped to draw in fp32 and record the draw,
  ops.quat_scale_to_covar_preci      (a CUDA kernel) is replaced by the reference's own torch form,
                                     gsplat.cuda._torch_impl._quat_scale_to_covar_preci,
  ops.compute_relocation             which the reference has ONLY as a CUDA kernel (gsplat/cuda/csrc/RelocationCUDA.cu), is replaced by
                                     tests/mcmc_helper.py's fp64 literal form of that kernel (the ratio clamp of relocation.py:43 included).
Eq. 9 itself is therefore pinned to the paper and to the kernel's source as read, NOT to a run of the reference.  What the reference's
own code pins: the bookkeeping (who is dead, who is drawn, the ratios), the order of the writes, the clamp of the new opacities, the
handling of the Adam moments, the covariance and the gate of the position noise.  Snapshots are taken after relocation and at the end.

Asserted here and again in the tests:
  mcmc_a_500g  about 10 % dead; a few Gaussians far more opaque than the rest, so that sources drawn once, twice and three or more
               times all occur (ratios 2, 3 and >= 4: a drawn index is counted at least once, so a ratio of 1 cannot come out of a
               draw; the closed-form test covers it); growth limited by cap_max.
  mcmc_b_130g  a handful alive, the rest dead: one index is drawn more than 51 times and the ratio clamp binds; growth limited by
               int(1.05 N).
  No opacity lies within relative 1e-4 of min_opacity (fp32 rounding cannot flip a decision).  If a scene violates any of this,
  change its seed."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mcmc_helper as MH  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
KEYS = MH.KEYS

SCENES = {
    "mcmc_a_500g": dict(seed=31, N=500, n_dead=50, n_bright=5, cap_max=515, step=200, lr=1.6e-4, noise_lr=5e5, min_opacity=0.005),
    "mcmc_b_130g": dict(seed=32, N=130, n_dead=126, n_bright=1, cap_max=1_000_000, step=300, lr=1.0e-4, noise_lr=5e5, min_opacity=0.005),
}


def make_inputs(sc):
    g = torch.Generator().manual_seed(sc["seed"])
    N = sc["N"]
    u = lambda *s: torch.rand(*s, generator=g)
    opac = 10 ** (-2.2 + 0.9 * u(N))                                  # alive and faint: 0.0063 .. 0.05
    perm = torch.randperm(N, generator=g)
    opac[perm[:sc["n_dead"]]] = 10 ** (-3.5 + 1.1 * u(sc["n_dead"]))  # dead: 0.0003 .. 0.004
    bright = perm[sc["n_dead"]: sc["n_dead"] + sc["n_bright"]]
    opac[bright] = 0.9 + 0.09 * u(sc["n_bright"])
    return {"means": torch.randn(N, 3, generator=g), "scales": torch.log(10 ** (-2.2 + 1.4 * u(N, 3))), "quats": torch.randn(N, 4, generator=g),
            "opacities": torch.logit(opac), "sh0": u(N, 1, 3), "shN": torch.randn(N, 3, 3, generator=g) * 0.1}


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


def run_reference(gsplat_ops, MCMCStrategy, covar_fn, sc, p, m, v):
    strat = MCMCStrategy(cap_max=sc["cap_max"], noise_lr=sc["noise_lr"], refine_start_iter=0, refine_every=100, min_opacity=sc["min_opacity"])
    params = torch.nn.ParameterDict({k: torch.nn.Parameter(t.double()) for k, t in p.items()})
    opts = {}
    for k in params:
        opts[k] = torch.optim.Adam([params[k]], lr=1e-3)
        opts[k].state[params[k]] = {"step": torch.tensor(1.0), "exp_avg": m[k].double(), "exp_avg_sq": v[k].double()}
    strat.check_sanity(params, opts)
    state = strat.initialize_state()
    draws, noise, snaps = [], [], []

    def snapshot():
        snaps.append(({k: params[k].detach().clone() for k in params}, {k: opts[k].state[params[k]]["exp_avg"].clone() for k in params},
                      {k: opts[k].state[params[k]]["exp_avg_sq"].clone() for k in params}))

    real = dict(multinomial=gsplat_ops._multinomial_sample, covar=gsplat_ops.quat_scale_to_covar_preci, reloc=gsplat_ops.compute_relocation,
                randn_like=torch.randn_like, relocate_gs=strat._relocate_gs)

    def multinomial(weights, n, replacement=True):
        d = real["multinomial"](weights, n, replacement=replacement)
        draws.append(d.clone())
        return d

    def randn_like32(t, **kw):
        kw.pop("dtype", None)
        z = real["randn_like"](t, dtype=torch.float32, **kw)
        noise.append(z.clone())
        return z.double()

    def compute_relocation(opacities, scales, ratios, binoms):
        ratios.clamp_(min=1, max=binoms.shape[0])                      # relocation.py:43
        return MH.relocation_literal(opacities, scales, ratios, torch.float64)

    def relocate_gs(*a, **k):
        n = real["relocate_gs"](*a, **k)
        snapshot()
        return n

    torch.manual_seed(sc["seed"])
    gsplat_ops._multinomial_sample, gsplat_ops.quat_scale_to_covar_preci, gsplat_ops.compute_relocation = multinomial, covar_fn, compute_relocation
    torch.randn_like = randn_like32
    object.__setattr__(strat, "_relocate_gs", relocate_gs)
    empty_cache = torch.cuda.empty_cache
    torch.cuda.empty_cache = lambda: None
    try:
        strat.step_post_backward(params, opts, state, sc["step"], {}, lr=sc["lr"])
    finally:
        gsplat_ops._multinomial_sample, gsplat_ops.quat_scale_to_covar_preci, gsplat_ops.compute_relocation = real["multinomial"], real["covar"], real["reloc"]
        torch.randn_like, torch.cuda.empty_cache = real["randn_like"], empty_cache
    snapshot()
    assert len(draws) == 2 and len(noise) == 1 and len(snaps) == 2
    assert all(float(opts[k].state[params[k]]["step"]) == 1.0 for k in params)
    return draws, noise[0], snaps


def gen_scene(gsplat_ops, MCMCStrategy, covar_fn, name, sc):
    p, m, v = adam_moments(make_inputs(sc), sc["seed"])
    torch.set_default_dtype(torch.float64)      # the reference allocates the new moments in the default dtype
    try:
        draws, noise, (rel, out) = run_reference(gsplat_ops, MCMCStrategy, covar_fn, sc, p, m, v)
    finally:
        torch.set_default_dtype(torch.float32)
    N, mo = sc["N"], sc["min_opacity"]
    mg = MH.margins(p["opacities"].double(), mo)          # the one decision of the step: who is dead
    dead, alive = MH.dead_alive(p["opacities"].double(), mo)
    sampled_rel, sampled_add = alive[draws[0]], draws[1]
    n_add = len(out[0]["means"]) - N
    counts_rel, counts_add = torch.bincount(sampled_rel)[sampled_rel], torch.bincount(sampled_add)[sampled_add]
    print(name, f"margin {mg:.2e} dead {len(dead)} added {n_add} multiplicities relocate {sorted(set(counts_rel.tolist()))} add {sorted(set(counts_add.tolist()))}")
    assert mg > 1e-4, mg
    assert len(sampled_rel) == len(dead) and len(sampled_add) == n_add > 0
    if name == "mcmc_a_500g":
        assert 0.08 * N <= len(dead) <= 0.12 * N
        c = set(counts_rel.tolist())
        assert 1 in c and 2 in c and max(c) >= 3 and max(c) + 1 <= MH.N_MAX, c
        assert n_add == sc["cap_max"] - N < int(1.05 * N) - N
    else:
        assert len(alive) <= 8 and int(counts_rel.max()) + 1 > MH.N_MAX
        assert n_add == int(1.05 * N) - N and sc["cap_max"] > int(1.05 * N)
    z = dict(N=N, cap_max=sc["cap_max"], step=sc["step"], lr=sc["lr"], noise_lr=sc["noise_lr"], min_opacity=mo, draw_relocate=draws[0].numpy(),
             sampled_relocate=sampled_rel.numpy(), sampled_add=sampled_add.numpy(), noise=noise.numpy())
    for k in KEYS:
        z["in_" + k], z["in_m_" + k], z["in_v_" + k] = p[k].numpy(), m[k].numpy(), v[k].numpy()
        z["rel_" + k], z["rel_m_" + k], z["rel_v_" + k] = (t[k].numpy() for t in rel)
        z["out_" + k], z["out_m_" + k], z["out_v_" + k] = (t[k].numpy() for t in out)
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **z)


if __name__ == "__main__":
    sys.path.insert(0, sys.argv[1])
    from gsplat.cuda._torch_impl import _quat_scale_to_covar_preci
    from gsplat.strategy import MCMCStrategy
    from gsplat.strategy import ops as gsplat_ops
    for name, sc in SCENES.items():
        gen_scene(gsplat_ops, MCMCStrategy, _quat_scale_to_covar_preci, name, sc)
