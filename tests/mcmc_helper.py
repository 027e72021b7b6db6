"""TEST INFRASTRUCTURE ONLY (not a test file): a torch restatement, in any float dtype, of gsplat's MCMC ops (gsplat/strategy/ops.py:
relocate :244-297, sample_add :300-340, inject_noise_to_position :343-369) and of compute_relocation (eq. 9 of arXiv:2404.09591 as
gsplat/cuda/csrc/RelocationCUDA.cu:26-43 evaluates it: the literal double sum over a table of binomial coefficients).
Pinned to the reference's own results by tests/golden/mcmc_*.npz (tools/gen_golden_mcmc.py, tests/test_mcmc_cpu.py) — except eq. 9
itself, which the reference has only as a CUDA kernel: the fixtures hold THIS file's fp64 literal form for it."""
from __future__ import annotations

import math
import os

import numpy as np
import torch

N_MAX = 51
SCENES = ["mcmc_a_500g", "mcmc_b_130g"]
KEYS = ("means", "scales", "quats", "opacities", "sh0", "shN")
EPS32 = float(torch.finfo(torch.float32).eps)


def load_scene(name):
    return dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz")))


def tensors(z, prefix, dtype=None):
    """the fixture's six tensors under a prefix ("in_", "in_m_", "rel_", "out_v_", ...)"""
    out = {k: torch.from_numpy(z[prefix + k]) for k in KEYS}
    return out if dtype is None else {k: t.to(dtype) for k, t in out.items()}


def binoms(dtype):
    """mcmc.py:57-63"""
    b = torch.zeros((N_MAX, N_MAX), dtype=dtype)
    for n in range(N_MAX):
        for k in range(n + 1):
            b[n, k] = math.comb(n, k)
    return b


def ratios_of(sampled, n_max=N_MAX):
    """ops.py:275 and relocation.py:43: how often each drawn index was drawn, plus one, clamped"""
    return (torch.bincount(sampled)[sampled] + 1).clamp(1, n_max)


def relocation_literal(opacities, scales, ratios, dtype):
    """RelocationCUDA.cu:26-43 for opacities [n] (activated), scales [n,3] (activated), ratios [n] int: every term of the double sum
    in the kernel's order, in `dtype`.  -> new_opacities (not clamped), new_scales."""
    o, s = opacities.to(dtype), scales.to(dtype)
    table = binoms(dtype)
    new_o = 1.0 - torch.pow(1.0 - o, 1.0 / ratios.to(dtype))
    denom = torch.zeros_like(o)
    for i in range(1, int(ratios.max()) + 1 if len(ratios) else 1):
        live = ratios >= i
        for k in range(i):
            term = ((-1.0) ** k / math.sqrt(k + 1)) * torch.pow(new_o, k + 1)
            denom = torch.where(live, denom + table[i - 1, k] * term, denom)
    return new_o, (o / denom)[:, None] * s


def relocation_collapsed(opacities, scales, ratios, dtype):
    """the same sum after sum_{i=k+1..n} C(i-1, k) = C(n, k+1) (hockey stick): n terms, what wm_mcmc_relocation evaluates"""
    o, s = opacities.to(dtype), scales.to(dtype)
    new_o = 1.0 - torch.pow(1.0 - o, 1.0 / ratios.to(dtype))
    denom = torch.zeros_like(o)
    for j in range(len(o)):
        n = int(ratios[j])
        denom[j] = sum(math.comb(n, k + 1) * (-1.0) ** k / math.sqrt(k + 1) * new_o[j] ** (k + 1) for k in range(n))
    return new_o, (o / denom)[:, None] * s


def dead_alive(opacities, min_opacity):
    """mcmc.py:154-155, ops.py:258-259 -> dead, alive indices, ascending"""
    dead = torch.sigmoid(opacities.reshape(-1)) <= min_opacity
    return dead.nonzero(as_tuple=True)[0], (~dead).nonzero(as_tuple=True)[0]


def margins(opacities, min_opacity):
    """smallest relative distance of an opacity from the threshold it is compared with"""
    return float(((torch.sigmoid(opacities.reshape(-1)) - min_opacity).abs() / min_opacity).min())


def new_values(p, sampled, min_opacity, dtype):
    """ops.py:267-278 -> logit of the clamped new opacities [n], log of the new scales [n,3], the ratios"""
    op = torch.sigmoid(p["opacities"].to(dtype).reshape(-1))
    ratios = ratios_of(sampled)
    new_o, new_s = relocation_literal(op[sampled], torch.exp(p["scales"].to(dtype))[sampled], ratios, dtype)
    new_o = torch.clamp(new_o, max=1.0 - EPS32, min=min_opacity)
    return torch.logit(new_o), torch.log(new_s), ratios


def relocate(p, m, v, sampled, min_opacity, dtype):
    """ops.py:244-297 with the draw given (sampled: indices of alive Gaussians, one per dead one).  p, m, v: dicts of parameters and
    Adam moments -> new dicts (inputs untouched)."""
    dead, _ = dead_alive(p["opacities"].to(dtype), min_opacity)
    assert len(dead) == len(sampled)
    lo, ls, _ = new_values(p, sampled, min_opacity, dtype)
    out, mo, vo = {}, {}, {}
    for k in p:
        t = p[k].to(dtype).clone()
        if k == "opacities":
            t[sampled] = lo.reshape(t[sampled].shape)
        elif k == "scales":
            t[sampled] = ls
        t[dead] = t[sampled]
        out[k] = t
        mo[k], vo[k] = m[k].to(dtype).clone(), v[k].to(dtype).clone()
        mo[k][sampled] = 0
        vo[k][sampled] = 0
    return out, mo, vo


def sample_add(p, m, v, sampled, min_opacity, dtype):
    """ops.py:300-340 with the draw given -> new dicts of N + n rows"""
    lo, ls, _ = new_values(p, sampled, min_opacity, dtype)
    out, mo, vo = {}, {}, {}
    for k in p:
        t = p[k].to(dtype).clone()
        if k == "opacities":
            t[sampled] = lo.reshape(t[sampled].shape)
        elif k == "scales":
            t[sampled] = ls
        out[k] = torch.cat([t, t[sampled]])
        zeros = torch.zeros((len(sampled), *t.shape[1:]), dtype=dtype)
        mo[k], vo[k] = torch.cat([m[k].to(dtype), zeros]), torch.cat([v[k].to(dtype), zeros])
    return out, mo, vo


def quat_to_rotmat(q):
    q = q / q.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    w, x, y, z = q.unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1).reshape(-1, 3, 3)


def noise_displacement(quats, scales, opacities, noise, scaler, dtype):
    """ops.py:343-369 -> what is added to the means.  scales log, opacities logit, noise [N,3] standard normal."""
    op = torch.sigmoid(opacities.to(dtype).reshape(-1))
    M = quat_to_rotmat(quats.to(dtype)) * torch.exp(scales.to(dtype))[:, None, :]
    covars = torch.einsum("nij,nkj->nik", M, M)
    gate = 1 / (1 + torch.exp(-100 * ((1 - op) - 0.995)))
    nz = noise.to(dtype) * gate.unsqueeze(-1) * scaler
    return torch.einsum("bij,bj->bi", covars, nz)


def scene_facts(z):
    """-> dead, alive, the fixture's two draws as Gaussian indices, their multiplicities"""
    p = tensors(z, "in_", torch.float64)
    dead, alive = dead_alive(p["opacities"], float(z["min_opacity"]))
    s_rel, s_add = torch.from_numpy(z["sampled_relocate"]), torch.from_numpy(z["sampled_add"])
    return dead, alive, s_rel, s_add, torch.bincount(s_rel)[s_rel], torch.bincount(s_add)[s_add]


def check_scene_properties(name, z):
    """what tools/gen_golden_mcmc.py asserted when it wrote the fixture"""
    N, mo = int(z["N"]), float(z["min_opacity"])
    dead, alive, s_rel, s_add, c_rel, c_add = scene_facts(z)
    assert margins(torch.from_numpy(z["in_opacities"]).double(), mo) > 1e-4           # fp32 rounding cannot flip who is dead
    assert len(dead) + len(alive) == N and len(s_rel) == len(dead) > 0 and len(s_add) == len(z["out_means"]) - N > 0
    assert torch.equal(alive[torch.from_numpy(z["draw_relocate"])], s_rel)                # the draw is among the alive ones
    if name == "mcmc_a_500g":
        assert 0.08 * N <= len(dead) <= 0.12 * N
        c = set(c_rel.tolist())
        assert 1 in c and 2 in c and max(c) >= 3 and max(c) + 1 <= N_MAX              # ratios 2, 3 and >= 4, none clamped
        assert len(s_add) == int(z["cap_max"]) - N < int(1.05 * N) - N                    # growth limited by the cap
    else:
        assert len(alive) <= 8 and int(c_rel.max()) + 1 > N_MAX                        # the ratio clamp binds
        assert len(s_add) == int(1.05 * N) - N and int(z["cap_max"]) > int(1.05 * N)      # growth limited by 5 %
