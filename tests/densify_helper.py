"""TEST INFRASTRUCTURE ONLY (not a test file): a torch restatement, in any float dtype, of gsplat's DefaultStrategy bookkeeping
(gsplat/strategy/default.py:203-339, ops.py:93-210) in the three steps the HIP entries take: update_state (accumulate), plan
(duplicate -> split -> remove followed literally, with the index bookkeeping the concatenations imply) and gather.
Pinned to the reference's own results by tests/golden/densify_*.npz (tools/gen_golden_densify.py, tests/test_densify_cpu.py)."""
from __future__ import annotations

import os

import numpy as np
import torch

KEEP, DUP, SPLIT0, SPLIT1 = 0, 1, 2, 3
DEFAULTS = dict(prune_opa=0.005, grow_grad2d=0.0002, grow_scale3d=0.01, grow_scale2d=0.05, prune_scale3d=0.1, prune_scale2d=0.15,
                refine_scale2d_stop_iter=0, refine_start_iter=500, refine_stop_iter=15000, reset_every=3000, refine_every=100,
                pause_refine_after_reset=0, absgrad=False, revised_opacity=False)


SCENES = ["densify_a_500g_3c", "densify_b_600g_2c"]
KEYS = ("means", "scales", "quats", "opacities", "sh0", "shN")


def load_scene(name):
    """-> the fixture's arrays and the strategy's configuration (DEFAULTS with the scene's overrides)"""
    z = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz")))
    cfg = dict(DEFAULTS)
    for k, v in zip(z["cfg_keys"], z["cfg_vals"]):
        cfg[str(k)] = type(DEFAULTS[str(k)])(v)
    return z, cfg


def helper_state(z, dtype):
    """the running state after the fixture's two accumulations"""
    N = int(z["N"])
    g2, cnt = torch.zeros(N, dtype=dtype), torch.zeros(N, dtype=dtype)
    rs = torch.zeros(N, dtype=dtype) if "state_radii" in z else None
    for i in range(2):
        g2, cnt, rs = update_state(torch.from_numpy(z["grads"][i]), torch.from_numpy(z["radii"][i]), int(z["width"]), int(z["height"]), g2, cnt, rs, dtype)
    return g2, cnt, rs


def update_state(grads, radii, width, height, grad2d, count, radii_state, dtype):
    """default.py:220-260 -> new grad2d, count, radii_state (None stays None).  grads [C,N,2], radii [C,N,2] int."""
    C = grads.shape[0]
    g = grads.to(dtype).clone()
    g[..., 0] *= width / 2.0 * C
    g[..., 1] *= height / 2.0 * C
    sel = (radii > 0).all(-1)
    ids = torch.where(sel)[1]
    grad2d = grad2d.to(dtype).clone().index_add_(0, ids, g[sel].norm(dim=-1))
    count = count.to(dtype).clone().index_add_(0, ids, torch.ones(len(ids), dtype=dtype))
    if radii_state is not None:
        r = radii[sel].max(-1).values.to(dtype) / float(max(width, height))
        radii_state = radii_state.to(dtype).clone()
        for i, v in zip(ids.tolist(), r.tolist()):          # a true scatter-max (the reference's indexed maximum keeps one writer)
            radii_state[i] = max(float(radii_state[i]), v)
    return grad2d, count, radii_state


def _quantities(grad2d, count, scales, opacities, cfg, step):
    mean = grad2d / count.clamp_min(1)
    smax = torch.exp(scales).max(-1).values
    op = torch.sigmoid(opacities.reshape(-1))
    use2d = step < cfg["refine_scale2d_stop_iter"]
    big = step > cfg["reset_every"]
    return mean, smax, op, use2d, big


def plan(grad2d, count, radii_state, scales, opacities, cfg, step, scene_scale=1.0):
    """-> src, kind, rank (int64 [n_out]) and (n_dupli, n_split, n_prune, n_out)"""
    N = scales.shape[0]
    mean, smax, op, use2d, big = _quantities(grad2d, count, scales, opacities, cfg, step)
    high = mean > cfg["grow_grad2d"]
    small = smax <= cfg["grow_scale3d"] * scene_scale
    is_dupli = high & small
    is_split = high & ~small
    if use2d:
        is_split = is_split | (radii_state > cfg["grow_scale2d"])
    # duplicate (ops.py:93-120)
    dsel = torch.where(is_dupli)[0]
    src = torch.cat([torch.arange(N), dsel])
    kind = torch.cat([torch.full((N,), KEEP), torch.full((len(dsel),), DUP)])
    is_split = torch.cat([is_split, torch.zeros(len(dsel), dtype=torch.bool)])
    # split (ops.py:123-180)
    ssel, rest = torch.where(is_split)[0], torch.where(~is_split)[0]
    ns = len(ssel)
    rank = torch.cat([torch.zeros(len(rest), dtype=torch.int64), torch.arange(ns), torch.arange(ns)])
    kind = torch.cat([kind[rest], torch.full((ns,), SPLIT0), torch.full((ns,), SPLIT1)])
    src = torch.cat([src[rest], src[ssel], src[ssel]])
    # remove (default.py:312-339, ops.py:183-210) on every produced entry's own values
    child = kind >= SPLIT0
    own_op = op[src]
    if cfg["revised_opacity"]:
        own_op = torch.where(child, 1.0 - torch.sqrt(1.0 - op[src]), own_op)
    own_s = torch.where(child, smax[src] / 1.6, smax[src])
    prune = own_op < cfg["prune_opa"]
    if big:
        too_big = own_s > cfg["prune_scale3d"] * scene_scale
        if use2d:
            too_big = too_big | (radii_state[src] > cfg["prune_scale2d"])
        prune = prune | too_big
    keep = torch.where(~prune)[0]
    return src[keep], kind[keep], rank[keep], (len(dsel), ns, int(prune.sum()), len(keep))


def margins(grad2d, count, radii_state, scales, opacities, cfg, step, scene_scale=1.0):
    """smallest relative distance of every compared quantity from every threshold it is compared with"""
    mean, smax, op, use2d, big = _quantities(grad2d, count, scales, opacities, cfg, step)
    rel = lambda x, t: float(((x - t).abs() / t).min())
    out = {"grad2d": rel(mean, cfg["grow_grad2d"]), "grow_scale3d": rel(smax, cfg["grow_scale3d"] * scene_scale),
           "opacity": min(rel(op, cfg["prune_opa"]), rel(1.0 - torch.sqrt(1.0 - op), cfg["prune_opa"]))}
    if big:
        out["prune_scale3d"] = min(rel(smax, cfg["prune_scale3d"] * scene_scale), rel(smax / 1.6, cfg["prune_scale3d"] * scene_scale))
    if use2d:
        out["radii"] = min(rel(radii_state, cfg["grow_scale2d"]), rel(radii_state, cfg["prune_scale2d"]))
    return out


def quat_to_rotmat(q):
    q = q / q.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    w, x, y, z = q.unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1).reshape(-1, 3, 3)


def gather(t, src, kind, rank, mode, dtype, quats=None, scales=None, noise=None):
    """mode: copy | zero_new | means | scales | opacities_revised.  noise [2, >= n_split, 3]."""
    t = t.to(dtype)
    out = t[src].clone()
    child = kind >= SPLIT0
    if mode == "zero_new":
        out[kind != KEEP] = 0
    elif mode == "means" and child.any():
        g, b = src[child], (kind[child] == SPLIT1).long()
        R = quat_to_rotmat(quats.to(dtype)[g])
        z = noise.to(dtype)[b, rank[child]]
        out[child] = t[g] + torch.einsum("nij,nj,nj->ni", R, torch.exp(scales.to(dtype)[g]), z)
    elif mode == "scales":
        out[child] = torch.log(torch.exp(t[src[child]]) / 1.6)
    elif mode == "opacities_revised":
        out[child] = torch.logit(1.0 - torch.sqrt(1.0 - torch.sigmoid(t[src[child]])))
    return out


def gather_mode(name, revised_opacity):
    return {"means": "means", "scales": "scales"}.get(name, "opacities_revised" if name == "opacities" and revised_opacity else "copy")
