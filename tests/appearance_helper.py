"""A torch restatement of the appearance module (what hunyuanworld_mirror_amd.appearance fuses), generic in the dtype: in fp64 it is the
reference for the GPU tests, in fp32 their yardstick, and on the GPU in fp32 the torch composition tools/bench_appearance.py times.
Pinned to the reference's own numbers by tests/test_appearance_cpu.py.

Per (camera c, Gaussian g): h = [embed[c] (16) | features[g] (32) | basis (module bands)], the basis being the real spherical harmonics of
d / max(|d|, 1e-12) up to the call's degree and zeros above it; out = W3 relu(W2 relu(W1 h + b1) + b2) + b3, before any sigmoid."""
import os

import numpy as np
import torch
import torch.nn.functional as F

KEYS = ("embeds.weight", "color_head.0.weight", "color_head.0.bias", "color_head.2.weight", "color_head.2.bias", "color_head.4.weight",
        "color_head.4.bias")
FEATURE_DIM, EMBED_DIM, WIDTH = 32, 16, 64


def sh_bases(n_bases, d):
    """the first n_bases (1, 4, 9 or 16) real SH basis polynomials of unit directions d [..., 3] (Sloan, JCGT 2013) -> [..., n_bases]"""
    x, y, z = d.unbind(-1)
    out = [torch.full_like(x, 0.2820947917738781)]
    if n_bases > 1:
        out += [-0.48860251190292 * y, 0.48860251190292 * z, -0.48860251190292 * x]
    if n_bases > 4:
        z2, c1, s1 = z * z, x * x - y * y, 2 * x * y
        out += [0.5462742152960395 * s1, -1.092548430592079 * z * y, 0.9461746957575601 * z2 - 0.3153915652525201,
                -1.092548430592079 * z * x, 0.5462742152960395 * c1]
        if n_bases > 9:
            c2, s2, pz = x * c1 - y * s1, x * s1 + y * c1, 0.4570457994644658 - 2.285228997322329 * z2
            out += [-0.5900435899266435 * s2, 1.445305721320277 * z * s1, pz * y, z * (1.865881662950577 * z2 - 1.119528997770346),
                    pz * x, 1.445305721320277 * z * c1, -0.5900435899266435 * c2]
    return torch.stack(out, -1)


def hidden(state, features, ids, dirs, degree):
    """-> (z1, z2): the two hidden pre-activations [C, N, 64]"""
    C, N = dirs.shape[:2]
    dt, dev = features.dtype, features.device
    n_module = state["color_head.0.weight"].shape[1] - EMBED_DIM - FEATURE_DIM
    emb = torch.zeros(C, EMBED_DIM, dtype=dt, device=dev) if ids is None else state["embeds.weight"][ids]
    basis = torch.zeros(C, N, n_module, dtype=dt, device=dev)
    basis[..., :(degree + 1) ** 2] = sh_bases((degree + 1) ** 2, F.normalize(dirs, dim=-1))
    h = torch.cat([emb[:, None, :].expand(-1, N, -1), features[None].expand(C, -1, -1), basis], -1)
    z1 = h @ state["color_head.0.weight"].T + state["color_head.0.bias"]
    z2 = torch.relu(z1) @ state["color_head.2.weight"].T + state["color_head.2.bias"]
    return z1, z2


def forward(state, features, ids, dirs, degree):
    _, z2 = hidden(state, features, ids, dirs, degree)
    return torch.relu(z2) @ state["color_head.4.weight"].T + state["color_head.4.bias"]


def gradients(state, features, ids, dirs, v_out, degree, dtype, device="cpu"):
    """the module in dtype from (fp32-valued) inputs -> dict: out, v_features, v_dirs and one entry per parameter key"""
    st = {k: torch.as_tensor(v).detach().to(device=device, dtype=dtype).requires_grad_(True) for k, v in state.items() if k in KEYS}
    f = features.detach().to(device=device, dtype=dtype).requires_grad_(True)
    d = dirs.detach().to(device=device, dtype=dtype).requires_grad_(True)
    ids = None if ids is None else torch.as_tensor(ids).to(device=device, dtype=torch.long)
    out = forward(st, f, ids, d, degree)
    (out * v_out.to(device=device, dtype=dtype)).sum().backward()
    res = dict(out=out.detach(), v_features=f.grad, v_dirs=torch.zeros_like(d) if d.grad is None else d.grad)      # degree 0: a constant basis
    for k in KEYS:
        res[k] = torch.zeros_like(st[k]) if st[k].grad is None else st[k].grad
    return res


def _pre_activations(state, features, ids, dirs, degree):
    pre = {}
    for dt in (torch.float64, torch.float32):
        st = {k: torch.as_tensor(v).to(dt) for k, v in state.items() if k in KEYS}
        pre[dt] = torch.cat(hidden(st, features.to(dt), ids, dirs.to(dt), degree), -1)      # [C, N, 128]
    return pre[torch.float64], pre[torch.float32].double()


def relu_margin(state, features, ids, dirs, degree):
    """(smallest |hidden pre-activation| of any pair in fp64, largest fp32-against-fp64 difference of those pre-activations).  ReLU has a
    kink at zero: a pre-activation that fp32 rounding can push across it changes a gradient by a finite amount."""
    p64, p32 = _pre_activations(state, features, ids, dirs, degree)
    return float(p64.abs().min()), float((p32 - p64).abs().max())


def random_state(n, module_degree, gen, scale=1.0):
    """parameters as nn.Embedding / nn.Linear initialise them (normal; uniform in +-1 / sqrt(fan_in)), from gen, fp32"""
    in_dim = EMBED_DIM + FEATURE_DIM + (module_degree + 1) ** 2
    u = lambda shape, fan: (torch.rand(*shape, generator=gen) * 2 - 1) * scale / fan ** 0.5
    return {"embeds.weight": torch.randn(n, EMBED_DIM, generator=gen),
            "color_head.0.weight": u((WIDTH, in_dim), in_dim), "color_head.0.bias": u((WIDTH,), in_dim),
            "color_head.2.weight": u((WIDTH, WIDTH), WIDTH), "color_head.2.bias": u((WIDTH,), WIDTH),
            "color_head.4.weight": u((3, WIDTH), WIDTH), "color_head.4.bias": u((3,), WIDTH)}


def random_scene(n, C, N, module_degree, degree, ids, seed0=0, tries=2000, redraw=False):
    """a scene whose hidden pre-activations all lie at least 16 x their own fp32 error from zero
    -> dict(state, features, ids, dirs, v_out, degree, margin, seed).  redraw = False: the next seed until a whole scene does (the golden
    generator's search; it succeeds within some tens of seeds up to about 10^5 pre-activations).  redraw = True, for larger scenes, where
    a whole draw practically never passes: the Gaussians that have a pre-activation within 24 x the error are drawn again (features
    and directions, from the same generator) until the same condition holds for every pair; no pair is left out."""
    for seed in range(seed0, seed0 + tries):
        g = torch.Generator().manual_seed(seed)
        state = random_state(n, module_degree, g)
        features = torch.randn(N, FEATURE_DIM, generator=g)
        dirs = torch.randn(C, N, 3, generator=g) * 2.0
        v_out = torch.randn(C, N, 3, generator=g)
        t_ids = None if ids is None else torch.tensor(ids)
        for _ in range(200 if redraw else 1):
            p64, p32 = _pre_activations(state, features, t_ids, dirs, degree)
            lo, err = float(p64.abs().min()), float((p32 - p64).abs().max())
            if lo >= 16 * err:
                return dict(state=state, features=features, ids=t_ids, dirs=dirs, v_out=v_out, degree=degree, margin=16 * err, seed=seed)
            if redraw:
                bad = (p64.abs() < 24 * err).any(-1).any(0).nonzero().reshape(-1)
                features[bad] = torch.randn(len(bad), FEATURE_DIM, generator=g)
                dirs[:, bad] = torch.randn(C, len(bad), 3, generator=g) * 2.0
    raise AssertionError(f"no seed in [{seed0}, {seed0 + tries}) keeps every hidden pre-activation off zero (C={C}, N={N})")


def max_rel(a, b):
    """largest |a - b| relative to the largest |b|"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def load_golden(name):
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    return dict(np.load(os.path.join(gold, f"appearance_{name}.npz"), allow_pickle=False))
