"""gsplat's ``MCMCStrategy`` (gsplat/strategy/mcmc.py, ops.py:240-369; "3D Gaussian Splatting as Markov Chain Monte Carlo",
arXiv:2404.09591) — the other strategy of the reference's "Post 3DGS Optimization" trainer (simple_trainer_worldmirror.py:130, the
``mcmc`` preset) — over the HIP entries ``wm_mcmc_inject_noise`` / ``wm_mcmc_partition`` / ``wm_mcmc_relocation`` /
``wm_mcmc_scatter`` / ``wm_mcmc_zero_rows``.  Same field names and defaults, same methods and module-level ops, same objects as
``strategy.DefaultStrategy``: ``params`` a dict / ``ParameterDict`` of contiguous fp32 ``[N, ...]`` parameters with ``means``,
``scales`` (log), ``quats`` (wxyz), ``opacities`` (logit, ``[N]`` or ``[N, 1]``) among them, ``optimizers`` a dict with one
single-group optimiser per trainable key.  No CPU fallback: the tensors live on a HIP device.

The random draws stay in torch so that they can be pinned: ``torch.multinomial`` for the relocation and growth sources,
``torch.randn`` for the position noise, each from ``generator``; ``sampled_idxs`` / ``noise`` replace them with the caller's own.

Not built: packed layouts, and the numpy sampler the reference switches to above 2**24 categories (``NotImplementedError``)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Any, Dict, Optional

import torch

from . import _lib
from ._lib import check, ptr, stream
from .strategy import _check

MAX_MULTINOMIAL = 2 ** 24       # torch.multinomial's limit on the number of categories (ops.py:30)


def _idx(t: torch.Tensor, name: str) -> torch.Tensor:
    _check(t, torch.int32, name)
    return t


def mcmc_inject_noise(means, quats, scales, opacities, noise, scaler: float) -> None:
    """ops.py:343-369 in place on means [N,3]: means += Sigma (noise * gate * scaler).  noise [N,3] standard normal."""
    N = int(means.shape[0])
    for t, name, shape in ((means, "means", (N, 3)), (quats, "quats", (N, 4)), (scales, "scales", (N, 3)), (noise, "noise", (N, 3))):
        _check(t, torch.float32, name)
        if tuple(t.shape) != shape:
            raise ValueError(f"{name}: {shape} expected, got {tuple(t.shape)}")
    _check(opacities, torch.float32, "opacities")
    if opacities.numel() != N:
        raise ValueError("opacities: [N] or [N,1]")
    if N == 0:
        return
    check(_lib.lib().wm_mcmc_inject_noise(ptr(means), ptr(quats), ptr(scales), ptr(opacities), ptr(noise), float(scaler), N, stream(means.device)),
          "wm_mcmc_inject_noise")


def mcmc_partition(opacities: torch.Tensor, min_opacity: float, mask: Optional[torch.Tensor] = None):
    """-> dead_idx, alive_idx (int32, ascending): dead = sigmoid(opacities) <= min_opacity, or the bool mask [N] when one is given.
    Synchronises the stream once."""
    op = opacities.detach().reshape(-1)
    _check(op, torch.float32, "opacities")
    N = op.numel()
    dev = op.device
    if mask is not None:
        if mask.device != dev or mask.dtype != torch.bool or mask.numel() != N or not mask.is_contiguous():
            raise ValueError("mask: a contiguous bool [N] tensor on the parameters' device")
    rows = torch.empty((2, N), device=dev, dtype=torch.int32)
    if N == 0:
        return rows[0], rows[1]
    L = _lib.lib()
    ws = torch.empty(L.wm_mcmc_partition_workspace_bytes(N), device=dev, dtype=torch.uint8)
    counts = (C.c_int * 2)()
    check(L.wm_mcmc_partition(ptr(op), ptr(mask), N, float(min_opacity), ptr(rows[0]), ptr(rows[1]), C.byref(counts), ptr(ws), ws.numel(),
                              stream(dev)), "wm_mcmc_partition")
    return rows[0, :int(counts[0])], rows[1, :int(counts[1])]


def mcmc_relocation(opacities: torch.Tensor, scales: torch.Tensor, sampled: torch.Tensor, min_opacity: float, return_counts: bool = False):
    """eq. 9 for the drawn sources -> new logit opacities [n], new log scales [n,3] (what relocate / sample_add write); with
    return_counts also how often each Gaussian was drawn (int32 [N]: the histogram the ratios come from)."""
    op, sc = opacities.detach().reshape(-1), scales.detach()
    _check(op, torch.float32, "opacities"); _check(sc, torch.float32, "scales"); _idx(sampled, "sampled_idxs")
    N, n = op.numel(), sampled.numel()
    if tuple(sc.shape) != (N, 3):
        raise ValueError("scales: [N,3]")
    dev = op.device
    new_op, new_sc = torch.empty(n, device=dev), torch.empty((n, 3), device=dev)
    hist = torch.zeros(N, device=dev, dtype=torch.int32)
    if n:
        check(_lib.lib().wm_mcmc_relocation(ptr(op), ptr(sc), ptr(sampled), n, N, float(min_opacity), ptr(new_op), ptr(new_sc), ptr(hist), stream(dev)),
              "wm_mcmc_relocation")
    return (new_op, new_sc, hist) if return_counts else (new_op, new_sc)


def mcmc_scatter(t: torch.Tensor, sampled: torch.Tensor, dest: torch.Tensor, values: Optional[torch.Tensor] = None) -> None:
    """t [rows, ...] in place: t[sampled[j]] = t[dest[j]] = values[j] (or t[sampled[j]] without values)."""
    _check(t, torch.float32, "tensor"); _idx(sampled, "sampled_idxs"); _idx(dest, "dest")
    n, rows = sampled.numel(), int(t.shape[0])
    if dest.numel() != n:
        raise ValueError("sampled_idxs and dest differ in length")
    if n == 0:
        return
    R = t.numel() // rows
    if values is not None:
        _check(values, torch.float32, "values")
        if values.numel() != n * R:
            raise ValueError("values: one row per drawn index")
    check(_lib.lib().wm_mcmc_scatter(ptr(t), rows, R, ptr(sampled), ptr(dest), ptr(values), n, stream(t.device)), "wm_mcmc_scatter")


def mcmc_zero_rows(t: torch.Tensor, idx: torch.Tensor) -> None:
    """t[idx] = 0 in place."""
    _check(t, torch.float32, "tensor"); _idx(idx, "idx")
    if idx.numel() == 0:
        return
    rows = int(t.shape[0])
    check(_lib.lib().wm_mcmc_zero_rows(ptr(t), rows, t.numel() // rows, ptr(idx), idx.numel(), stream(t.device)), "wm_mcmc_zero_rows")


def _multinomial_sample(probs: torch.Tensor, n: int, generator: Optional[torch.Generator]) -> torch.Tensor:
    if probs.numel() > MAX_MULTINOMIAL:
        raise NotImplementedError(f"sampling among more than 2**24 Gaussians is not built (the reference switches to numpy.random.choice there); "
                                  f"got {probs.numel()}: pass sampled_idxs from a sampler of your own")
    return torch.multinomial(probs, n, replacement=True, generator=generator)


def _given(sampled_idxs: torch.Tensor, n: int, N: int, dev) -> torch.Tensor:
    s = sampled_idxs.to(device=dev, dtype=torch.int32).contiguous()
    if s.dim() != 1 or s.numel() != n:
        raise ValueError(f"sampled_idxs: {n} indices expected, got {tuple(s.shape)}")
    if n and (int(s.min()) < 0 or int(s.max()) >= N):
        raise ValueError(f"sampled_idxs: indices in [0, {N}) expected")
    return s


def _update_param_with_optimizer(param_fn, optimizer_fn, params, optimizers) -> None:
    """ops.py:48-89, as strategy.apply_plan re-keys: a new nn.Parameter per name, the optimiser's single param group and its state
    follow it, "step" is kept."""
    for name in list(params.keys()):
        p = params[name]
        new_p = torch.nn.Parameter(param_fn(name, p.detach()), requires_grad=p.requires_grad)
        params[name] = new_p
        if name not in optimizers:
            assert not p.requires_grad, f"Optimizer for {name} is not found, but the parameter is trainable."
            continue
        opt = optimizers[name]
        for group in opt.param_groups:
            st = opt.state.pop(p, {})
            for key, v in st.items():
                if key != "step":
                    st[key] = optimizer_fn(key, v)
            group["params"] = [new_p]
            opt.state[new_p] = st


def _require(params) -> None:
    for name, p in params.items():
        _check(p.detach(), torch.float32, name)


@torch.no_grad()
def relocate(params, optimizers, state: Dict[str, Any], mask: Optional[torch.Tensor], min_opacity: float = 0.005,
             generator: Optional[torch.Generator] = None, sampled_idxs: Optional[torch.Tensor] = None) -> int:
    """ops.py:244-297: every dead Gaussian becomes a copy of an alive one drawn with probability proportional to its opacity; the
    sources and their copies share the opacity and scale of eq. 9.  In place on the parameters' storage (new Parameter objects);
    the Adam moments of the SOURCES are zeroed, those of the dead rows stay as they were (as in the reference).
    mask: bool [N], or None for sigmoid(opacities) <= min_opacity.  -> the number of relocated Gaussians; 0 leaves every object
    untouched."""
    _require(params)
    N = len(params["means"])
    dead, alive = mcmc_partition(params["opacities"], min_opacity, mask)
    n = dead.numel()
    if n == 0:
        return 0
    if alive.numel() == 0:
        raise RuntimeError(f"relocate: all {N} Gaussians are dead (opacity <= {min_opacity}), there is none to relocate them to")
    dev = dead.device
    if sampled_idxs is None:
        probs = torch.sigmoid(params["opacities"].detach().reshape(-1))[alive.long()]
        sampled = alive[_multinomial_sample(probs, n, generator)].contiguous()
    else:
        sampled = _given(sampled_idxs, n, N, dev)
        is_dead = torch.zeros(N, device=dev, dtype=torch.bool)
        is_dead[dead.long()] = True
        if bool(is_dead[sampled.long()].any()):
            raise ValueError("sampled_idxs: a dead Gaussian cannot be a source")
    new_op, new_sc = mcmc_relocation(params["opacities"], params["scales"], sampled, min_opacity)

    def param_fn(name, t):
        mcmc_scatter(t, sampled, dead, new_op if name == "opacities" else new_sc if name == "scales" else None)
        return t

    def optimizer_fn(key, v):
        mcmc_zero_rows(v, sampled)
        return v

    _update_param_with_optimizer(param_fn, optimizer_fn, params, optimizers)
    for v in state.values():
        if isinstance(v, torch.Tensor) and v.dim() > 0 and v.shape[0] == N:
            mcmc_zero_rows(v, sampled)
    return n


@torch.no_grad()
def sample_add(params, optimizers, state: Dict[str, Any], n: int, min_opacity: float = 0.005, generator: Optional[torch.Generator] = None,
               sampled_idxs: Optional[torch.Tensor] = None) -> int:
    """ops.py:300-340: n new Gaussians, copies of sources drawn with probability proportional to their opacity, appended in the
    order of the draw; sources and copies share the opacity and scale of eq. 9.  Every parameter becomes a new tensor of N + n rows;
    the new rows' Adam moments are zero, nothing else is touched.  n == 0 leaves every object untouched."""
    n = int(n)
    if n <= 0:
        return 0
    _require(params)
    N = len(params["means"])
    dev = params["means"].device
    if sampled_idxs is None:
        sampled = _multinomial_sample(torch.sigmoid(params["opacities"].detach().reshape(-1)), n, generator).to(torch.int32)
    else:
        sampled = _given(sampled_idxs, n, N, dev)
    new_op, new_sc = mcmc_relocation(params["opacities"], params["scales"], sampled, min_opacity)
    dest = torch.arange(N, N + n, device=dev, dtype=torch.int32)

    def grown(t):
        out = torch.zeros((N + n, *t.shape[1:]), device=t.device, dtype=t.dtype)
        out[:N] = t
        return out

    def param_fn(name, t):
        out = grown(t)
        mcmc_scatter(out, sampled, dest, new_op if name == "opacities" else new_sc if name == "scales" else None)
        return out

    _update_param_with_optimizer(param_fn, lambda key, v: grown(v), params, optimizers)
    for k, v in state.items():
        if isinstance(v, torch.Tensor) and v.dim() > 0 and v.shape[0] == N:
            state[k] = grown(v)
    return n


@torch.no_grad()
def inject_noise_to_position(params, optimizers, state: Dict[str, Any], scaler: float, generator: Optional[torch.Generator] = None,
                             noise: Optional[torch.Tensor] = None) -> None:
    """ops.py:343-369: means += Sigma (noise * gate * scaler) in place, gate = 1 / (1 + exp(-100 ((1 - opacity) - 0.995))): only
    nearly transparent Gaussians move.  noise: [N,3] standard normal, drawn with torch.randn from generator when not given."""
    means = params["means"]
    if noise is None:
        gdev = generator.device if generator is not None else means.device
        noise = torch.randn(means.shape, generator=generator, device=gdev, dtype=torch.float32).to(means.device)
    mcmc_inject_noise(means.detach(), params["quats"].detach(), params["scales"].detach(), params["opacities"].detach(), noise, scaler)


@dataclass
class MCMCStrategy:
    """Field names and defaults: gsplat/strategy/mcmc.py:49-55."""
    cap_max: int = 1_000_000
    noise_lr: float = 5e5
    refine_start_iter: int = 500
    refine_stop_iter: int = 25_000
    refine_every: int = 100
    min_opacity: float = 0.005
    verbose: bool = False

    def initialize_state(self) -> Dict[str, Any]:
        """Empty: the reference keeps its 51 x 51 table of binomial coefficients here; wm_mcmc_relocation needs none (it evaluates
        the collapsed sum with the coefficients by recurrence)."""
        return {}

    def check_sanity(self, params, optimizers) -> None:
        trainable = set(name for name, p in params.items() if p.requires_grad)
        assert trainable == set(optimizers.keys()), f"trainable parameters and optimizers must have the same keys, got {trainable} and {set(optimizers.keys())}"
        for opt in optimizers.values():
            assert len(opt.param_groups) == 1, f"each optimizer must have exactly one param_group, got {len(opt.param_groups)}"
        for key in ("means", "scales", "quats", "opacities"):
            assert key in params, f"{key} is required in params but missing."

    def step_post_backward(self, params, optimizers, state, step: int, info: Dict[str, Any], lr: float,
                           generator: Optional[torch.Generator] = None) -> None:
        """lr: the learning rate of "means".  generator: for the multinomial draws and the position noise (on the parameters' device).
        Schedule of mcmc.py:122-145: at a refinement relocate, then add; the position noise every step."""
        if step < self.refine_stop_iter and step > self.refine_start_iter and step % self.refine_every == 0:
            n_relocated_gs = self._relocate_gs(params, optimizers, generator)
            if self.verbose:
                print(f"Step {step}: Relocated {n_relocated_gs} GSs.")
            n_new_gs = self._add_new_gs(params, optimizers, generator)
            if self.verbose:
                print(f"Step {step}: Added {n_new_gs} GSs. Now having {len(params['means'])} GSs.")
        inject_noise_to_position(params, optimizers, {}, lr * self.noise_lr, generator)

    def _relocate_gs(self, params, optimizers, generator=None) -> int:
        return relocate(params, optimizers, {}, None, self.min_opacity, generator)

    def _add_new_gs(self, params, optimizers, generator=None) -> int:
        current = len(params["means"])
        n_target = min(self.cap_max, int(1.05 * current))
        return sample_add(params, optimizers, {}, max(0, n_target - current), self.min_opacity, generator)
