"""gsplat's ``DefaultStrategy`` (gsplat/strategy/default.py, ops.py) — the adaptive density control the reference's "Post 3DGS
Optimization" trainer runs around every step (simple_trainer_worldmirror.py:776 ``step_pre_backward``, :961 ``step_post_backward``)
— over the HIP entries ``wm_densify_accumulate`` / ``wm_densify_plan`` / ``wm_densify_gather``.  Same field names and defaults, same
methods, same objects: ``params`` a dict / ``ParameterDict`` of ``[N, ...]`` parameters with ``means``, ``scales`` (log), ``quats``,
``opacities`` (logit) among them, ``optimizers`` a dict with one single-group optimiser per trainable key, ``info`` what
``Rasterizer.rasterize_splats(..., return_info=True)`` returns.  No CPU fallback: the tensors live on a HIP device.

Not built: packed (sparse) gradients, ``key_for_gradient`` other than ``"means2d"``."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Any, Dict, Optional, Tuple

import torch

from . import _lib
from ._lib import check, ptr, stream

KEEP, DUP, SPLIT0, SPLIT1 = 0, 1, 2, 3
GATHER_MODES = {"copy": 0, "zero_new": 1, "means": 2, "scales": 3, "opacities_revised": 4}


def _check(t, dtype, name):
    if t.device.type != "cuda" or t.dtype != dtype or not t.is_contiguous():
        raise RuntimeError(f"{name}: a contiguous {dtype} tensor on a HIP device is required (the densification runs in libwm_hip.so)")


def densify_accumulate(grads: torch.Tensor, radii: torch.Tensor, width: int, height: int, grad2d: torch.Tensor, count: torch.Tensor,
                       radii_state: Optional[torch.Tensor] = None) -> None:
    """_update_state (default.py:220-260), in place on grad2d / count / radii_state [N].  grads [C,N,2] fp32 (means2d.grad or
    .absgrad), radii [C,N,2] int32."""
    V, N = int(grads.shape[0]), int(grads.shape[1])
    _check(grads, torch.float32, "grads"); _check(radii, torch.int32, "radii")
    _check(grad2d, torch.float32, "grad2d"); _check(count, torch.float32, "count")
    if radii_state is not None:
        _check(radii_state, torch.float32, "radii_state")
    if tuple(radii.shape) != (V, N, 2) or grad2d.numel() != N or count.numel() != N or (radii_state is not None and radii_state.numel() != N):
        raise ValueError("shapes: grads / radii [C,N,2], grad2d / count / radii_state [N]")
    if N == 0:
        return
    st = _lib.lib().wm_densify_accumulate(ptr(grads), ptr(radii), N, V, int(width), int(height), ptr(grad2d), ptr(count), ptr(radii_state),
                                          stream(grads.device))
    check(st, "wm_densify_accumulate")


def densify_plan(grad2d, count, radii_state, scales, opacities, *, grow_grad2d, grow_scale3d, grow_scale2d, prune_opa, prune_scale3d,
                 prune_scale2d, use_scale2d, prune_big, revised_opacity) -> Dict[str, Any]:
    """_grow_gs + _prune_gs as one plan.  grow_scale3d / prune_scale3d: already multiplied by the scene scale.  -> dict with src,
    kind, rank (int32 [n_out] device tensors) and the ints n_dupli, n_split, n_prune, n_out, n_in.  Synchronises the stream once."""
    N = int(scales.shape[0])
    op = opacities.detach().reshape(-1)
    sc = scales.detach()
    for t, name in ((grad2d, "grad2d"), (count, "count"), (sc, "scales"), (op, "opacities")):
        _check(t, torch.float32, name)
    if radii_state is not None:
        _check(radii_state, torch.float32, "radii_state")
    if use_scale2d and radii_state is None:
        raise ValueError("the screen-size clauses need the radii state")
    dev = sc.device
    L = _lib.lib()
    rows = torch.empty((3, 3 * N), device=dev, dtype=torch.int32)
    ws = torch.empty(L.wm_densify_plan_workspace_bytes(N), device=dev, dtype=torch.uint8)
    counts = (C.c_int * 4)()
    st = L.wm_densify_plan(ptr(grad2d), ptr(count), ptr(radii_state), ptr(sc), ptr(op), N, grow_grad2d, grow_scale3d, grow_scale2d, prune_opa,
                           prune_scale3d, prune_scale2d, int(use_scale2d), int(prune_big), int(revised_opacity), ptr(rows[0]), ptr(rows[1]),
                           ptr(rows[2]), C.byref(counts), ptr(ws), ws.numel(), stream(dev))
    check(st, "wm_densify_plan")
    n_dupli, n_split, n_prune, n_out = (int(x) for x in counts)
    return {"src": rows[0, :n_out], "kind": rows[1, :n_out], "rank": rows[2, :n_out], "n_dupli": n_dupli, "n_split": n_split,
            "n_prune": n_prune, "n_out": n_out, "n_in": N}


def densify_gather(t: torch.Tensor, plan: Dict[str, Any], mode: str = "copy", quats=None, scales=None, noise=None) -> torch.Tensor:
    """[N, ...] fp32 -> [n_out, ...] by the plan.  mode: copy | zero_new (Adam moments) | means (needs quats [N,4], log scales
    [N,3], noise [2,N,3]) | scales | opacities_revised."""
    N, n_out = plan["n_in"], plan["n_out"]
    x = t.detach()
    _check(x, torch.float32, "tensor")
    if int(x.shape[0]) != N:
        raise ValueError(f"the plan was made for {N} rows, the tensor has {x.shape[0]}")
    R = x.numel() // N
    out = torch.empty((n_out, *x.shape[1:]), device=x.device, dtype=torch.float32)
    if mode == "means":
        quats, scales = quats.detach(), scales.detach()
        _check(quats, torch.float32, "quats"); _check(scales, torch.float32, "scales"); _check(noise, torch.float32, "noise")
        if tuple(noise.shape) != (2, N, 3):
            raise ValueError("noise: [2, N, 3]")
    else:
        quats = scales = noise = None
    st = _lib.lib().wm_densify_gather(ptr(x), ptr(out), N, R, GATHER_MODES[mode], ptr(plan["src"]), ptr(plan["kind"]), ptr(plan["rank"]), n_out,
                                      ptr(quats), ptr(scales), ptr(noise), stream(x.device))
    check(st, f"wm_densify_gather({mode})")
    return out


@dataclass
class DefaultStrategy:
    """Field names and defaults: gsplat/strategy/default.py:79-94."""
    prune_opa: float = 0.005
    grow_grad2d: float = 0.0002
    grow_scale3d: float = 0.01
    grow_scale2d: float = 0.05
    prune_scale3d: float = 0.1
    prune_scale2d: float = 0.15
    refine_scale2d_stop_iter: int = 0
    refine_start_iter: int = 500
    refine_stop_iter: int = 15_000
    reset_every: int = 3000
    refine_every: int = 100
    pause_refine_after_reset: int = 0
    absgrad: bool = False
    revised_opacity: bool = False
    verbose: bool = False
    key_for_gradient: str = "means2d"

    def initialize_state(self, scene_scale: float = 1.0) -> Dict[str, Any]:
        """grad2d: running sum of the 2-D mean gradient norms, count: how often each splat was seen, radii: largest normalised
        screen radius (only with refine_scale2d_stop_iter > 0).  Allocated at the first step, on the gradients' device."""
        state = {"grad2d": None, "count": None, "scene_scale": scene_scale}
        if self.refine_scale2d_stop_iter > 0:
            state["radii"] = None
        return state

    def check_sanity(self, params, optimizers) -> None:
        trainable = set(name for name, p in params.items() if p.requires_grad)
        assert trainable == set(optimizers.keys()), f"trainable parameters and optimizers must have the same keys, got {trainable} and {set(optimizers.keys())}"
        for opt in optimizers.values():
            assert len(opt.param_groups) == 1, f"each optimizer must have exactly one param_group, got {len(opt.param_groups)}"
        for key in ("means", "scales", "quats", "opacities"):
            assert key in params, f"{key} is required in params but missing."

    def _key(self) -> str:
        if self.key_for_gradient != "means2d":
            raise NotImplementedError('key_for_gradient: only "means2d" is built (no 2DGS)')
        return self.key_for_gradient

    def step_pre_backward(self, params, optimizers, state, step: int, info: Dict[str, Any]) -> None:
        key = self._key()
        assert key in info, "The 2D means of the Gaussians is required but missing."
        info[key].retain_grad()

    def step_post_backward(self, params, optimizers, state, step: int, info: Dict[str, Any], packed: bool = False,
                           generator: Optional[torch.Generator] = None) -> None:
        """generator: for the split noise (torch.randn(2, n_split, 3), the one random draw of a refinement)."""
        if packed:
            raise NotImplementedError("packed (sparse) gradients are not built: the layout is always [C,N,...]")
        self._key()
        if step >= self.refine_stop_iter:
            return
        self._update_state(params, state, info)
        if step > self.refine_start_iter and step % self.refine_every == 0 and step % self.reset_every >= self.pause_refine_after_reset:
            n_dupli, n_split, n_prune = self._refine(params, optimizers, state, step, generator)
            if self.verbose:
                print(f"Step {step}: {n_dupli} GSs duplicated, {n_split} GSs split, {n_prune} GSs pruned. "
                      f"Now having {len(params['means'])} GSs.")
        if step % self.reset_every == 0 and step > 0:
            reset_opa(params, optimizers, state, self.prune_opa * 2.0)

    def _update_state(self, params, state, info) -> None:
        key = self._key()
        for k in ("width", "height", "n_cameras", "radii", "gaussian_ids", key):
            assert k in info, f"{k} is required but missing."
        grads = info[key].absgrad if self.absgrad else info[key].grad
        if grads is None:
            raise RuntimeError("means2d has no gradient: call step_pre_backward before loss.backward()")
        n = len(next(iter(params.values())))
        dev = grads.device
        for k in ("grad2d", "count") + (("radii",) if self.refine_scale2d_stop_iter > 0 else ()):
            if state.get(k) is None:
                state[k] = torch.zeros(n, device=dev)
        densify_accumulate(grads.contiguous(), info["radii"], info["width"], info["height"], state["grad2d"], state["count"], state.get("radii"))

    @torch.no_grad()
    def _refine(self, params, optimizers, state, step: int, generator=None) -> Tuple[int, int, int]:
        if len(params["means"]) == 0:
            return 0, 0, 0
        scene = float(state["scene_scale"])
        use2d = step < self.refine_scale2d_stop_iter
        plan = densify_plan(state["grad2d"], state["count"], state.get("radii"), params["scales"].detach().contiguous(),
                            params["opacities"].detach().contiguous(), grow_grad2d=self.grow_grad2d, grow_scale3d=self.grow_scale3d * scene,
                            grow_scale2d=self.grow_scale2d, prune_opa=self.prune_opa, prune_scale3d=self.prune_scale3d * scene,
                            prune_scale2d=self.prune_scale2d, use_scale2d=use2d, prune_big=step > self.reset_every,
                            revised_opacity=self.revised_opacity)
        n_dupli, n_split, n_prune = plan["n_dupli"], plan["n_split"], plan["n_prune"]
        if n_dupli or n_split or n_prune:
            apply_plan(params, optimizers, plan, self.revised_opacity, generator)
        n = len(params["means"])
        for k, v in state.items():
            if isinstance(v, torch.Tensor):
                state[k] = torch.zeros(n, device=v.device) if n != v.numel() else v.zero_()
        return n_dupli, n_split, n_prune


@torch.no_grad()
def apply_plan(params, optimizers, plan, revised_opacity: bool = False, generator: Optional[torch.Generator] = None) -> None:
    """duplicate -> split -> remove (ops.py:93-210) in one pass per tensor: every parameter becomes a new nn.Parameter of the new
    length, and each optimiser's param group and state follow it (_update_param_with_optimizer, ops.py:48-89): tensor states are
    gathered with new rows zero, "step" is kept."""
    N, n_split = plan["n_in"], plan["n_split"]
    dev = params["means"].device
    old = {k: p.detach().contiguous() for k, p in params.items()}
    noise = None
    if n_split > 0:
        noise = torch.empty((2, N, 3), device=dev, dtype=torch.float32)
        gdev = generator.device if generator is not None else dev
        noise[:, :n_split] = torch.randn(2, n_split, 3, generator=generator, device=gdev).to(dev)
    for name in list(params.keys()):
        p = params[name]
        if name == "means" and n_split > 0:
            new = densify_gather(old[name], plan, "means", old["quats"], old["scales"], noise)
        elif name == "scales":
            new = densify_gather(old[name], plan, "scales")
        elif name == "opacities" and revised_opacity:
            new = densify_gather(old[name], plan, "opacities_revised")
        else:
            new = densify_gather(old[name], plan, "copy")
        new_p = torch.nn.Parameter(new, requires_grad=p.requires_grad)
        params[name] = new_p
        if name not in optimizers:
            assert not p.requires_grad, f"Optimizer for {name} is not found, but the parameter is trainable."
            continue
        opt = optimizers[name]
        for group in opt.param_groups:
            st = opt.state.pop(p, {})
            for key, v in st.items():
                if key != "step" and isinstance(v, torch.Tensor) and v.dim() > 0 and v.shape[0] == N:
                    st[key] = densify_gather(v.contiguous(), plan, "zero_new")
            group["params"] = [new_p]
            opt.state[new_p] = st


@torch.no_grad()
def reset_opa(params, optimizers, state, value: float) -> None:
    """ops.py:214-241: clamp the (logit) opacities to at most logit(value) and zero their optimiser moments.  Plain torch: one
    clamp, every reset_every steps."""
    p = params["opacities"]
    new_p = torch.nn.Parameter(torch.clamp(p, max=torch.logit(torch.tensor(value)).item()), requires_grad=p.requires_grad)
    params["opacities"] = new_p
    if "opacities" not in optimizers:
        return
    opt = optimizers["opacities"]
    for group in opt.param_groups:
        st = opt.state.pop(p, {})
        for key, v in st.items():
            if key != "step":
                st[key] = torch.zeros_like(v)
        group["params"] = [new_p]
        opt.state[new_p] = st
