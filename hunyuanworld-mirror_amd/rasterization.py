"""Host-side mirror of the reference's ``Rasterizer`` (src/models/models/rasterization.py:17-93) over the C ABI entries
``wm_rasterize_splats_opt`` / ``wm_rasterize_splats_backward_opt`` (hand-written HIP: projection, tile binning, radix sort, tile
compositing).  Same method names, argument order and return triples, so ``model.gs_renderer.rasterizer.rasterize_batches(...)`` as
called by ``render_interpolated_video`` (src/utils/render_utils.py:242-312) and ``GaussianSplatRenderer.render``
(rasterization.py:221-241) keeps working.  No CPU fallback: tensors must live on a HIP device.

Differentiable: when autograd is recording and any of means / quats / scales / opacities / colors requires grad, ``.backward()`` is
one ``wm_rasterize_splats_backward_opt`` call (what gsplat's CUDA extension gives the reference's post-3DGS
optimisation).  No packed / sparse gradients.

Cameras: by default ``camtoworlds`` and ``Ks`` get no gradient (``None``).  ``Rasterizer(camera_grad=True)`` makes ``camtoworlds``
differentiable (gsplat: the ``viewmats`` gradient of ``_FullyFusedProjection``, which the reference trainer's ``--pose_opt`` trains a
pose.CameraOptModule on): the inverse ``viewmats = inv(camtoworlds)`` is then taken once in the graph, the kernels see its values,
the backward call returns the gradient of the rendered images with respect to ``viewmats`` and torch's own inverse
backward carries it on to ``camtoworlds`` and whatever produced it.  It works on both routes and when no splat tensor requires grad
(pose-only refinement); forward outputs are the same bits either way.  ``Ks`` gets ``None`` in every case, as in gsplat.

View-dependent colour: ``colors [N,K,3]`` with ``sh_degree`` 1-3, ``(sh_degree + 1)^2 <= K`` (gsplat/rendering.py:509-525; the reference
trainer raises ``sh_degree_to_use`` while it trains, simple_trainer_worldmirror.py:613, :738-746), works on every route.  The colour of
a (camera, Gaussian) pair is evaluated along ``means - campos``, ``campos = camtoworlds[:, :3, 3]`` (gsplat's
``inverse(viewmats)[:, :3, 3]``); ``colors.grad`` has the full ``[N,K,3]`` shape with exact zeros in the bands at or above
``(sh_degree + 1)^2``, ``means.grad`` includes the direction's term, and with ``camera_grad`` ``campos`` is a second graph tensor beside
``viewmats``, so that ``camtoworlds.grad`` is the sum of both.  ``sh_degree`` 0 and ``None`` go as before.

Per-camera colours: ``colors [C,N,3]`` with ``sh_degree=None`` (post-activation colours with a camera axis, as the reference trainer's
``--app_opt`` passes them: ``sigmoid(app_module(...) + colors)``, simple_trainer_worldmirror.py:603-611) render pair (c, g) with
``colors[c, g]`` as it is, on every route (``colors_are_sh0 = WM_COLORS_PER_CAMERA``); ``colors.grad`` is
``[C,N,3]`` with exact zeros where a camera culled the Gaussian.  A leading size other than the number of cameras is a ``ValueError``.

``rasterize_splats(..., return_info=True)`` also returns what gsplat.rasterization's ``info`` gives a densification strategy
(strategy.DefaultStrategy): the projected ``means2d`` as part of the graph, so that ``retain_grad()`` works and ``.grad`` (and,
with absgrad, the plain attribute ``.absgrad``) is there after ``loss.backward()``, and the per-(camera, Gaussian) ``radii``.
``means2d`` receives gradient from the rendered images only; unlike gsplat's, it does not pass gradient on to the splats, so a loss
computed from ``means2d`` itself raises ``NotImplementedError`` in ``backward()`` rather than being dropped.

gsplat's own call: the module-level ``rasterization(...)`` has gsplat.rasterization's signature and ``(render_colors, render_alphas, info)``
return (gsplat/rendering.py), as the reference's post-3DGS trainer calls it (simple_trainer_worldmirror.py:619-642, :741-752): world-to-camera
``viewmats`` (differentiable where they require grad), ``render_mode`` "RGB" | "D" | "ED" | "RGB+D" | "RGB+ED", ``rasterize_mode`` "classic" |
"antialiased", ``near_plane``, ``far_plane``, ``eps2d``, ``radius_clip`` and differentiable ``backgrounds [C,3]``.  These options travel as one
``wm_raster_options`` struct (an ``_Opts`` here) on every call.  ``Rasterizer`` takes
``rasterization_mode="antialiased"`` and the same keywords except ``render_mode`` (its triple stays rgb, expected depth, alpha, as in the
reference class); what is not given takes gsplat's default value.  Every call of either surface goes through the ``_opt`` pair: the C ABI
keeps its older entries without options as wrappers around that pair, which give the same bits.  What the kernels do not do (packed,
sparse_grad, distributed, tile_size != 16, non-pinhole cameras, with_ut, with_eval3d, colour channels other than 3, unknown keywords)
raises ``NotImplementedError`` naming the argument."""
from __future__ import annotations

import collections
import ctypes as C
import weakref
import torch

from . import _lib
from ._lib import check, ptr, stream


def _f32(t: torch.Tensor) -> torch.Tensor:
    return t.detach().to(torch.float32).contiguous()


class _RasterizeSplats(torch.autograd.Function):
    """rasterize_splats with a backward (gsplat: _wrapper.py _RasterizeToPixels / _FullyFusedProjection / _QuatScaleToCovarPreci
    .backward).  The node owns the forward's workspace: a later rasterize_splats call cannot disturb it before .backward()."""

    @staticmethod
    def forward(ctx, rz, is_sh, width, height, camtoworlds, Ks, means, quats, scales, opacities, colors, viewmats, campos, sh_degree, opts,
                backgrounds):
        # viewmats: None, or with camera_grad inv(camtoworlds) as a graph tensor: the input that receives the camera gradient;
        # campos: None, or with camera_grad and sh_degree > 0 the camera positions as a graph tensor: receives the colour's camera term
        # opts: the _Opts of the call; backgrounds: None or [C,3], receives its gradient
        rgb, depth, alpha, state = rz._forward(means, quats, scales, opacities, _cin(colors, is_sh, sh_degree), is_sh, camtoworlds, Ks, width, height,
                                               own_workspace=True, viewmats=viewmats, sh_degree=sh_degree, campos=campos, opts=opts,
                                               backgrounds=backgrounds)
        ctx.state, ctx.geom = state, (is_sh, width, height)
        _keep(ctx, (means, quats, scales, opacities, colors), backgrounds, depth, alpha)
        return rgb, depth, alpha

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, v_rgb, v_depth, v_alpha):
        grads, _, _, v_vm, v_cp, v_bg = _node_backward(ctx, (v_rgb, v_depth, v_alpha), False, False, first=6)
        # camtoworlds, Ks: no gradient of their own (camtoworlds gets its through viewmats and campos)
        return (None, None, None, None, None, None, *grads, v_vm, v_cp, None, None, v_bg)


def _keep(ctx, splat_in, backgrounds, depth, alpha):
    """what a node's backward needs beside ctx.state and ctx.geom: the shapes and dtypes its gradients go back in, and the forward outputs
    the backward call reads"""
    ctx.meta = [(t.shape, t.dtype) for t in splat_in]
    ctx.bg_meta = None if backgrounds is None else (backgrounds.shape, backgrounds.dtype)
    if backgrounds is None:
        ctx.save_for_backward(depth)     # the one forward output the backward reads
    else:
        ctx.save_for_backward(depth, alpha)     # v_backgrounds reads the forward's alpha


def _node_backward(ctx, cotangents, want_means2d, want_absgrad, first):
    """_backward for a node whose inputs are ..., means, quats, scales, opacities, colors, viewmats, campos, ..., backgrounds with means at
    index `first` -> the five splat gradients and v_backgrounds in their inputs' shapes and dtypes, the rest as _backward returns it"""
    depth, alpha = (*ctx.saved_tensors, None)[:2]
    need = ctx.needs_input_grad
    grads, v2d, v2d_abs, v_vm, v_cp, v_bg = _backward(ctx.state, depth, ctx.geom, cotangents, want_means2d, want_absgrad, need[first + 5],
                                                      need[first + 6], ctx.bg_meta is not None and need[-1], alpha)
    grads = _shape_grads(grads, ctx.meta, ctx.geom[0] == 1 and not ctx.state.sh_degree, need[first:first + 5])
    return grads, v2d, v2d_abs, v_vm, v_cp, _shape_bg(v_bg, ctx.bg_meta)


def _cin(colors, is_sh, sh_degree):
    """what the kernels read: all of the SH coefficients [N,K,3] for sh_degree 1-3, band 0 for degree 0, the colours [N,3] otherwise"""
    return colors[:, 0, :] if is_sh == 1 and not sh_degree else colors


# what _forward hands to _backward and _means2d: its fp32 inputs, the workspace it filled and the pair capacity / count of that workspace
_State = collections.namedtuple("_State", "means quats scales opacities cin viewmats Ks ws cap n sh_degree campos opts backgrounds")


def _backward(state, depth, geom, cotangents, want_means2d, want_absgrad, want_cam=False, want_campos=False, want_bg=False, alpha=None):
    """One fused wm_rasterize_splats_backward_opt call -> [g_means, g_quats, g_scales, g_opacities, g_colors], v_means2d, v_means2d_abs,
    v_viewmats, v_campos, v_backgrounds (each None unless asked for): g_colors is [N,K,3] for SH degree 1-3, v_viewmats [C,4,4] the gradient
    of the world-to-camera matrices, v_campos [C,3] that of the camera positions (SH degree 1-3 only), and v_backgrounds [C,3] reads the
    forward's alpha.  The five splat gradients are the same bits whatever else is asked for."""
    L, s = _lib.lib(), state
    is_sh, width, height = geom
    dev = s.means.device
    N, V = int(s.means.shape[0]), int(s.viewmats.shape[0])
    cot = [torch.zeros((V, height, width, ch), device=dev) if v is None else _f32(v) for v, ch in zip(cotangents, (3, 1, 1))]
    grads = [torch.empty_like(t) for t in (s.means, s.quats, s.scales, s.opacities, s.cin)]
    want_absgrad = bool(want_means2d and want_absgrad)
    f32 = dict(device=dev, dtype=torch.float32)
    v2d = torch.empty((V, N, 2), **f32) if want_means2d else None
    v2d_abs = torch.empty((V, N, 2), **f32) if want_absgrad else None
    v_vm = torch.empty((V, 4, 4), **f32) if want_cam else None
    v_cp = torch.empty((V, 3), **f32) if want_campos and s.sh_degree else None
    v_bg = torch.empty((V, 3), **f32) if want_bg and s.backgrounds is not None else None
    gws = torch.empty(L.wm_rasterize_backward_workspace_bytes_opt(N, V, width, height, s.n, int(want_absgrad), int(v_vm is not None), s.sh_degree,
                                                                  int(v_cp is not None), int(v_bg is not None)), device=dev, dtype=torch.uint8)
    st = L.wm_rasterize_splats_backward_opt(ptr(s.means), ptr(s.quats), ptr(s.scales), ptr(s.opacities), ptr(s.cin), is_sh,
                                            int(s.cin.shape[1]) if s.sh_degree else 0, s.sh_degree, ptr(s.campos) if s.sh_degree else None, N,
                                            ptr(s.viewmats), ptr(s.Ks), V, width, height, C.byref(s.opts.struct(s.backgrounds)), ptr(s.ws),
                                            s.ws.numel(), s.cap, s.n, None, ptr(depth), None if v_bg is None else ptr(_f32(alpha)),
                                            ptr(cot[0]), ptr(cot[1]), ptr(cot[2]), *(ptr(g) for g in grads), ptr(v2d), ptr(v2d_abs),
                                            int(want_absgrad), ptr(v_vm), ptr(v_cp), ptr(v_bg), ptr(gws), gws.numel(), stream(dev))
    check(st, "wm_rasterize_splats_backward")
    return grads, v2d, v2d_abs, v_vm, v_cp, v_bg


def _shape_bg(v_bg, meta):
    return None if v_bg is None else v_bg.reshape(meta[0]).to(meta[1])


def _shape_grads(grads, meta, is_sh, needed):
    out = []
    for i, (g, (shape, dtype)) in enumerate(zip(grads, meta)):
        if not needed[i]:
            out.append(None)
            continue
        if i == 4 and is_sh:     # SH coefficients [N, K, 3] of which only degree 0 is rendered (is_sh here: degree 0)
            full = torch.zeros(shape, device=g.device, dtype=torch.float32)
            full[:, 0, :] = g
            g = full
        out.append(g.reshape(shape).to(dtype))
    return out


class _ProjectMeans2d(torch.autograd.Function):
    """First half of the return_info route: runs the forward, keeps what it made in `shared` and returns the projected means
    [C,N,2] as a graph tensor (gsplat: the means2d output of _FullyFusedProjection).  Its own backward passes nothing on: the
    parameter gradients all come from the one fused backward of _CompositeWithInfo, so nothing is counted twice."""

    @staticmethod
    def forward(ctx, rz, shared, is_sh, width, height, camtoworlds, Ks, means, quats, scales, opacities, colors, viewmats, campos, sh_degree,
                opts, backgrounds):
        radii = torch.empty((int((viewmats if camtoworlds is None else camtoworlds).shape[0]), int(means.shape[0]), 2), device=means.device,
                            dtype=torch.int32)
        rgb, depth, alpha, state = rz._forward(means, quats, scales, opacities, _cin(colors, is_sh, sh_degree), is_sh, camtoworlds, Ks, width, height,
                                               own_workspace=True, radii=radii, viewmats=viewmats, sh_degree=sh_degree, campos=campos, opts=opts,
                                               backgrounds=backgrounds)
        shared.update(out=(rgb, depth, alpha), state=state, radii=radii)
        ctx.shared = shared
        m2 = rz._means2d(state, radii, width, height)
        return m2

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, v_means2d):
        # what arrives here must be exactly what _CompositeWithInfo.backward handed to means2d.  Anything else is a loss that used
        # means2d itself: gsplat would carry that on to the parameters, this route does not, so it refuses instead of dropping it.
        sent = ctx.shared.get("v_means2d")
        if sent is None or not (v_means2d.data_ptr() == sent.data_ptr() or torch.equal(v_means2d, sent)):
            raise NotImplementedError("info['means2d'] carries gradient only from the rendered images to itself (.grad / .absgrad for a "
                                      "densification strategy): a loss computed from means2d directly is not propagated to the splats")
        return (None,) * 17


class _CompositeWithInfo(torch.autograd.Function):
    """Second half: hands out the images of the forward _ProjectMeans2d ran, with means2d as an input.  Its backward is the one
    fused backward call: the five parameter gradients, and v_means2d as the gradient of the means2d input (-> means2d.grad
    under retain_grad()); with absgrad, means2d.absgrad is set as a plain attribute, as gsplat's _RasterizeToPixels.backward does.
    viewmats (None, or with camera_grad the graph's inv(camtoworlds)) receives the camera gradient of the same call, campos (None, or with
    camera_grad and SH degree 1-3 the graph's camera positions) the colour's camera term."""

    @staticmethod
    def forward(ctx, shared, geom, want_absgrad, means2d, means, quats, scales, opacities, colors, viewmats, campos, backgrounds):
        rgb, depth, alpha = shared.pop("out")
        ctx.state, ctx.geom, ctx.want_absgrad = shared.pop("state"), geom, want_absgrad
        ctx.means2d_ref, ctx.shared = shared["means2d_ref"], shared
        _keep(ctx, (means, quats, scales, opacities, colors), backgrounds, depth, alpha)
        return rgb, depth, alpha

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, v_rgb, v_depth, v_alpha):
        grads, v2d, v2d_abs, v_vm, v_cp, v_bg = _node_backward(ctx, (v_rgb, v_depth, v_alpha), True, ctx.want_absgrad, first=4)
        m2 = ctx.means2d_ref()
        if ctx.want_absgrad and m2 is not None:
            m2.absgrad = v2d_abs
        ctx.shared["v_means2d"] = v2d
        return (None, None, None, v2d, *grads, v_vm, v_cp, v_bg)


class _Opts(collections.namedtuple("_Opts", "antialiased depth_mode eps2d near_plane far_plane radius_clip")):
    """gsplat.rasterization's options as the _opt entries take them (include/wm_hip.h wm_raster_options); backgrounds travel beside it"""
    __slots__ = ()

    def struct(self, backgrounds=None):
        return _lib.wm_raster_options(int(self.antialiased), int(self.depth_mode), float(self.eps2d), float(self.near_plane), float(self.far_plane),
                                      float(self.radius_clip), None if backgrounds is None else backgrounds.data_ptr())


PER_CAMERA = 2     # include/wm_hip.h WM_COLORS_PER_CAMERA


def _per_camera(colors, V, N):
    """colors [C,N,3] with sh_degree None: one post-activation colour per (camera, Gaussian); sh_degree is None, so it is never SH"""
    if tuple(colors.shape) != (V, N, 3):
        raise ValueError(f"per-camera colors must be [C, N, 3] = [{V}, {N}, 3], not {tuple(colors.shape)}")
    return colors


_OPTION_DEFAULTS = dict(near_plane=0.01, far_plane=1e10, eps2d=0.3, radius_clip=0.0)


class Rasterizer:
    def __init__(self, rasterization_mode="classic", packed=True, abs_grad=True, with_eval3d=False, camera_model="pinhole",
                 sparse_grad=False, distributed=False, grad_strategy=None, camera_grad: bool = False):
        """camera_grad: give a camtoworlds that requires grad its gradient (through viewmats = inv(camtoworlds), taken in the graph);
        off by default: cameras then get None.  Ks never gets a gradient (as in gsplat)."""
        if rasterization_mode not in ("classic", "antialiased") or camera_model != "pinhole" or with_eval3d or distributed:
            raise NotImplementedError("only the reference's configuration is built: classic or antialiased / pinhole / no eval3d / single process")
        self.rasterization_mode, self.packed, self.abs_grad, self.camera_model = rasterization_mode, packed, abs_grad, camera_model
        self.sparse_grad, self.grad_strategy, self.distributed, self.with_eval3d = sparse_grad, grad_strategy, distributed, with_eval3d
        self.camera_grad = bool(camera_grad)
        self._ws = None          # reusable workspace (torch uint8 tensor) and the pair capacity it was sized for
        self._cap = 0
        self.last_n_isects = 0

    # rasterization.py:29-66
    def rasterize_splats(self, means, quats, scales, opacities, colors, camtoworlds, Ks, width: int, height: int,
                         sh_degree=None, return_info: bool = False, absgrad: bool | None = None, near_plane=None, far_plane=None, eps2d=None,
                         radius_clip=None, backgrounds=None, **kwargs):
        """-> (rgb, depth, alpha), or with return_info=True (rgb, depth, alpha, info): info["means2d"] [C,N,2] fp32 (zero where
        culled, part of the graph), info["radii"] [C,N,2] int32, "width", "height", "n_cameras", "gaussian_ids" = None (the layout
        is always the unpacked [C,N,...] one).  absgrad (None: self.abs_grad) is read on the return_info route only.
        near_plane / far_plane / eps2d / radius_clip (gsplat's defaults 0.01 / 1e10 / 0.3 / 0) and backgrounds [C,3] (differentiable) are
        gsplat.rasterization's; depth stays the expected depth (the reference class hard-wires render_mode "RGB+ED", so render_mode here is a
        TypeError as it is there).  They reach the kernels as an _Opts on every call, given or not."""
        if kwargs:
            raise TypeError(f"unsupported gsplat.rasterization arguments: {sorted(kwargs)}")
        given = dict(near_plane=near_plane, far_plane=far_plane, eps2d=eps2d, radius_clip=radius_clip)
        opts = _Opts(int(self.rasterization_mode == "antialiased"), 0, **{k: _OPTION_DEFAULTS[k] if v is None else float(v) for k, v in given.items()})
        if means.device.type != "cuda":
            raise RuntimeError("the rasteriser runs in libwm_hip.so on the GPU: move the splats to a HIP device")
        L = 0
        if colors.dim() == 3 and sh_degree is None:      # post-activation colours per camera [C, N, 3]
            cin, is_sh = _per_camera(colors, int(camtoworlds.shape[0]), int(means.shape[0])), PER_CAMERA
        elif colors.dim() == 3:          # SH coefficients [N, K, 3]
            if sh_degree is None or not 0 <= int(sh_degree) <= 3:
                raise NotImplementedError(f"SH degrees 0 to 3 are built, not sh_degree = {sh_degree}")
            L, K = int(sh_degree), int(colors.shape[1])
            if (L + 1) ** 2 > K:
                raise ValueError(f"sh_degree = {L} reads {(L + 1) ** 2} bands, colors has K = {K}")
            cin, is_sh = _cin(colors, 1, L), 1
        else:                            # post-activation colours [N, 3]
            if sh_degree is not None:
                raise ValueError("colors [N, 3] go with sh_degree = None")
            cin, is_sh = colors, 0
        splat_in = (means, quats, scales, opacities, colors)
        if return_info:
            return self._with_info(splat_in, cin, is_sh, camtoworlds, Ks, int(width), int(height), self.abs_grad if absgrad is None else absgrad, L,
                                   opts=opts, backgrounds=backgrounds)
        if absgrad:
            raise ValueError("absgrad is reported through info: pass return_info=True")
        viewmats, campos = self._graph_viewmats(camtoworlds), None
        if viewmats is not None and L:
            campos = camtoworlds.to(torch.float32)[:, :3, 3]
        return self._render(splat_in, cin, is_sh, camtoworlds, Ks, int(width), int(height), L, viewmats, campos, opts, backgrounds)

    def _render(self, splat_in, cin, is_sh, camtoworlds, Ks, width, height, L, viewmats, campos, opts, backgrounds):
        """the route without info.  viewmats / campos: None, or graph tensors (with camtoworlds = None: the cameras themselves)"""
        if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (*splat_in, viewmats, campos, backgrounds)):
            return _RasterizeSplats.apply(self, is_sh, width, height, camtoworlds, Ks, *splat_in, viewmats, campos, L, opts, backgrounds)
        rgb, depth, alpha, _ = self._forward(*splat_in[:4], cin, is_sh, camtoworlds, Ks, width, height, own_workspace=False,
                                             viewmats=None if camtoworlds is not None else viewmats, sh_degree=L,
                                             campos=None if camtoworlds is not None else campos, opts=opts, backgrounds=backgrounds)
        return rgb, depth, alpha

    def _graph_viewmats(self, camtoworlds):
        """with camera_grad, autograd recording and a camtoworlds that requires grad: inv(camtoworlds) as part of the graph; else None"""
        if self.camera_grad and torch.is_grad_enabled() and camtoworlds.requires_grad:
            return torch.linalg.inv(camtoworlds.to(torch.float32))
        return None

    def _with_info(self, splat_in, cin, is_sh, camtoworlds, Ks, width, height, want_absgrad, sh_degree, opts, backgrounds=None, cameras=None):
        """cameras: None (camtoworlds given), or (viewmats, campos) with camtoworlds = None: the world-to-camera matrices themselves and, for SH
        degree 1-3, the camera positions, graph tensors where they require grad (the module-level rasterization())"""
        if cameras is None:
            viewmats, campos = self._graph_viewmats(camtoworlds), None
            if viewmats is not None and sh_degree:
                campos = camtoworlds.to(torch.float32)[:, :3, 3]
        else:
            viewmats, campos = cameras
        V, N = int((viewmats if camtoworlds is None else camtoworlds).shape[0]), int(splat_in[0].shape[0])
        if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (*splat_in, viewmats, campos, backgrounds)):
            shared = {}
            m2 = _ProjectMeans2d.apply(self, shared, is_sh, width, height, camtoworlds, Ks, *splat_in, viewmats, campos, sh_degree, opts, backgrounds)
            shared["means2d_ref"] = weakref.ref(m2)
            radii = shared.pop("radii")
            rgb, depth, alpha = _CompositeWithInfo.apply(shared, (is_sh, width, height), bool(want_absgrad), m2, *splat_in, viewmats, campos,
                                                         backgrounds)
        else:
            radii = torch.empty((V, N, 2), device=splat_in[0].device, dtype=torch.int32)
            rgb, depth, alpha, state = self._forward(*splat_in[:4], cin, is_sh, camtoworlds, Ks, width, height, own_workspace=False, radii=radii,
                                                     viewmats=None if camtoworlds is not None else viewmats, sh_degree=sh_degree,
                                                     campos=None if camtoworlds is not None else campos, opts=opts, backgrounds=backgrounds)
            m2 = self._means2d(state, radii, width, height)
        info = {"means2d": m2, "radii": radii, "width": width, "height": height, "n_cameras": V, "gaussian_ids": None}
        return rgb, depth, alpha, info

    @staticmethod
    def _means2d(state, radii, width, height):
        """the pixel-space means of the forward that left `state`, [C,N,2], zero where culled"""
        N, V = int(state.means.shape[0]), int(state.viewmats.shape[0])
        m2 = torch.empty((V, N, 2), device=state.means.device, dtype=torch.float32)
        st = _lib.lib().wm_rasterize_means2d(ptr(state.ws), state.ws.numel(), N, V, width, height, state.cap, ptr(radii), ptr(m2),
                                             stream(state.means.device))
        check(st, "wm_rasterize_means2d")
        return m2

    def _forward(self, means, quats, scales, opacities, cin, is_sh, camtoworlds, Ks, width, height, own_workspace, opts, radii=None, viewmats=None,
                 sh_degree=0, campos=None, backgrounds=None):
        """One wm_rasterize_splats_opt call.  cin: the colours [N,3] or [C,N,3], or for sh_degree 1-3 the coefficients [N,K,3]; opts: the
        _Opts of the call; backgrounds: [C,3] or None; camtoworlds may be None when viewmats, and for SH degree 1-3 campos, are given.
        own_workspace: a workspace of this call's own (kept by the autograd node until its backward has run) instead of the rasteriser's
        reusable one.  radii: optional [C,N,2] int32 output.  viewmats, campos: the inverse of camtoworlds and its translation column where
        the caller has taken them already (camera_grad); their values are used, detached.
        -> rgb, depth, alpha, the _State for the backward."""
        L = _lib.lib()
        dev = means.device
        N, V = int(means.shape[0]), int((viewmats if camtoworlds is None else camtoworlds).shape[0])
        means, quats, scales, opacities, cin = _f32(means), _f32(quats), _f32(scales), _f32(opacities).reshape(-1), _f32(cin)
        if backgrounds is not None:
            if tuple(backgrounds.shape) != (V, 3):
                raise ValueError(f"backgrounds must be [C, 3] = [{V}, 3], not {tuple(backgrounds.shape)}")
            backgrounds = _f32(backgrounds)
        viewmats = _f32(torch.linalg.inv(camtoworlds.detach().to(torch.float32)) if viewmats is None else viewmats)  # :48
        Ks = _f32(Ks)
        if sh_degree:
            campos = _f32(camtoworlds[:, :3, 3] if campos is None else campos)
        rgb = torch.empty((V, height, width, 3), device=dev, dtype=torch.float32)
        depth = torch.empty((V, height, width, 1), device=dev, dtype=torch.float32)
        alpha = torch.empty((V, height, width, 1), device=dev, dtype=torch.float32)
        cap = max(self._cap, 8 * N * V, 1 << 16)
        n = C.c_ulonglong(0)
        ws = None if own_workspace else self._ws
        for _ in range(2):
            need = L.wm_rasterize_workspace_bytes(N, V, width, height, cap)
            if ws is None or ws.numel() < need or ws.device != dev:
                ws = torch.empty(need, device=dev, dtype=torch.uint8)
            if not own_workspace:
                self._ws = ws
            self._cap = cap
            st = L.wm_rasterize_splats_opt(ptr(means), ptr(quats), ptr(scales), ptr(opacities), ptr(cin), is_sh, int(cin.shape[1]) if sh_degree else 0,
                                           sh_degree, ptr(campos) if sh_degree else None, N, ptr(viewmats), ptr(Ks), V, width, height,
                                           C.byref(opts.struct(backgrounds)), ptr(rgb), ptr(depth), ptr(alpha), ptr(radii), ptr(ws), ws.numel(), cap,
                                           C.byref(n), stream(dev))
            if st == 0:
                break
            if st == 3 and n.value > cap:   # WM_ERR_STATE: more (Gaussian, tile) pairs than the workspace holds
                cap = int(n.value * 1.25) + 1024
                continue
            raise RuntimeError(f"wm_rasterize_splats failed with status {st}")
        else:
            raise RuntimeError("wm_rasterize_splats: workspace re-size did not converge")
        self.last_n_isects = int(n.value)
        return rgb, depth, alpha, _State(means, quats, scales, opacities, cin, viewmats, Ks, ws, cap, int(n.value), int(sh_degree), campos, opts,
                                         backgrounds)

    # rasterization.py:68-93 (NB: the reference passes what it calls `viewmats` on as `camtoworlds`)
    def rasterize_batches(self, means, quats, scales, opacities, colors, viewmats, Ks, width, height, **kwargs):
        if kwargs.get("return_info") or kwargs.get("absgrad"):
            raise TypeError("rasterize_batches returns the stacked (rgb, depth, alpha) only: call rasterize_splats(..., return_info=True) per batch element")
        rc, rd, ra = [], [], []
        for i in range(len(means)):
            c, d, a = self.rasterize_splats(means[i], quats[i], scales[i], opacities[i], colors[i], viewmats[i], Ks[i], width, height, **kwargs)
            rc.append(c); rd.append(d); ra.append(a)
        return torch.stack(rc, 0), torch.stack(rd, 0), torch.stack(ra, 0)


_RENDER_MODES = {"RGB": (True, None), "D": (False, 1), "ED": (False, 0), "RGB+D": (True, 1), "RGB+ED": (True, 0)}   # colour?, depth_mode
_shared = None


def rasterization(means, quats, scales, opacities, colors, viewmats, Ks, width, height, near_plane=0.01, far_plane=1e10, radius_clip=0.0,
                  eps2d=0.3, sh_degree=None, packed=False, tile_size=16, backgrounds=None, render_mode="RGB", sparse_grad=False, absgrad=False,
                  rasterize_mode="classic", channel_chunk=32, distributed=False, camera_model="pinhole", segmented=False, covars=None,
                  with_ut=False, with_eval3d=False, **unsupported):
    """gsplat.rasterization (gsplat/rendering.py) as the reference's post-3DGS trainer calls it (simple_trainer_worldmirror.py:619-642):
    -> (render_colors [C,H,W,3 | 1 | 4], render_alphas [C,H,W,1], info).  viewmats [C,4,4] are WORLD-TO-CAMERA, as in gsplat; a viewmats
    that requires grad receives the camera gradient directly and, with sh_degree > 0, also through campos = inv(viewmats)[:, :3, 3], taken
    in the graph.  colors: [N,3] or per-camera [C,N,3] with sh_degree None, or SH coefficients [N,K,3] with sh_degree 0-3.  render_mode: "RGB", "D" (accumulated
    depth), "ED" (expected depth), "RGB+D", "RGB+ED"; backgrounds [C,3] (differentiable) reach the colour channels only.  info is that of
    Rasterizer.rasterize_splats(return_info=True): means2d (with .grad, and .absgrad with absgrad=True, after backward), radii, width,
    height, n_cameras, gaussian_ids = None.  Whatever the kernels do not do raises NotImplementedError naming the argument."""
    global _shared
    for name, bad in (("packed", packed), ("sparse_grad", sparse_grad), ("distributed", distributed), ("with_ut", with_ut),
                      ("with_eval3d", with_eval3d), ("segmented", segmented), ("covars", covars is not None),
                      ("tile_size", tile_size != 16), ("camera_model", camera_model != "pinhole"),
                      ("rasterize_mode", rasterize_mode not in ("classic", "antialiased")), ("render_mode", render_mode not in _RENDER_MODES)):
        if bad:
            raise NotImplementedError(f"rasterization(): {name} = {locals()[name]!r} is not built")
    if unsupported:
        raise NotImplementedError(f"rasterization(): arguments not built: {sorted(unsupported)}")
    per_camera = sh_degree is None and colors.dim() == 3 and colors.shape[-1] == 3
    if per_camera:
        _per_camera(colors, int(viewmats.shape[0]), int(means.shape[0]))
    elif colors.shape[-1] != 3 or colors.dim() != (2 if sh_degree is None else 3):
        raise NotImplementedError(f"rasterization(): colors of shape {tuple(colors.shape)} with sh_degree = {sh_degree}: 3 colour channels, "
                                  "[N,3], [C,N,3] (sh_degree None) or SH coefficients [N,K,3], are built")
    L, is_sh = 0, PER_CAMERA if per_camera else 0
    if sh_degree is not None:
        L, is_sh = int(sh_degree), 1
        if not 0 <= L <= 3:
            raise NotImplementedError(f"rasterization(): sh_degree = {sh_degree} (0 to 3 are built)")
        if (L + 1) ** 2 > int(colors.shape[1]):
            raise ValueError(f"sh_degree = {L} reads {(L + 1) ** 2} bands, colors has K = {int(colors.shape[1])}")
    if means.device.type != "cuda":
        raise RuntimeError("the rasteriser runs in libwm_hip.so on the GPU: move the splats to a HIP device")
    want_rgb, depth_mode = _RENDER_MODES[render_mode]
    opts = _Opts(int(rasterize_mode == "antialiased"), int(depth_mode or 0), float(eps2d), float(near_plane), float(far_plane), float(radius_clip))
    if _shared is None:
        _shared = Rasterizer()
    vm = viewmats.to(torch.float32)
    campos = None
    if L:
        with torch.set_grad_enabled(torch.is_grad_enabled() and vm.requires_grad):
            campos = torch.linalg.inv(vm)[:, :3, 3]
    rgb, depth, alpha, info = _shared._with_info((means, quats, scales, opacities, colors), _cin(colors, is_sh, L), is_sh, None, Ks, int(width),
                                                 int(height), bool(absgrad), L, opts=opts, backgrounds=backgrounds, cameras=(vm, campos))
    if depth_mode is None:
        return rgb, alpha, info
    return (torch.cat([rgb, depth], -1) if want_rgb else depth), alpha, info
