"""The fly-through video of the reference, ``render_interpolated_video`` (src/utils/render_utils.py:121-377, called by infer.py:264, the
demo and the post-3DGS trainer's ``render_traj``), with everything around the rasteriser on the device:

* the camera path (``interpolate_trajectory``, ``wobble_trajectory`` and the quaternion helpers, render_utils.py:14-194): plain torch ops in
  fp32 on the inputs' device, a few hundred 4 x 4 matrices;
* ``GSEffects`` (src/utils/gs_effects.py): the spread effect as one kernel, ``wm_gs_effect_spread`` (csrc/video.hip);
* ``depth_frames`` / ``rgb_frames``: ``depth_vis`` (render_utils.py:326-335), the turbo colour map and ``_make_video``'s uint8 conversion
  (:355-357) for all frames in one call, ``wm_video_frames``: exact per-frame quantiles by radix selection, no sort, no host colour map;
* ``render_interpolated_frames``: the reference's schedule (chunks of 40 views; with effects the normalisation, the 320-frame intro and the
  ``t`` / ``t_ed`` / ``loop_dir`` bookkeeping) -> uint8 frames on the device; ``render_interpolated_video`` hands them to a writer.

The kernels have no CPU path: a tensor that is not on a HIP device raises RuntimeError.  The module imports without moviepy, colorspacious,
jaxtyping and matplotlib.

Not built: mp4 encoding itself (moviepy, or a ``writer`` callable), ``effect_type`` other than 2 (the reference's ``apply_effect`` has no
other branch either), the trainer-parametrised effect output (render_utils.py:236-241: log scales and logit opacities written into
``runner.splats``; ``Rasterizer`` takes linear values), the other colour maps of color_map.py."""
from __future__ import annotations

import math
from typing import Callable, Dict, Optional, Tuple

import torch

from . import _lib
from ._lib import check, ptr, stream

SH_C0 = 0.28209479177387814
EFFECT_INTRO_FRAMES = 320      # render_utils.py:214
VIEW_CHUNK = 40                # render_utils.py:202


# ---------------------------------------------------------------------------------------------- camera path
def rotation_matrix_to_quaternion(R: torch.Tensor) -> torch.Tensor:
    """render_utils.py:14-52: R [...,3,3] -> (w, x, y, z) [...,4] by the four-branch method (trace > 0, else the largest diagonal entry).
    Every branch is evaluated and the reference's one is selected, so the selected values are the reference's."""
    m = lambda i, j: R[..., i, j]
    trace = m(0, 0) + m(1, 1) + m(2, 2)
    c1 = trace > 0
    c2 = (~c1) & (m(0, 0) > m(1, 1)) & (m(0, 0) > m(2, 2))
    c3 = (~c1) & (~c2) & (m(1, 1) > m(2, 2))
    s1 = torch.sqrt(trace + 1.0) * 2
    s2 = torch.sqrt(1.0 + m(0, 0) - m(1, 1) - m(2, 2)) * 2
    s3 = torch.sqrt(1.0 + m(1, 1) - m(0, 0) - m(2, 2)) * 2
    s4 = torch.sqrt(1.0 + m(2, 2) - m(0, 0) - m(1, 1)) * 2
    q1 = torch.stack([0.25 * s1, (m(2, 1) - m(1, 2)) / s1, (m(0, 2) - m(2, 0)) / s1, (m(1, 0) - m(0, 1)) / s1], -1)
    q2 = torch.stack([(m(2, 1) - m(1, 2)) / s2, 0.25 * s2, (m(0, 1) + m(1, 0)) / s2, (m(0, 2) + m(2, 0)) / s2], -1)
    q3 = torch.stack([(m(0, 2) - m(2, 0)) / s3, (m(0, 1) + m(1, 0)) / s3, 0.25 * s3, (m(1, 2) + m(2, 1)) / s3], -1)
    q4 = torch.stack([(m(1, 0) - m(0, 1)) / s4, (m(0, 2) + m(2, 0)) / s4, (m(1, 2) + m(2, 1)) / s4, 0.25 * s4], -1)
    return torch.where(c1[..., None], q1, torch.where(c2[..., None], q2, torch.where(c3[..., None], q3, q4)))


def quaternion_to_rotation_matrix(q: torch.Tensor) -> torch.Tensor:
    """render_utils.py:55-75: (w, x, y, z) [...,4], normalised here -> [...,3,3]"""
    w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    norm = torch.sqrt(w * w + x * x + y * y + z * z)
    w, x, y, z = w / norm, x / norm, y / norm, z / norm
    rows = [1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
            2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
            2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]
    return torch.stack(rows, -1).reshape(q.shape[:-1] + (3, 3))


def slerp_quaternions(q1: torch.Tensor, q2: torch.Tensor, t) -> torch.Tensor:
    """render_utils.py:78-118: the shorter arc; normalised linear interpolation where the dot product exceeds 0.9995.  t: a number, or a
    tensor that broadcasts against q[..., :1]."""
    dot = (q1 * q2).sum(dim=-1, keepdim=True)
    neg = dot < 0
    q2 = torch.where(neg, -q2, q2)
    dot = torch.where(neg, -dot, dot)
    linear = dot > 0.9995
    lin = q1 + t * (q2 - q1)
    lin = lin / torch.norm(lin, dim=-1, keepdim=True)
    theta_0 = torch.acos(torch.abs(dot))
    sin_theta_0 = torch.sin(theta_0)
    theta = theta_0 * t
    sin_theta = torch.sin(theta)
    s0 = torch.cos(theta) - dot * sin_theta / sin_theta_0
    s1 = sin_theta / sin_theta_0
    return torch.where(linear, lin, (s0 * q1) + (s1 * q2))


def interpolate_trajectory(camtoworlds: torch.Tensor, intrinsics: torch.Tensor, interp_per_pair: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """build_interpolated_traj (render_utils.py:137-178) over all S cameras: camtoworlds [B,S,4,4], intrinsics [B,S,3,3] ->
    ([1,F,4,4], [1,F,3,3]) with F = (S - 1)(interp_per_pair + 1).  As in the reference: each camera i < S - 1 is followed by interp_per_pair
    interpolants at alpha = j / (interp_per_pair + 1) (translation and intrinsics linear, rotation slerp), the LAST input camera is not
    emitted, and only batch element 0 is returned.  fp32, on the inputs' device."""
    n = int(interp_per_pair)
    if camtoworlds.dim() != 4 or camtoworlds.shape[-2:] != (4, 4) or intrinsics.shape[:2] != camtoworlds.shape[:2] or intrinsics.shape[-2:] != (3, 3):
        raise ValueError(f"camtoworlds [B,S,4,4] and intrinsics [B,S,3,3] expected, got {tuple(camtoworlds.shape)} and {tuple(intrinsics.shape)}")
    if n < 0 or camtoworlds.shape[1] < 2:
        raise ValueError("interpolate_trajectory needs S >= 2 cameras and interp_per_pair >= 0")
    c2w, K = camtoworlds.to(torch.float32), intrinsics.to(torch.float32)
    B, S = c2w.shape[:2]
    dev = c2w.device
    # the reference's alpha and 1 - alpha are Python floats, rounded to fp32 where they meet a tensor
    a64 = torch.tensor([j / (n + 1) for j in range(1, n + 1)], dtype=torch.float64)
    alpha = a64.to(torch.float32).to(dev).reshape(1, 1, n, 1)
    beta = (1 - a64).to(torch.float32).to(dev).reshape(1, 1, n, 1)
    R0, R1 = c2w[:, :-1, :3, :3], c2w[:, 1:, :3, :3]
    t0, t1 = c2w[:, :-1, None, :3, 3], c2w[:, 1:, None, :3, 3]                        # [B,S-1,1,3]
    q0, q1 = rotation_matrix_to_quaternion(R0)[:, :, None], rotation_matrix_to_quaternion(R1)[:, :, None]   # [B,S-1,1,4]
    t_i = beta * t0 + alpha * t1                                                        # [B,S-1,n,3]
    R_i = quaternion_to_rotation_matrix(slerp_quaternions(q0, q1, alpha))               # [B,S-1,n,3,3]
    ext = torch.eye(4, device=dev, dtype=torch.float32).repeat(B, S - 1, n, 1, 1)
    ext[..., :3, :3] = R_i
    ext[..., :3, 3] = t_i
    K_i = beta[..., None] * K[:, :-1, None] + alpha[..., None] * K[:, 1:, None]         # [B,S-1,n,3,3]
    exts = torch.cat([c2w[:, :-1, None], ext], dim=2).reshape(B, (S - 1) * (n + 1), 4, 4)
    ints = torch.cat([K[:, :-1, None], K_i], dim=2).reshape(B, (S - 1) * (n + 1), 3, 3)
    return exts[:1], ints[:1]


def wobble_trajectory(camtoworlds: torch.Tensor, intrinsics: torch.Tensor, nums: int, delta: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """build_wobble_traj (render_utils.py:181-194) for a single camera: camtoworlds [B,1,4,4], intrinsics [B,1,3,3], delta [1] (the driver
    passes the norm of the median splat position) -> ([B,nums,4,4], [B,nums,3,3]): a spiral of radius 0.15 delta in the camera's x-y plane."""
    if camtoworlds.shape[1] != 1:
        raise ValueError("wobble_trajectory is the single-camera path (S = 1)")
    dev = camtoworlds.device
    c2w, K = camtoworlds.to(torch.float32), intrinsics.to(torch.float32)
    t = torch.linspace(0, 1, int(nums), dtype=torch.float32, device=dev)
    t = (torch.cos(torch.pi * (t + 1)) + 1) / 2
    radius = torch.as_tensor(delta, dtype=torch.float32, device=dev) * 0.15
    tf = torch.eye(4, dtype=torch.float32, device=dev).broadcast_to((*radius.shape, t.shape[0], 4, 4)).clone()
    radius = radius[..., None] * t
    tf[..., 0, 3] = torch.sin(2 * torch.pi * t) * radius
    tf[..., 1, 3] = -torch.cos(2 * torch.pi * t) * radius
    exts = c2w @ tf
    return exts, K.repeat(1, exts.shape[1], 1, 1)


# ---------------------------------------------------------------------------------------------- the spread effect
def _gpu(t: torch.Tensor, what: str) -> None:
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise RuntimeError(f"{what} runs in libwm_hip.so on the GPU: pass tensors on a HIP device")


def _f32c(t: torch.Tensor) -> torch.Tensor:
    return t.detach().to(torch.float32).contiguous()


class GSEffects:
    """src/utils/gs_effects.py GSEffects with the reference's constructor, dict keys and return shape; ``apply_effect`` is one kernel.

    ``random_vals`` [N] (the per-Gaussian draw behind the random mask) is drawn once per object with ``torch.rand`` at the first call, as in
    the reference; it can be passed to the constructor or assigned to ``.random_vals`` beforehand.  After every call ``.last_stats`` holds
    a device tensor of two doubles: the number of ``flag < 0.99`` and the sum of ``flag`` (what the video driver reads each frame).

    The reference's noise term is dropped: gs_effects.py:218 multiplies it by 0.0, so the only observable difference is for non-finite
    positions (0 * inf = NaN there), which are out of contract."""

    def __init__(self, start_time: float = 0.0, end_time: float = 10.0, random_vals: Optional[torch.Tensor] = None):
        self.start_time, self.end_time = start_time, end_time
        self.last_stats = None
        if random_vals is not None:
            self.random_vals = random_vals

    def apply_effect(self, gsplat: Dict[str, torch.Tensor], t: float, effect_type: int, ignore_scale: bool = False):
        """gsplat: 'means' [N,3], 'scales' [N,3], 'colors' [N,3], 'quats' [N,4], 'opacities' [N] -> (dict with the same keys, flag [N]):
        gs_effects.py:162-242.  flag is the reference's smoothstep_val.  effect_type other than 2 raises NotImplementedError."""
        if effect_type != 2:
            raise NotImplementedError(f"effect_type = {effect_type!r}: only 2 (spread) exists, here and in the reference's apply_effect")
        out, flag = self.apply_splats(gsplat["means"], gsplat["scales"], gsplat["opacities"], gsplat["colors"], t, ignore_scale=ignore_scale)
        out["quats"] = gsplat["quats"].clone()
        return out, flag

    def apply_splats(self, means, scales, opacities, colors, t: float, ignore_scale: bool = False, shift: Optional[torch.Tensor] = None,
                     inv_scale: float = 1.0, colors_are_sh0: bool = False):
        """The kernel call behind apply_effect, as the video driver uses it: positions enter as (means - shift) * inv_scale, scales as
        scales * inv_scale (shift [3] on the device), and with colors_are_sh0 the colours are degree-0 SH on both sides
        (render_utils.py:230-234 without intermediate tensors).  -> ({'means', 'scales', 'opacities', 'colors'}, flag)"""
        _gpu(means, "GSEffects")
        dev = means.device
        m, s, o, c = _f32c(means).reshape(-1, 3), _f32c(scales).reshape(-1, 3), _f32c(opacities).reshape(-1), _f32c(colors).reshape(-1, 3)
        N = int(m.shape[0])
        if s.shape[0] != N or o.shape[0] != N or c.shape[0] != N:
            raise ValueError(f"GSEffects: {N} means, {s.shape[0]} scales, {o.shape[0]} opacities, {c.shape[0]} colours")
        for x in (s, o, c):
            _gpu(x, "GSEffects")
        if not hasattr(self, "random_vals"):
            self.random_vals = torch.rand((N,), device=dev, dtype=torch.float32)
        rv = _f32c(self.random_vals).reshape(-1)
        _gpu(rv, "GSEffects")
        if rv.shape[0] != N:
            raise ValueError(f"GSEffects: random_vals has {rv.shape[0]} entries for {N} Gaussians")
        sh = None
        if shift is not None:
            sh = _f32c(shift).reshape(-1)
            _gpu(sh, "GSEffects")
            if sh.shape[0] != 3:
                raise ValueError("GSEffects: shift must hold 3 values")
        t_n = float(t) - float(self.start_time)
        if math.isnan(t_n):
            raise ValueError("GSEffects: t is NaN")
        L = _lib.lib()
        ws_bytes = L.wm_gs_effect_spread_workspace_bytes(N)
        if ws_bytes == 0:
            raise ValueError(f"GSEffects: {N} Gaussians are outside what the library takes (N < 2^31)")
        ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
        out = {"means": torch.empty_like(m), "scales": torch.empty_like(s), "opacities": torch.empty_like(o), "colors": torch.empty_like(c)}
        flag = torch.empty((N,), device=dev, dtype=torch.float32)
        stats = torch.empty((2,), device=dev, dtype=torch.float64)
        with torch.cuda.device(dev):
            check(L.wm_gs_effect_spread(ptr(m), ptr(s), ptr(o), ptr(c), ptr(rv), N, t_n, int(bool(ignore_scale)), ptr(sh), float(inv_scale),
                                        int(bool(colors_are_sh0)), ptr(out["means"]), ptr(out["scales"]), ptr(out["opacities"]),
                                        ptr(out["colors"]), ptr(flag), ptr(stats), ptr(ws), ws_bytes, stream(dev)), "wm_gs_effect_spread")
        self.last_stats = stats
        return out, flag


# ---------------------------------------------------------------------------------------------- frames in bytes
def turbo_lut() -> torch.Tensor:
    """The 256 x 3 uint8 table the depth frames index (host): matplotlib's turbo rows as clamp(0, 1) * 255 -> uint8 gives them."""
    import ctypes as C
    buf = (C.c_ubyte * 768)()
    _lib.lib().wm_turbo_lut(buf)
    return torch.tensor(list(buf), dtype=torch.uint8).reshape(256, 3)


def _frames(rgbs: Optional[torch.Tensor], depths: Optional[torch.Tensor]):
    ref = rgbs if rgbs is not None else depths
    _gpu(ref, "the frame conversion")
    dev = ref.device
    if depths is not None:
        _gpu(depths, "the frame conversion")
        if depths.dim() == 4 and depths.shape[-1] == 1:
            depths = depths[..., 0]
        if depths.dim() != 3:
            raise ValueError(f"depths must be [F,H,W] or [F,H,W,1], got {tuple(depths.shape)}")
        depths = _f32c(depths)
    if rgbs is not None:
        if rgbs.dim() != 4 or rgbs.shape[-1] != 3:
            raise ValueError(f"rgbs must be [F,H,W,3], got {tuple(rgbs.shape)}")
        rgbs = _f32c(rgbs)
    F, H, W = (int(v) for v in (rgbs if rgbs is not None else depths).shape[:3])
    if rgbs is not None and depths is not None and tuple(depths.shape) != (F, H, W):
        raise ValueError(f"rgbs {tuple(rgbs.shape)} and depths {tuple(depths.shape)} do not describe the same frames")
    L = _lib.lib()
    ws_bytes = L.wm_video_frames_workspace_bytes(F, H, W)
    if ws_bytes == 0:
        raise ValueError(f"{F} frames of {H} x {W} are outside what the library converts (F <= 65535, H W < 2^31)")
    ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
    rgb_out = torch.empty((F, H, W, 3), device=dev, dtype=torch.uint8) if rgbs is not None else None
    dep_out = torch.empty((F, H, W, 3), device=dev, dtype=torch.uint8) if depths is not None else None
    near_far = torch.empty((F, 2), device=dev, dtype=torch.float32) if depths is not None else None
    with torch.cuda.device(dev):
        check(L.wm_video_frames(ptr(rgbs), ptr(depths), F, H, W, ptr(rgb_out), ptr(dep_out), ptr(near_far), ptr(ws), ws_bytes, stream(dev)),
              "wm_video_frames")
    return rgb_out, dep_out, near_far


def depth_frames(depths: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """depth_vis (render_utils.py:326-335) and _make_video's uint8 conversion for every frame: depths [F,H,W] (or the rasteriser's [F,H,W,1])
    -> (uint8 [F,H,W,3], near_far [F,2] fp32).  Per frame near = log(quantile(d[d > 0], 0.01)), the number 0.0 where no pixel is valid,
    far = log(quantile(d, 0.99)) over all pixels, exact with torch.quantile's linear interpolation; then
    x = 1 - (log(max(d, 1e-9)) - near) / (far - near + 1e-9), clipped to [0, 1], through the 256-row turbo table.  Degenerate frames come
    out as that arithmetic gives them (all-zero depth: every pixel turbo(1)).  NaN depths are out of contract."""
    _, out, nf = _frames(None, depths)
    return out, nf


def rgb_frames(rgbs: torch.Tensor) -> torch.Tensor:
    """_make_video's conversion (render_utils.py:355-357): rgbs [F,H,W,3] -> uint8 [F,H,W,3] = (clamp(0, 1) * 255).to(uint8)"""
    return _frames(rgbs, None)[0]


# ---------------------------------------------------------------------------------------------- the driver
def render_interpolated_frames(gs_renderer, splats: dict, camtoworlds: torch.Tensor, intrinsics: torch.Tensor, hw: Tuple[int, int],
                               interp_per_pair: int = 20, loop_reverse: bool = True, effects: Optional[GSEffects] = None, effect_type: int = 2,
                               save_mode: str = "split") -> Dict[str, torch.Tensor]:
    """render_interpolated_video up to the encoder (render_utils.py:121-359): -> {'rgb', 'depth'} (save_mode 'split') or {'both'} (rgb above
    depth), uint8 [F',H,W,3] (or [F',2H,W,3]) on the device, with ``video + video[::-1][1:-1]`` appended when loop_reverse and F > 1.

    camtoworlds [B,S,4,4], intrinsics [B,S,3,3]; S > 1 takes interpolate_trajectory, S = 1 wobble_trajectory with 12 interp_per_pair views.
    Without effects the path is rendered in chunks of 40 views from ``splats`` (batch element 0; 'sh' or 'colors').  With ``effects`` (a
    GSEffects of this module; the renderer's sh_degree must be 0 and the splats carry 'sh'): the splats are pruned by
    ``gs_renderer.prune_gs`` where the renderer has one, normalised by their median and the largest 0.95 quantile of the absolute offsets
    (the cameras with them), a 320-frame intro on the first camera runs until some flag < 0.99, keeping the frames after index 0.14 * 320,
    then every view is rendered alone with the reference's t / t_ed / loop_dir bookkeeping.  The decisions read ``effects.last_stats`` (two
    doubles per frame); the mean of flag is the fp64 sum over N where the reference takes an fp32 mean.
    ``gs_renderer.rasterizer.rasterize_batches`` is called as the reference calls it."""
    if save_mode not in ("both", "split"):
        raise ValueError("save_mode must be 'both' or 'split'")
    if effects is not None:
        if effect_type != 2:
            raise NotImplementedError(f"effect_type = {effect_type!r}: only 2 (spread) exists, here and in the reference's apply_effect")
        if not isinstance(effects, GSEffects):
            raise TypeError("effects must be a GSEffects of this module")
    b, s = int(camtoworlds.shape[0]), int(camtoworlds.shape[1])
    h, w = int(hw[0]), int(hw[1])
    if s > 1:
        all_ext, all_int = interpolate_trajectory(camtoworlds, intrinsics, interp_per_pair)
    else:
        all_ext, all_int = wobble_trajectory(camtoworlds, intrinsics, int(interp_per_pair) * 12,
                                             splats["means"][0].median(dim=0).values.norm(dim=-1)[None])
    rast = gs_renderer.rasterizer
    n_views = int(all_ext.shape[1])
    rendered_rgbs, rendered_depths = [], []

    if effects is None:
        colors = splats["sh"][:1] if "sh" in splats else splats["colors"][:1]
        sh_degree = gs_renderer.sh_degree if "sh" in splats else None
        for st in range(0, n_views, VIEW_CHUNK):
            ed = min(st + VIEW_CHUNK, n_views)
            c, d, _ = rast.rasterize_batches(splats["means"][:1], splats["quats"][:1], splats["scales"][:1], splats["opacities"][:1], colors,
                                             all_ext[:, st:ed].to(torch.float32), all_int[:, st:ed].to(torch.float32), width=w, height=h,
                                             sh_degree=sh_degree)
            rendered_rgbs.append(c)
            rendered_depths.append(d)
    else:
        if gs_renderer.sh_degree != 0:
            raise ValueError("the effects path needs a renderer with sh_degree 0 (render_utils.py:227)")
        prune = getattr(gs_renderer, "prune_gs", None)
        pruned = prune(splats, gs_renderer.voxel_size) if prune is not None else splats
        if "sh" not in pruned:
            raise ValueError("the effects path reads the splats' degree-0 'sh' (render_utils.py:231)")
        p_means, p_quats, p_scales = pruned["means"][0], pruned["quats"][0], pruned["scales"][0]
        p_opac, p_sh = pruned["opacities"][0], pruned["sh"][0].reshape(-1, 3)
        # render_utils.py:216-219: once per video
        shift = p_means.median(dim=0).values
        scale_factor = (p_means - shift).abs().quantile(0.95, dim=0).max()
        all_ext = all_ext.clone()
        all_ext[0, :, :3, -1] = (all_ext[0, :, :3, -1] - shift) / scale_factor
        inv_scale = 1.0 / float(scale_factor)
        quats = p_quats[None]

        def frame(t, ignore_scale, ext, K):
            fx, _ = effects.apply_splats(p_means, p_scales, p_opac, p_sh, t, ignore_scale=ignore_scale, shift=shift, inv_scale=inv_scale,
                                         colors_are_sh0=True)
            c, d, _ = rast.rasterize_batches(fx["means"][None], quats, fx["scales"][None], fx["opacities"][None], fx["colors"].reshape(1, -1, 1, 3),
                                             ext.to(torch.float32), K.to(torch.float32), width=w, height=h, sh_degree=gs_renderer.sh_degree)
            count, total = effects.last_stats.tolist()      # the frame's one read-back: 16 bytes
            return c, d, count, total / max(int(p_means.shape[0]), 1)

        t = 0
        count = 0
        first_ext, first_int = all_ext[:, :1], all_int[:, :1]
        for st in range(EFFECT_INTRO_FRAMES):       # render_utils.py:225-262
            if st > 0 and count > 0:
                break
            c, d, count, _ = frame(t, False, first_ext, first_int)
            t += 0.04
            if st > EFFECT_INTRO_FRAMES * 0.14:
                rendered_rgbs.append(c)
                rendered_depths.append(d)
        t_st, t_ed, loop_dir = t, 0, 1
        for st in range(n_views):                    # render_utils.py:267-319
            c, d, _, mean = frame(t, False, all_ext[:, st:st + 1], all_int[:, st:st + 1])
            t = t - 0.04 if loop_dir < 0 else t + 0.04
            if mean < 0.01 and t_ed == 0:
                t_ed = t
            if t > n_views * 0.04 + t_st - (t_ed - t_st) * 2 - 15 * 0.04 or t < t_st:
                loop_dir *= -1
                t = t_ed if loop_dir == -1 else t
            rendered_rgbs.append(c)
            rendered_depths.append(d)

    rgbs = torch.cat(rendered_rgbs, dim=1)[0]                    # [F,H,W,3]
    depths = torch.cat(rendered_depths, dim=1)[0, ..., 0]        # [F,H,W]
    rgb8, dep8, _ = _frames(rgbs, depths)

    def loop(v):
        return torch.cat([v, v.flip(0)[1:-1]], dim=0) if loop_reverse and v.shape[0] > 1 else v

    if save_mode == "both":
        return {"both": loop(torch.cat([rgb8, dep8], dim=1))}
    return {"rgb": loop(rgb8), "depth": loop(dep8)}


def _moviepy_writer() -> Callable:
    try:
        try:
            from moviepy.editor import ImageSequenceClip      # moviepy 1.x, as the reference imports it
        except ImportError:
            from moviepy import ImageSequenceClip             # moviepy 2.x
    except ImportError as e:
        raise ImportError("render_interpolated_video encodes with moviepy, which is not installed: install moviepy, or pass "
                          "writer=callable(frames uint8 [F,H,W,3], path, fps=30)") from e

    def write(frames, path, fps=30):
        ImageSequenceClip(list(frames), fps=fps).write_videofile(str(path), logger=None)
    return write


def render_interpolated_video(gs_renderer, splats: dict, camtoworlds: torch.Tensor, intrinsics: torch.Tensor, hw: Tuple[int, int], out_path,
                              interp_per_pair: int = 20, loop_reverse: bool = True, effects: Optional[GSEffects] = None, effect_type: int = 2,
                              save_mode: str = "split", writer: Optional[Callable] = None) -> None:
    """render_utils.py:121-377 with the reference's signature plus ``writer``: a callable (uint8 numpy [F,H,W,3], path, fps=30) that encodes
    one video; None is moviepy's ImageSequenceClip, and a missing moviepy raises ImportError before any GPU work.  Writes
    ``{out_path}_rgb.mp4`` and ``{out_path}_depth.mp4`` (save_mode 'split') or ``{out_path}.mp4`` ('both')."""
    if save_mode not in ("both", "split"):
        raise ValueError("save_mode must be 'both' or 'split'")
    if writer is None:
        writer = _moviepy_writer()
    frames = render_interpolated_frames(gs_renderer, splats, camtoworlds, intrinsics, hw, interp_per_pair=interp_per_pair,
                                        loop_reverse=loop_reverse, effects=effects, effect_type=effect_type, save_mode=save_mode)
    if save_mode == "both":
        writer(frames["both"].cpu().numpy(), f"{out_path}.mp4", fps=30)
    else:
        writer(frames["rgb"].cpu().numpy(), f"{out_path}_rgb.mp4", fps=30)
        writer(frames["depth"].cpu().numpy(), f"{out_path}_depth.mp4", fps=30)
