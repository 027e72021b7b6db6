"""numpy / torch restatement of the trainer's evaluation (gsplat's simple_trainer_worldmirror.py:1040-1060) for the tests of
hunyuanworld_mirror_amd.metrics: the canvas bytes, the PSNR in fp64, and color_correct (examples/lib_bilagrid.py:56-126) in two forms.

  color_correct        the normal-equation form the kernels use: per iteration and channel the masked 10 x 10 Gram matrix and right-hand
                       side, a symmetric eigendecomposition and the minimum-norm solution over the eigenvalues above CUTOFF * largest.
                       Run in fp64 it is the yardstick of the GPU tests; tests/test_eval_cpu.py pins it to the reference's own fp64
                       output (tests/golden/eval_*.npz).
  color_correct_lstsq  the reference's composition restated: the [P,10] feature matrix, three masked copies, torch.linalg.lstsq.  Run in
                       fp32 against the fp64 form above it gives e32, the reference's own fp32 error, for sizes without a fixture; on
                       the GPU it is the torch baseline of tools/bench_eval_metrics.py.

Scenes (make_inputs): the masks are step functions at eps and 1 - eps, so a value within rounding distance of a threshold would flip a
row of a system and move the fit by far more than any tolerance.  The scenes are built so that this cannot happen, and guard_margin
measures it: ref is 8-bit (k / 255, so eps = 0.5 / 255 sits half a level from every value), the interior stays in [0.1, 0.9] under a
mild tint plus noise, and separate small populations that exercise each term of the mask (render saturated, ground truth saturated,
estimate clipped by the warp) take a handful of values each (draw_scene)."""
import os

import numpy as np
import torch

EPS = 0.5 / 255
NUM_ITERS = 5
CUTOFF = 1e-10          # relative eigenvalue cut-off; csrc/evalmetrics.hip CC_CUTOFF, DESIGN.md section 8
GUARD_FACTOR = 256.0    # no masked value within GUARD_FACTOR * e32 of a threshold

# name: (B, H, W, first seed tried)
SCENES = {"a": (1, 37, 52, 100), "b": (1, 61, 83, 200), "min": (1, 11, 11, 300), "big": (1, 300, 301, 400), "pair": (2, 37, 52, 500)}


def features(m):
    """[P,3] -> [P,10]: rr rg rb gg gb bb r g b 1"""
    r, g, b = m[:, 0:1], m[:, 1:2], m[:, 2:3]
    return torch.cat([r * r, r * g, r * b, g * g, g * b, b * b, m, torch.ones_like(r)], dim=-1)


def _unclipped(z, eps):
    return (z >= eps) & (z <= 1 - eps)


def color_correct(img, ref, num_iters=NUM_ITERS, eps=EPS, cutoff=CUTOFF, info=None):
    """Gram + pseudo-inverse form, in img's dtype.  info (a dict) receives: margin = the smallest distance of any ref value and of any
    img_mat value of any iteration from eps / 1 - eps; ratio_genuine = the smallest kept eigenvalue ratio; ratio_spurious = the largest
    dropped one (0 if none)."""
    shape = img.shape
    m = img.reshape(-1, 3)
    r = ref.reshape(-1, 3).to(m.dtype)
    mask0 = _unclipped(m, eps)

    def margin(z):
        z = z.double()
        return float(torch.minimum((z - eps).abs(), (z - (1 - eps)).abs()).min())
    mar, gen, spu = margin(r), float("inf"), 0.0
    for _ in range(num_iters):
        mar = min(mar, margin(m))
        A = features(m)
        W = []
        for c in range(3):
            mask = (mask0[:, c] & _unclipped(m[:, c], eps) & _unclipped(r[:, c], eps)).to(m.dtype)
            Am = A * mask[:, None]
            G = Am.T @ Am
            rhs = Am.T @ (r[:, c] * mask)
            lam, V = torch.linalg.eigh(G)
            lmax = float(lam.max())
            keep = lam > cutoff * lmax if lmax > 0 else torch.zeros_like(lam, dtype=torch.bool)
            if lmax > 0:
                ratios = (lam / lmax).double()
                if keep.any():
                    gen = min(gen, float(ratios[keep].min()))
                if (~keep).any():
                    spu = max(spu, float(ratios[~keep].abs().max()))
            coef = torch.where(keep, (V.T @ rhs) / torch.where(keep, lam, torch.ones_like(lam)), torch.zeros_like(lam))
            W.append(V @ coef)
        m = torch.clip(A @ torch.stack(W, dim=-1), 0, 1)
    mar = min(mar, margin(m))
    if info is not None:
        info.update(margin=mar, ratio_genuine=gen, ratio_spurious=spu)
    return m.reshape(shape)


def color_correct_lstsq(img, ref, num_iters=NUM_ITERS, eps=EPS, driver=None):
    """The reference's composition: feature matrix, masked copies, lstsq (driver None: torch's default for the device)."""
    shape = img.shape
    m = img.reshape(-1, 3)
    r = ref.reshape(-1, 3).to(m.dtype)
    mask0 = _unclipped(m, eps)
    for _ in range(num_iters):
        A = features(m)
        W = []
        for c in range(3):
            mask = mask0[:, c] & _unclipped(m[:, c], eps) & _unclipped(r[:, c], eps)
            Am = torch.where(mask[:, None], A, torch.zeros_like(A))
            bm = torch.where(mask, r[:, c], torch.zeros_like(r[:, c]))
            W.append(torch.linalg.lstsq(Am, bm[:, None], rcond=-1, driver=driver)[0][:, 0])
        m = torch.clip(A @ torch.stack(W, dim=-1), 0, 1)
    return m.reshape(shape)


def color_correct_normal(img, ref, num_iters=NUM_ITERS, eps=EPS):
    """The same steps as device-agnostic torch ops in normal-equation form (Gram matrix, torch.linalg.solve): the baseline where the
    device's lstsq is unusable.  Full-rank systems only."""
    shape = img.shape
    m = img.reshape(-1, 3)
    r = ref.reshape(-1, 3).to(m.dtype)
    mask0 = _unclipped(m, eps)
    for _ in range(num_iters):
        A = features(m)
        W = []
        for c in range(3):
            mask = (mask0[:, c] & _unclipped(m[:, c], eps) & _unclipped(r[:, c], eps)).to(m.dtype)
            Am = A * mask[:, None]
            W.append(torch.linalg.solve((Am.T @ Am).double(), (Am.T @ (r[:, c] * mask)).double()).to(m.dtype))
        m = torch.clip(A @ torch.stack(W, dim=-1), 0, 1)
    return m.reshape(shape)


def e32_of(img, ref, num_iters=NUM_ITERS, eps=EPS):
    """max |fp32 composition - fp64 Gram form| on fp32-valued inputs: the reference's own fp32 error, with LAPACK's gels (QR) driver, the
    one driver torch.linalg.lstsq has on the device and the most accurate of the CPU's (at 300 x 300 the CPU default gelsy gives 4e-6
    and varies with the thread count, gels 1e-6): the smaller yardstick"""
    lo = color_correct_lstsq(img.float(), ref.float(), num_iters, eps, driver="gels").double()
    hi = color_correct(img.double(), ref.double(), num_iters, eps)
    return float((lo - hi).abs().max())


def draw_scene(B, H, W, seed):
    """-> img (the clamped render), ref (the 8-bit ground truth): fp32 [B,H,W,3]"""
    g = torch.Generator().manual_seed(seed)
    k = torch.randint(26, 230, (B, H, W, 3), generator=g)                 # interior: 0.1 .. 0.9
    ref = k.to(torch.float32) / 255.0
    M = 0.85 * torch.eye(3) + 0.04 * torch.rand(3, 3, generator=g)
    off = 0.02 * torch.rand(3, generator=g) - 0.01
    noise = 0.03 * torch.rand(B, H, W, 3, generator=g) - 0.015
    r64, M64 = ref.double(), M.double()
    tint = r64[..., 0:1] * M64[:, 0] + r64[..., 1:2] * M64[:, 1] + r64[..., 2:3] * M64[:, 2]     # elementwise: the same bits on every host
    img = (tint + 0.03 * r64 * r64 + off.double() + noise.double()).float()
    # separate populations that take a handful of values each, one per term of the mask (the warp moves them to at most 8 values per
    # channel and iteration, which the guard checks like every other value):
    #   the render saturated to exactly 0 / 1 per channel (about 4 %): out by mask0
    #   the ground truth saturated to exactly 0 / 1 per channel under a render of 0.25 / 0.75 (about 3 %): out by is_unclipped(ref)
    #   the render at 0.985 / 0.004 per channel, just inside the unclipped range (about 2 %): in at first; the warp pushes 0.985 past 1,
    #   so the clip takes it out by is_unclipped(img_mat) from the second iteration on
    pop = torch.rand(B, H, W, generator=g)
    corner = torch.randint(0, 2, (B, H, W, 3), generator=g).to(torch.float32)
    other = torch.randint(0, 2, (B, H, W, 3), generator=g).to(torch.float32)
    sat_img = (pop < 0.04)[..., None]
    sat_ref = ((pop >= 0.04) & (pop < 0.07))[..., None]
    edge = ((pop >= 0.07) & (pop < 0.09))[..., None]
    img = torch.where(sat_img, corner, img)
    ref = torch.where(sat_ref, corner, ref)
    img = torch.where(sat_ref, 0.25 + 0.5 * other, img)
    img = torch.where(edge, torch.where(other > 0, torch.full_like(img, 0.985), torch.full_like(img, 0.004)), img)
    return img.contiguous(), ref.contiguous()


def guard_margin(img, ref, per_image=False, num_iters=NUM_ITERS, eps=EPS):
    """The smallest distance from a threshold over ref and every iteration's img_mat, from the fp64 Gram form"""
    if per_image:
        return min(guard_margin(img[b], ref[b], False, num_iters, eps) for b in range(img.shape[0]))
    info = {}
    color_correct(img.double(), ref.double(), num_iters, eps, info=info)
    return info["margin"]


_CACHE = {}


def make_inputs(name):
    """-> dict(img, ref, seed, e32, margin [, cc64]).  Scenes with a fixture (tests/golden/eval_<name>.npz: "a", "b") take the fixture's
    inputs (draw_scene of its seed), its e32 (the reference's own) and its cc64.  The others take the first seed from
    the scene's start for which the guard holds, for the batch as one system and for each image alone, with e32 computed here from the
    restated composition.  The guard is asserted for every scene.  Cached; do not modify."""
    if name in _CACHE:
        return _CACHE[name]
    B, H, W, seed0 = SCENES[name]
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"eval_{name}.npz")
    if os.path.exists(path):
        z = np.load(path, allow_pickle=False)
        seed, e = int(z["seed"]), float(z["e32"])
        img, ref = torch.from_numpy(z["img"]), torch.from_numpy(z["ref"])      # (tests/test_eval_cpu.py: they are draw_scene(seed))
        mar = guard_margin(img, ref)
        extra = dict(cc64=torch.from_numpy(z["cc64"]))
    else:
        extra = {}
        for seed in range(seed0, seed0 + 50):
            img, ref = draw_scene(B, H, W, seed)
            e, mar = e32_of(img, ref), guard_margin(img, ref)
            if B > 1:
                mar = min(mar, guard_margin(img, ref, per_image=True))
                e = max([e] + [e32_of(img[b], ref[b]) for b in range(B)])
            if mar >= GUARD_FACTOR * e:
                break
    assert mar >= GUARD_FACTOR * e, f"scene {name}: a masked value lies within {GUARD_FACTOR} e32 = {GUARD_FACTOR * e:.3e} of a threshold ({mar:.3e})"
    _CACHE[name] = dict(img=img, ref=ref, seed=seed, e32=e, margin=mar, **extra)
    return _CACHE[name]


def frame_inputs(B, H, W, seed):
    """-> colors (unclamped render, about 10 % of the values outside [0, 1]) and pixels (uint8 / 255.0 in fp32, as the trainer's loader)"""
    g = torch.Generator().manual_seed(seed)
    k = torch.randint(0, 256, (B, H, W, 3), generator=g)
    pixels = k.to(torch.float32) / 255.0
    colors = pixels + 0.1 * torch.randn(B, H, W, 3, generator=g)
    wild = torch.rand(B, H, W, 3, generator=g)
    colors = torch.where(wild < 0.05, -0.3 * torch.ones_like(colors), colors)
    colors = torch.where(wild > 0.95, 1.7 * torch.ones_like(colors), colors)
    return colors.contiguous(), pixels.contiguous()


def canvas_bytes(colors, pixels):
    """:1040-1046 for a batch: uint8 [B,H,2W,3]"""
    c = torch.clamp(colors, 0.0, 1.0)
    canvas = torch.cat([pixels, c], dim=2).numpy()
    assert canvas.dtype == np.float32
    return (canvas * 255).astype(np.uint8)


def psnr64(colors, pixels, data_range=1.0, per_image=False, clamp=True):
    """10 log10(range^2 / mse) in fp64 of the fp32 values (clamped as :1040 first): a float, or [B] with per_image"""
    c = (torch.clamp(colors, 0.0, 1.0) if clamp else colors).double()
    d2 = (c - pixels.double()) ** 2
    mse = d2.reshape(d2.shape[0], -1).mean(dim=1) if per_image else d2.mean()
    out = 10.0 * torch.log10(data_range ** 2 / mse)
    return out.numpy() if per_image else float(out)
