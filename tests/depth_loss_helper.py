"""A torch restatement of the trainer's sparse disparity loss and of the dataset's point projection (what
hunyuanworld_mirror_amd.depth_loss and project_depth_points fuse), generic in the dtype: in fp64 it is the reference for the GPU tests,
in fp32 their yardstick, and on the GPU in fp32 the torch composition tools/bench_depth_loss.py times.  Pinned to the reference's own
lines by tools/gen_golden_depth_loss.py through tests/golden/depth_loss_*.npz (tests/test_depth_loss_cpu.py).

loss: depths [C,H,W] sampled at the pixel coordinates points [C,M,2] (pixel centres at integers) with F.grid_sample (bilinear,
align_corners=True, zero padding) after normalising with (W - 1, H - 1); disp = 1 / d where d > 0 else 0; the mean of
|disp - 1 / depths_gt| over the rows that valid [C,M] selects (all rows of all cameras in one mean: F.l1_loss over their
concatenation).
projection: p_cam = inv(camtoworld) p_world, q = K p_cam, (x, y) = q.xy / q.z, depth = p_cam.z,
valid = visible & (0 <= x < W) & (0 <= y < H) & (depth > 0)."""
import os

import numpy as np
import torch
import torch.nn.functional as F


def pixel_span(depths, points):
    """(W - 1, H - 1) as a tensor beside points: what sample divides the pixel coordinates by"""
    return torch.tensor([depths.shape[2] - 1, depths.shape[1] - 1], dtype=points.dtype, device=points.device)


def sample(depths, points, scale=None):
    """depths [C,H,W], points [C,M,2] in pixels -> the sampled depths [C,M].  scale: pixel_span(depths, points) made ahead by a caller that
    times this on a GPU (making it is a copy from the host); None makes it here"""
    if scale is None:
        scale = pixel_span(depths, points)
    grid = (points / scale * 2 - 1).unsqueeze(2)                                 # [C, M, 1, 2] in [-1, 1]
    return F.grid_sample(depths.unsqueeze(1), grid, mode="bilinear", padding_mode="zeros", align_corners=True)[:, 0, :, 0]


def disparity(d):
    """1 / d where d > 0, else 0 with a ZERO derivative: the reciprocal is taken of a stand-in 1 where d <= 0.  (Differentiating
    torch.where(d > 0, 1 / d, 0) as written gives 0 * (-1 / 0^2) = NaN for a sample that is exactly 0; the kernels define such a row to
    add nothing.)"""
    pos = d > 0.0
    return torch.where(pos, 1.0 / torch.where(pos, d, torch.ones_like(d)), torch.zeros_like(d))


def terms(depths, points, depths_gt):
    """-> disp [C,M], disp_gt [C,M]"""
    return disparity(sample(depths, points)), 1.0 / depths_gt


def loss(depths, points, depths_gt, valid=None):
    """valid: bool [C,M] or None.  Rows that valid leaves out are replaced by harmless values before any arithmetic (they may be NaN)."""
    if valid is None:
        valid = torch.ones(depths_gt.shape, dtype=torch.bool, device=depths_gt.device)
    points = torch.where(valid[..., None], points, torch.zeros_like(points))
    depths_gt = torch.where(valid, depths_gt, torch.ones_like(depths_gt))
    disp, disp_gt = terms(depths, points, depths_gt)
    return (disp - disp_gt).abs()[valid].mean()


def gradients(depths, points, depths_gt, valid, dtype, g=1.0):
    """the loss in dtype from (fp32) inputs -> dict(loss 0-d, v_depth [C,H,W]) as CPU tensors of dtype; g: the upstream gradient"""
    d = depths.detach().to(dtype).requires_grad_(True)
    out = loss(d, points.detach().to(dtype), depths_gt.detach().to(dtype), valid)
    (out * g).backward()
    return dict(loss=out.detach(), v_depth=d.grad)


def scalar_bound(depths, points, depths_gt, valid=None):
    """the bound of the scalar loss in fp32 arithmetic: 16 * 2^-24 * mean(disp + disp_gt) over the valid rows, from the fp64 helper"""
    disp, disp_gt = terms(depths.double(), points.double(), depths_gt.double())
    s = disp + disp_gt
    if valid is not None:
        s = s[valid]
    return 16.0 * 2.0 ** -24 * float(s.mean())


def gradient_bound(depths, points, depths_gt, valid=None):
    """An absolute bound on any element of a gradient formed as csrc/depthloss.hip forms it (fp32 inputs taken exactly, the sample and the
    coefficient -sign / d^2 in fp64, the coefficient rounded to fp32 once, a pixel's sum and the scale in fp64, one final rounding):
    2^-24 * (A + V), doubled for slack, with V the largest |element| and A the largest element of sum_m w_m / (n d_m^2) -- the sum of the
    magnitudes a pixel adds up, which is the gradient of mean(disp) (every sign equal), from the fp64 helper."""
    d = depths.detach().double().requires_grad_(True)
    p, gt = points.double(), depths_gt.double()
    if valid is None:
        valid = torch.ones(gt.shape, dtype=torch.bool)
    p = torch.where(valid[..., None], p, torch.zeros_like(p))
    disparity(sample(d, p))[valid].mean().backward()
    v = gradients(depths, points, depths_gt, valid, torch.float64)["v_depth"]
    return 2.0 * 2.0 ** -24 * (float(d.grad.abs().max()) + float(v.abs().max()))


def project(points_world, camtoworlds, Ks, width, height, visible=None):
    """points_world [P,3], camtoworlds [C,4,4], Ks [C,3,3] -> points [C,P,2], depths [C,P], valid [C,P] in the inputs' dtype"""
    w2c = torch.linalg.inv(camtoworlds)
    cam = torch.einsum("cij,pj->cpi", w2c[:, :3, :3], points_world) + w2c[:, None, :3, 3]
    proj = torch.einsum("cij,cpj->cpi", Ks, cam)
    points = proj[..., :2] / proj[..., 2:3]
    depths = cam[..., 2]
    valid = (points[..., 0] >= 0) & (points[..., 0] < width) & (points[..., 1] >= 0) & (points[..., 1] < height) & (depths > 0)
    if visible is not None:
        valid = valid & visible
    return points, depths, valid


def kink_margin(depths, points, depths_gt, valid=None):
    """smallest |disp - disp_gt| / disp_gt over the valid rows (fp64): the L1 kink, where fp32 and fp64 could disagree about a sign"""
    disp, disp_gt = terms(depths.double(), points.double(), depths_gt.double())
    r = (disp - disp_gt).abs() / disp_gt
    if valid is not None:
        r = r[valid]
    return float(r.min()) if r.numel() else float("inf")


def cell_margin(points, valid=None):
    """smallest distance of a valid coordinate to an integer (fp64): closer than fp32 rounding, and the two precisions could pick
    different cells.  Points placed on integers on purpose are exact in both and are left out (distance 0)."""
    p = points.double()
    if valid is not None:
        p = p[valid]
    d = (p - p.round()).abs()
    d = d[d > 0]
    return float(d.min()) if d.numel() else float("inf")


def max_rel(a, b):
    """largest |a - b| relative to the largest |b| (the measure of tests/bilagrid_helper.py)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def load_golden(name):
    """tests/golden/depth_loss_<name>.npz -> dict of arrays"""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"depth_loss_{name}.npz")
    return dict(np.load(path, allow_pickle=False))
