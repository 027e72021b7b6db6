"""Writes tests/golden/depth_loss_a.npz, depth_loss_b.npz and depth_loss_proj.npz: the REFERENCE's own depth-loss lines and its own
projection lines, run on the CPU in fp64 on fp32-valued inputs.  Data only: inputs, the loss, depths.grad (as the reference gives it, `v_depth_raw`: NaN in the
pixels under a row whose sample is exactly 0, see reference_live_gradient, and `v_depth`: the same block on the rows with d > 0), the
projected points, the camera-space depths and the selector.

    python tools/gen_golden_depth_loss.py <reference gsplat examples dir>

Nothing of the reference is copied or imported (the trainer needs CUDA-only packages, the dataset module needs pycolmap and cv2).  Both
files are parsed with `ast`; the `if cfg.depth_loss:` statement of simple_trainer_worldmirror.py that holds the grid_sample call and
the `if self.load_depths:` statement of Dataset.__getitem__ in datasets/colmap.py are compiled on their own and executed in a small
namespace of torch, F, np and stub self / cfg / parser objects, on this tool's inputs.

Scenes (loss)
  a   2 cameras, 9 x 13 (H x W), 50 points per camera, a rectangle of zero depths, some x > W - 1.
  b   3 cameras, 48 x 64, 1537 points per camera: 320 inside one cell (four pixels share them), 40 on integer coordinates, 20 on
      x = W - 1 exactly, 40 with x in (W - 1, W), 40 with y in (H - 1, H), the rest uniform; the groups are interleaved by a fixed
      permutation so that the crowded pixels receive their rows spread over the whole index range.
  Every depth is exactly 0 or at least 0.2.  A candidate point is drawn again until: it is at least 1e-3 px from an integer on both
  axes (except where it was put on one), its sampled depth is exactly 0 or at least 0.05, and its term keeps
  |disp - disp_gt| >= 1e-2 disp_gt (the L1 kink: ten times what tests/test_depth_loss_cpu.py asks again); a point placed on a grid line is
  also drawn again when its sample is exactly 0 (see _draw), so that the restatement in fp32 stays a yardstick for the scene.
Scene (projection)
  proj  3 cameras (rotations of up to ~25 degrees, fp32-rounded), 64 x 48 (W x H), 400 world points, a `visible` mask that drops 15 %:
        points behind the camera and outside every image bound included; no coordinate of a visible point within 1e-4 px of a bound,
        no z within 1e-5 of 0."""
import ast
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import depth_loss_helper as DH  # noqa: E402


def _find_if(path, test_src, must_call=None, inside=None):
    """the ast.If of `path` whose test reads `test_src` (and whose body calls `must_call`; inside = (class name, function name))"""
    tree = ast.parse(open(path).read())
    scope = tree
    if inside:
        cls = next(n for n in ast.walk(tree) if isinstance(n, ast.ClassDef) and n.name == inside[0])
        scope = next(n for n in ast.walk(cls) if isinstance(n, ast.FunctionDef) and n.name == inside[1])
    found = []
    for n in ast.walk(scope):
        if isinstance(n, ast.If) and ast.unparse(n.test) == test_src:
            calls = {c.func.attr for c in ast.walk(n) if isinstance(c, ast.Call) and isinstance(c.func, ast.Attribute)}
            if must_call is None or must_call in calls:
                found.append(n)
    assert len(found) == 1, (path, test_src, len(found))
    return found[0]


def _compile_body(node, name):
    mod = ast.Module(body=node.body, type_ignores=[])
    return compile(ast.fix_missing_locations(mod), name, "exec")


def reference_loss(code, depths, points, depths_gt):
    """the trainer's block on fp64 tensors: depths [C,H,W] -> loss (scene_scale = depth_lambda = 1), depths.grad"""
    C, H, W = depths.shape
    d = depths.double().reshape(C, H, W, 1).clone().requires_grad_(True)
    ns = dict(torch=torch, F=F, np=np, cfg=types.SimpleNamespace(depth_loss=True, depth_lambda=1.0), self=types.SimpleNamespace(scene_scale=1.0),
              points=points.double(), depths=d, depths_gt=depths_gt.double(), width=W, height=H, loss=torch.zeros((), dtype=torch.float64))
    exec(code, ns)
    ns["depthloss"].backward()
    assert abs(float(ns["loss"].detach()) - float(ns["depthloss"].detach())) == 0.0
    return ns["depthloss"].detach(), d.grad.reshape(C, H, W), ns["depths"].detach()       # (the block rebinds `depths` to the samples [C,M])


def reference_live_gradient(code, depths, points, depths_gt, sampled):
    """The reference differentiates torch.where(d > 0, 1 / d, 0) as written: a row whose sample is EXACTLY 0 sends 0 * (-1 / 0^2) = NaN
    into its four pixels.  This project defines such a row to add nothing (include/wm_hip.h).  The same block, run per camera on the rows
    with d > 0 alone and weighted by their share of the mean, is the reference's own number for that definition."""
    C, M = depths_gt.shape
    out = torch.zeros(depths.shape, dtype=torch.float64)
    for c in range(C):
        live = sampled[c] > 0
        if int(live.sum()):
            _, g, _ = reference_loss(code, depths[c:c + 1], points[c:c + 1, live], depths_gt[c:c + 1, live])
            out[c] = g[0] * (int(live.sum()) / (C * M))
    return out


def reference_projection(code, points_world, camtoworlds, Ks, W, H, visible):
    """the dataset's block per camera in numpy fp64 -> points [C,P,2], depths [C,P] (NaN where not visible), valid [C,P]"""
    C, P = visible.shape
    pts = np.full((C, P, 2), np.nan)
    dep = np.full((C, P), np.nan)
    valid = np.zeros((C, P), bool)
    for c in range(C):
        idx = np.nonzero(visible[c].numpy())[0]
        parser = types.SimpleNamespace(image_names=["img"], point_indices={"img": idx}, points=points_world.double().numpy())
        data = {}
        ns = dict(np=np, torch=torch, self=types.SimpleNamespace(parser=parser, load_depths=True), camtoworlds=camtoworlds[c].double().numpy(),
                  K=Ks[c].double().numpy(), index=0, image=np.zeros((H, W, 3), np.float32), data=data)
        exec(code, ns)
        sel = ns["selector"]
        proj, cam = ns["points_proj"], ns["points_cam"]
        pts[c, idx] = proj[:, :2] / proj[:, 2:3]
        dep[c, idx] = cam[:, 2]
        valid[c, idx[sel]] = True
        # what the block hands on is the selected rows of exactly these numbers
        assert np.array_equal(data["points"].numpy(), pts[c, idx[sel]].astype(np.float32))
        assert np.array_equal(data["depths"].numpy(), dep[c, idx[sel]].astype(np.float32))
    return pts, dep, valid


def _depth_image(g, C, H, W, rect):
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    ph = torch.arange(C, dtype=torch.float32).reshape(C, 1, 1)
    d = 1.6 + 0.9 * torch.sin(0.45 * xx + 0.3 * yy + ph) * torch.cos(0.2 * yy - 0.6 * ph) + 0.4 * torch.rand(C, H, W, generator=g)
    d = d.clamp_min(0.2)
    y0, y1, x0, x1 = rect
    d[:, y0:y1, x0:x1] = 0.0
    return d


def _draw(g, depth_c, n, kind, cell=None):
    """n accepted points of one kind for one camera -> points [n,2], depths_gt [n] (fp32)"""
    H, W = depth_c.shape
    out_p, out_g = [], []
    while len(out_p) < n:
        u = torch.rand(2, generator=g)
        if kind == "uniform":
            p = u * torch.tensor([W, H], dtype=torch.float32)
        elif kind == "cluster":
            p = torch.tensor(cell, dtype=torch.float32) + u
        elif kind == "integer":
            p = torch.floor(u * torch.tensor([W, H], dtype=torch.float32))
        elif kind == "x_last":
            p = torch.stack([torch.tensor(float(W - 1)), u[1] * H])
        elif kind == "x_strip":
            p = torch.stack([W - 1 + u[0], u[1] * H])
        elif kind == "y_strip":
            p = torch.stack([u[0] * W, H - 1 + u[1]])
        gt = (0.4 + 3.6 * torch.rand((), generator=g)).float()
        if not (0 <= float(p[0]) < W and 0 <= float(p[1]) < H):
            continue
        frac = (p.double() - p.double().round()).abs()
        on_grid = {"integer": (True, True), "x_last": (True, False)}.get(kind, (False, False))
        if any((not og) and float(f) < 1e-3 for og, f in zip(on_grid, frac)):
            continue
        d = float(DH.sample(depth_c.double()[None], p.double()[None, None])[0, 0])
        if not (d == 0.0 or d >= 0.05):
            continue
        if any(on_grid) and d == 0.0:
            # a point ON a grid line whose sample is exactly 0 has zero pixels under it and live ones a rounding away: in fp32 the reference's own
            # normalisation with (W - 1) moves it off the line, the sample becomes ~1e-7 and the disparity ~1e7, and the fp32 restatement stops
            # being a yardstick for the whole scene.  Rows with a sample of exactly 0 come from points strictly inside the zero rectangle.
            continue
        disp = 1.0 / d if d > 0 else 0.0
        if abs(disp - 1.0 / float(gt)) < 1e-2 / float(gt):
            continue
        out_p.append(p)
        out_g.append(gt)
    return torch.stack(out_p), torch.stack(out_g)


def scene_a(seed=11):
    g = torch.Generator().manual_seed(seed)
    C, H, W, M = 2, 9, 13, 50
    depths = _depth_image(g, C, H, W, (2, 5, 3, 8))
    pts, gts = [], []
    for c in range(C):
        parts = [_draw(g, depths[c], 6, "x_strip"), _draw(g, depths[c], 4, "y_strip"), _draw(g, depths[c], M - 10, "uniform")]
        perm = torch.randperm(M, generator=g)
        pts.append(torch.cat([p for p, _ in parts])[perm])
        gts.append(torch.cat([q for _, q in parts])[perm])
    return dict(depths=depths, points=torch.stack(pts), depths_gt=torch.stack(gts))


def scene_b(seed=12):
    g = torch.Generator().manual_seed(seed)
    C, H, W, M = 3, 48, 64, 1537
    depths = _depth_image(g, C, H, W, (30, 41, 10, 29))
    cells = [(40, 12), (31, 15), (62, 46)]        # (x0, y0) per camera: the tile interior, the 32-pixel seams, the last cell
    groups = [("cluster", 320), ("integer", 40), ("x_last", 20), ("x_strip", 40), ("y_strip", 40)]
    pts, gts = [], []
    for c in range(C):
        parts = [_draw(g, depths[c], n, kind, cells[c]) for kind, n in groups]
        parts.append(_draw(g, depths[c], M - sum(n for _, n in groups), "uniform"))
        perm = torch.randperm(M, generator=g)
        pts.append(torch.cat([p for p, _ in parts])[perm])
        gts.append(torch.cat([q for _, q in parts])[perm])
    return dict(depths=depths, points=torch.stack(pts), depths_gt=torch.stack(gts))


def scene_proj(seed=13):
    g = torch.Generator().manual_seed(seed)
    C, P, W, H = 3, 400, 64, 48

    def rot(ax, a):
        c, s = np.cos(a), np.sin(a)
        m = {0: [[1, 0, 0], [0, c, -s], [0, s, c]], 1: [[c, 0, s], [0, 1, 0], [-s, 0, c]], 2: [[c, -s, 0], [s, c, 0], [0, 0, 1]]}[ax]
        return torch.tensor(m, dtype=torch.float64)

    c2w = torch.eye(4, dtype=torch.float64).repeat(C, 1, 1)
    for c in range(C):
        a = (torch.rand(3, generator=g, dtype=torch.float64) - 0.5) * 0.9
        c2w[c, :3, :3] = rot(0, float(a[0])) @ rot(1, float(a[1])) @ rot(2, float(a[2]))
        c2w[c, :3, 3] = (torch.rand(3, generator=g, dtype=torch.float64) - 0.5) * torch.tensor([1.0, 0.6, 0.8])
    c2w = c2w.float()
    Ks = torch.tensor([[52.0, 0, W / 2 + 0.7], [0, 49.0, H / 2 - 1.3], [0, 0, 1]]).repeat(C, 1, 1)
    Ks[1, 0, 1] = 0.25                              # a skew term: the whole 3 x 3 is used
    pw = []
    while len(pw) < P:
        p = ((torch.rand(3, generator=g) - 0.5) * torch.tensor([7.0, 5.0, 9.0]) + torch.tensor([0.0, 0.0, 2.0])).float()
        xy, z, _ = DH.project(p.double()[None], c2w.double(), Ks.double(), W, H)
        xy, z = xy[:, 0], z[:, 0]
        near = torch.cat([xy[:, 0].abs(), (xy[:, 0] - W).abs(), xy[:, 1].abs(), (xy[:, 1] - H).abs()]).min()
        if float(near) < 1e-4 or float(z.abs().min()) < 1e-5:
            continue
        pw.append(p)
    visible = torch.rand(C, P, generator=g) >= 0.15
    return dict(points_world=torch.stack(pw), camtoworlds=c2w, Ks=Ks, visible=visible, width=W, height=H)


def main(examples_dir):
    loss_code = _compile_body(_find_if(os.path.join(examples_dir, "simple_trainer_worldmirror.py"), "cfg.depth_loss", must_call="grid_sample"),
                              "reference depth-loss block")
    proj_code = _compile_body(_find_if(os.path.join(examples_dir, "datasets", "colmap.py"), "self.load_depths", inside=("Dataset", "__getitem__")),
                              "reference projection block")
    gold = os.path.join(ROOT, "tests", "golden")
    for name, sc in (("a", scene_a()), ("b", scene_b())):
        loss, grad, sampled = reference_loss(loss_code, sc["depths"], sc["points"], sc["depths_gt"])
        live = reference_live_gradient(loss_code, sc["depths"], sc["points"], sc["depths_gt"], sampled)
        dead = int((sampled == 0).sum())
        assert torch.isfinite(loss) and torch.isfinite(live).all() and float(live.abs().max()) > 0 and dead >= 5
        fin = torch.isfinite(grad)
        assert int((~fin).sum()) > 0 and float((grad[fin] - live[fin]).abs().max()) <= 1e-12 * float(live.abs().max())
        assert ((sc["depths"] == 0) | (sc["depths"] >= 0.2)).all() and int((sc["depths"] == 0).sum()) > 0
        assert DH.kink_margin(sc["depths"], sc["points"], sc["depths_gt"]) >= 1e-2
        f32 = DH.gradients(sc["depths"], sc["points"], sc["depths_gt"], None, torch.float32)
        yard = DH.max_rel(f32["v_depth"].numpy(), live.numpy())
        assert yard < 1e-4 and abs(float(f32["loss"]) - float(loss)) < 1e-5, (name, yard)      # the fp32 restatement stays a measure on this scene
        path = os.path.join(gold, f"depth_loss_{name}.npz")
        np.savez_compressed(path, depths=sc["depths"].numpy(), points=sc["points"].numpy(), depths_gt=sc["depths_gt"].numpy(),
                            loss=np.float64(loss), v_depth_raw=grad.numpy(), v_depth=live.numpy())
        print(name, "fp32 yardstick", yard, "loss", float(loss), "max |grad|", float(live.abs().max()), "rows with d == 0:", dead, "NaN pixels in the raw gradient:",
              int((~fin).sum()), os.path.getsize(path), "bytes")
    sc = scene_proj()
    pts, dep, valid = reference_projection(proj_code, sc["points_world"], sc["camtoworlds"], sc["Ks"], sc["width"], sc["height"], sc["visible"])
    path = os.path.join(gold, "depth_loss_proj.npz")
    np.savez_compressed(path, points_world=sc["points_world"].numpy(), camtoworlds=sc["camtoworlds"].numpy(), Ks=sc["Ks"].numpy(),
                        visible=sc["visible"].numpy(), width=np.int64(sc["width"]), height=np.int64(sc["height"]), points=pts, depths=dep, valid=valid)
    print("proj valid", int(valid.sum()), "of", int(sc["visible"].sum()), "visible,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
