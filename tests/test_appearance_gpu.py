"""The appearance module on the GPU (wm_appearance_* through hunyuanworld_mirror_amd.AppearanceOptModule) against the reference's own fp64
numbers (tests/golden/appearance_*.npz) and against the torch restatement tests/appearance_helper.py (pinned to those numbers by
tests/test_appearance_cpu.py).

Tolerance (the yardstick of test_bilagrid_gpu.py): per quantity the helper's own fp32-against-fp64 error on the same inputs, as the largest
element error relative to the largest element, never less than one fp32 ulp; the kernels order their sums differently (an MFMA's k order,
per-block partial sums), so they may exceed it by FACTOR = 4.  Ratios measured on MI355X: profiles/r14_appearance.md.

Scenes are drawn so that no hidden pre-activation lies within 16 x its own fp32 error of zero (ReLU's kink).  The goldens get there by
trying seeds; a scene of N = 1000, C = 4 has 5 x 10^5 pre-activations of which a dozen land inside that margin in any draw, so the extra
shapes draw those Gaussians again instead (appearance_helper.random_scene(redraw=True)): the same condition, every pair included."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import appearance_helper as AH

pytestmark = pytest.mark.gpu

FACTOR = 4.0
ULP = 2.0 ** -23
DEV = "cuda:0"
QUANTITIES = ("out", "v_features", "v_dirs") + AH.KEYS


def _module(state, n, module_degree):
    import hunyuanworld_mirror_amd as wm
    m = wm.AppearanceOptModule(n, AH.FEATURE_DIM, AH.EMBED_DIM, module_degree)
    m.load_state_dict({k: torch.as_tensor(v) for k, v in state.items()})
    return m.to(DEV)


def _gpu(state, features, ids, dirs, v_out, degree, module_degree=3):
    """-> dict over QUANTITIES as CPU fp32 tensors, through the public module and autograd (embeds.weight: zeros where autograd gives None)"""
    m = _module(state, state["embeds.weight"].shape[0], module_degree)
    f = features.to(DEV).requires_grad_(True)
    d = dirs.to(DEV).requires_grad_(True)
    out = m(f, None if ids is None else ids.to(DEV), d, degree)
    assert out.shape == dirs.shape and out.dtype == torch.float32
    out.backward(v_out.to(DEV))
    torch.cuda.synchronize()
    res = dict(out=out.detach().cpu(), v_features=f.grad.cpu(), v_dirs=d.grad.cpu())
    for k, p in m.named_parameters():
        res[k] = torch.zeros(p.shape) if p.grad is None else p.grad.cpu()
    return res


def _check(tag, got, ref, f32):
    """got (GPU), ref (fp64), f32 (helper fp32): dicts over QUANTITIES.  Prints every ratio, then asserts."""
    fails = []
    for k in QUANTITIES:
        assert torch.isfinite(got[k]).all(), (tag, k)
        r = np.asarray(ref[k], np.float64)
        if not r.any():
            assert not got[k].any(), (tag, k, "the reference is exactly zero")
            continue
        yard = max(AH.max_rel(f32[k].numpy(), r), ULP)
        err = AH.max_rel(got[k].numpy(), r)
        print(f"{tag} {k}: yardstick {yard:.3e} gpu {err:.3e} ratio {err / yard:.2f}")
        if not err <= FACTOR * yard:
            fails.append((tag, k, yard, err))
    assert not fails, fails


@functools.lru_cache(maxsize=None)
def _golden(name):
    z = AH.load_golden(name)
    state = {k[6:]: torch.from_numpy(v) for k, v in z.items() if k.startswith("state.")}
    t = dict(state=state, features=torch.from_numpy(z["features"]), dirs=torch.from_numpy(z["dirs"]), v_out=torch.from_numpy(z["v_out"]),
             ids=torch.from_numpy(z["embed_ids"]) if bool(z["has_ids"]) else None, degree=int(z["degree"]))
    ref = {k: z[k] for k in ("out", "v_features", "v_dirs")}
    ref.update({k: z["grad." + k] for k in AH.KEYS})
    f32 = AH.gradients(state, t["features"], t["ids"], t["dirs"], t["v_out"], t["degree"], torch.float32)
    return t, ref, f32


@functools.lru_cache(maxsize=None)
def _scene(n, C_, N, module_degree, degree, ids):
    sc = AH.random_scene(n, C_, N, module_degree, degree, ids, seed0=7000 + N, redraw=True)
    lo, err = AH.relu_margin(sc["state"], sc["features"], sc["ids"], sc["dirs"], degree)
    assert lo >= 16 * err
    ref = AH.gradients(sc["state"], sc["features"], sc["ids"], sc["dirs"], sc["v_out"], degree, torch.float64)
    f32 = AH.gradients(sc["state"], sc["features"], sc["ids"], sc["dirs"], sc["v_out"], degree, torch.float32)
    return sc, {k: v.numpy() for k, v in ref.items()}, f32


def _run_scene(sc, module_degree=3):
    return _gpu(sc["state"], sc["features"], sc["ids"], sc["dirs"], sc["v_out"], sc["degree"], module_degree)


# ------------------------------------------------------------------ 1. the reference's numbers
@pytest.mark.parametrize("name", ["a", "b"])
def test_gpu_matches_the_reference_goldens(name):
    t, ref, f32 = _golden(name)
    got = _gpu(t["state"], t["features"], t["ids"], t["dirs"], t["v_out"], t["degree"])
    _check(f"golden {name}", got, ref, f32)


# ------------------------------------------------------------------ 2. extra shapes
def _ids(C_, n):
    return tuple((2 * c + 1) % n for c in range(C_))


# (n, C, N, module degree, call degree, ids): one Gaussian; the 32-Gaussian wave and 64 around their seams; several block tiles with a
# partial last one; every call degree; a module of degree 2 and 0; embed_ids None
EXTRA = [(3, C_, N, 3, L, _ids(C_, 3)) for N in (1, 63, 64, 65, 1000) for C_, L in ((1, 3), (4, N % 4))]
EXTRA += [(3, 1, 65, 3, 0, (2,)), (3, 4, 63, 3, 2, (0, 0, 2, 1)), (3, 4, 64, 3, 1, None), (4, 2, 130, 2, 2, (3, 3)), (2, 2, 40, 2, 1, (1, 0)),
          (2, 3, 33, 0, 0, (0, 1, 0))]


@pytest.mark.parametrize("case", EXTRA, ids=[f"n{c[0]}-C{c[1]}-N{c[2]}-deg{c[3]}at{c[4]}-{'ids' if c[5] else 'noids'}" for c in EXTRA])
def test_gpu_matches_the_helper_on_extra_shapes(case):
    sc, ref, f32 = _scene(*case)
    got = _run_scene(sc, module_degree=case[3])
    _check(str(case[:5]), got, ref, f32)


def test_gpu_persistent_grid_with_several_tiles_per_block():
    """N just over 2 x MAX_BLOCKS x TILE Gaussians: the backward's grid is more than one block and its blocks walk more than one tile
    (two, and the last block one full and one partial tile)"""
    from hunyuanworld_mirror_amd import appearance as A, _lib
    N = 2 * A.MAX_BLOCKS * A.TILE - 3 * A.TILE + 37
    tiles = -(-N // A.TILE)
    # the grid the library itself plans for this N, read back from its workspace size (blocks x (7428 + 256 C) floats + two fixed parts)
    al = lambda x: (x + 255) // 256 * 256
    rest = _lib.lib().wm_appearance_backward_workspace_bytes(N, 2) - al(7428 * 4) - al(2 * 64 * 4)
    blocks = [b for b in range(1, 4097) if al(b * 7428 * 4) + al(b * 4 * 2 * 64 * 4) == rest]
    assert len(blocks) == 1 and 1 < blocks[0] < tiles and -(-tiles // blocks[0]) == 2, (blocks, tiles)
    sc, ref, f32 = _scene(3, 2, N, 3, 3, (2, 0))
    got = _run_scene(sc)
    _check(f"N = {N}", got, ref, f32)


# ------------------------------------------------------------------ 3. exactness
def test_gpu_unused_bands_and_unused_embeddings_get_exact_zeros():
    t, ref, f32 = _golden("a")
    got = _gpu(t["state"], t["features"], t["ids"], t["dirs"], t["v_out"], 1)          # module degree 3 called at degree 1
    w1 = got["color_head.0.weight"]
    assert not w1[:, 48 + 4:].any() and w1[:, 48:52].abs().sum() > 0 and w1[:, :48].abs().sum() > 0
    emb = got["embeds.weight"]
    assert not emb[[1, 2, 3]].any() and emb[0].abs().sum() > 0 and emb[4].abs().sum() > 0       # ids [4, 0, 4]
    full = _gpu(t["state"], t["features"], t["ids"], t["dirs"], t["v_out"], 3)
    assert full["color_head.0.weight"][:, 52:].abs().sum() > 0


def test_gpu_no_ids_is_a_zero_embedding():
    t, ref, f32 = _golden("b")
    m = _module(t["state"], 5, 3)
    f, d = t["features"].to(DEV).requires_grad_(True), t["dirs"].to(DEV)
    out = m(f, None, d, 1)
    out.backward(t["v_out"].to(DEV))
    assert m.embeds.weight.grad is None or not m.embeds.weight.grad.any()
    zero = dict(t["state"])
    zero["embeds.weight"] = torch.zeros_like(zero["embeds.weight"])
    m0 = _module(zero, 5, 3)
    with torch.no_grad():
        out0 = m0(t["features"].to(DEV), torch.tensor([3, 1], device=DEV), d, 1)
    assert torch.equal(out0, out.detach())


def test_gpu_zero_direction_has_a_finite_gradient():
    t, ref, f32 = _golden("a")
    dirs = t["dirs"].clone()
    dirs[1, 7] = 0.0
    dirs[0, 299] = 0.0
    got = _gpu(t["state"], t["features"], t["ids"], dirs, t["v_out"], 3)
    assert all(torch.isfinite(v).all() for v in got.values())


def test_gpu_device_id_out_of_range_is_a_zero_embedding_without_gradient():
    """ids are read on the device, without a host synchronisation: where nn.Embedding would trip a device-side assert, an id outside [0, n)
    reads a zero embedding and adds nothing to embeds.weight.grad; the other cameras are untouched"""
    t, ref, f32 = _golden("a")
    m = _module(t["state"], 5, 3)
    f, d, v = t["features"].to(DEV), t["dirs"].to(DEV), t["v_out"].to(DEV)
    for bad in (5, -1, 2 ** 31 - 1, 2 ** 32 + 1):           # the last would wrap to 1 if it were narrowed unclamped
        m.zero_grad()
        out = m(f, torch.tensor([4, bad, 4], device=DEV), d, 3)
        out.backward(v)
        g_bad = {k: p_.grad.clone() for k, p_ in m.named_parameters()}
        zero = dict(t["state"])
        zero["embeds.weight"] = zero["embeds.weight"].clone()
        zero["embeds.weight"][0] = 0.0
        m0 = _module(zero, 5, 3)
        out0 = m0(f, torch.tensor([4, 0, 4], device=DEV), d, 3)                   # camera 1 on a row of zeros: the same output
        out0.backward(v)
        assert torch.isfinite(out).all() and torch.equal(out, out0)
        alone = _module(t["state"], 5, 3)
        alone(f, torch.tensor([4, 4], device=DEV), d[[0, 2]].contiguous(), 3).backward(v[[0, 2]].contiguous())
        assert not g_bad["embeds.weight"][:4].any() and torch.equal(g_bad["embeds.weight"], alone.embeds.weight.grad)
        for k, p_ in m0.named_parameters():
            if k != "embeds.weight":
                assert torch.equal(g_bad[k], p_.grad), k


# ------------------------------------------------------------------ 4. reproducibility
@pytest.mark.parametrize("name", ["a", "b"])
def test_gpu_bitwise_reproducible_and_one_forward(name):
    t, _, _ = _golden(name)
    first = _gpu(t["state"], t["features"], t["ids"], t["dirs"], t["v_out"], t["degree"])
    again = _gpu(t["state"], t["features"], t["ids"], t["dirs"], t["v_out"], t["degree"])
    assert all(torch.equal(first[k], again[k]) for k in QUANTITIES)
    m = _module(t["state"], 5, 3)
    ids = None if t["ids"] is None else t["ids"].to(DEV)
    with torch.no_grad():
        plain = m(t["features"].to(DEV), ids, t["dirs"].to(DEV), t["degree"])
    assert plain.grad_fn is None and torch.equal(plain.cpu(), first["out"])


# ------------------------------------------------------------------ 5. surface
def test_gpu_surface_strides_dtypes_and_state_dict():
    import hunyuanworld_mirror_amd as wm
    t, _, _ = _golden("a")
    base = _gpu(t["state"], t["features"], t["ids"], t["dirs"], t["v_out"], 3)
    m = _module(t["state"], 5, 3)
    # non-contiguous views of the same values, ids as a list / int64 / CPU tensor
    f_view = t["features"].t().contiguous().to(DEV).t()
    d_view = t["dirs"].permute(2, 0, 1).contiguous().to(DEV).permute(1, 2, 0)
    assert not f_view.is_contiguous() and not d_view.is_contiguous()
    for ids in ([4, 0, 4], t["ids"], t["ids"].to(DEV), t["ids"].to(DEV).int()):
        with torch.no_grad():
            assert torch.equal(m(f_view, ids, d_view, 3).cpu(), base["out"])
    # fp64 inputs: computed in fp32, gradients come back in the inputs' dtype
    f64 = t["features"].double().to(DEV).requires_grad_(True)
    d64 = t["dirs"].double().to(DEV).requires_grad_(True)
    out = m(f64, [4, 0, 4], d64, 3)
    out.backward(t["v_out"].to(DEV))
    assert torch.equal(out.detach().cpu(), base["out"]) and f64.grad.dtype == torch.float64 and d64.grad.dtype == torch.float64
    assert torch.equal(f64.grad.float().cpu(), base["v_features"]) and torch.equal(d64.grad.float().cpu(), base["v_dirs"])
    # the state dict round trip, as a trainer checkpoint's app_module entry
    m2 = wm.AppearanceOptModule(5, 32, 16, 3)
    m2.load_state_dict({k: v.cpu() for k, v in m.state_dict().items()})
    with torch.no_grad():
        assert torch.equal(m2.to(DEV)(t["features"].to(DEV), [4, 0, 4], t["dirs"].to(DEV), 3).cpu(), base["out"])
    # guards
    with pytest.raises(RuntimeError):
        m(t["features"], [4, 0, 4], t["dirs"].to(DEV), 3)
    with pytest.raises(RuntimeError):
        wm.AppearanceOptModule(5, 32)(t["features"].to(DEV), [4, 0, 4], t["dirs"].to(DEV), 3)        # the module on the CPU
    with pytest.raises(IndexError):
        m(t["features"].to(DEV), [4, 0, 5], t["dirs"].to(DEV), 3)
    with pytest.raises(ValueError):
        m(t["features"].to(DEV), [4, 0], t["dirs"].to(DEV), 3)


def test_gpu_c_abi_refuses_a_small_workspace_before_launching():
    from hunyuanworld_mirror_amd import _lib
    L = _lib.lib()
    t, _, _ = _golden("a")
    st = {k: v.to(DEV).contiguous() for k, v in t["state"].items()}
    f, d, v = t["features"].to(DEV), t["dirs"].to(DEV), t["v_out"].to(DEV)
    ids = t["ids"].to(DEV).int()
    Cn, N = d.shape[:2]
    p = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    need = L.wm_appearance_backward_workspace_bytes(N, Cn)
    assert need > 0 and L.wm_appearance_backward_workspace_bytes(0, Cn) == 0
    outs = [torch.full_like(x, 7.0) for x in (f, d, st["embeds.weight"], st["color_head.0.weight"], st["color_head.0.bias"], st["color_head.2.weight"],
                                              st["color_head.2.bias"], st["color_head.4.weight"], st["color_head.4.bias"])]
    ws = torch.empty(need, device=DEV, dtype=torch.uint8)
    head = (p(f), p(st["embeds.weight"]), 5, p(ids), p(d), p(st["color_head.0.weight"]), p(st["color_head.0.bias"]), p(st["color_head.2.weight"]),
            p(st["color_head.2.bias"]), p(st["color_head.4.weight"]), p(st["color_head.4.bias"]), N, Cn)
    grads = tuple(p(o) for o in outs)
    assert L.wm_appearance_backward(*head, 3, 3, p(v), *grads, p(ws), need - 1, None) == 1
    assert L.wm_appearance_backward(*head, 3, 4, p(v), *grads, p(ws), need, None) == 1            # call degree above the module's
    assert L.wm_appearance_backward(*head, 4, 3, p(v), *grads, p(ws), need, None) == 1
    out = torch.full_like(d, 7.0)
    assert L.wm_appearance_forward(*head[:11], 0, Cn, 3, 3, p(out), None) == 1
    assert L.wm_appearance_forward(*head, 2, 3, p(out), None) == 1
    torch.cuda.synchronize()
    assert all(bool((o == 7.0).all()) for o in outs) and bool((out == 7.0).all())
    assert L.wm_appearance_backward(*head, 3, 3, p(v), *grads, p(ws), need, None) == 0
    torch.cuda.synchronize()
    base = _gpu(t["state"], t["features"], t["ids"], t["dirs"], t["v_out"], 3)
    assert torch.equal(outs[0].cpu(), base["v_features"]) and torch.equal(outs[3].cpu(), base["color_head.0.weight"])
    assert torch.equal(outs[2].cpu(), base["embeds.weight"])


# ------------------------------------------------------------------ 7. in the loop
def test_gpu_app_opt_in_the_optimisation_loop():
    """10 steps of the trainer's --app_opt branch from this library's own pieces: dirs = means - campos, colours = sigmoid(app(features,
    ids, dirs, degree) + colors) [C,N,3] -> rasterize_splats(sh_degree=None, return_info=True) -> photometric_loss -> DefaultStrategy
    with one refinement -> Adam per parameter plus the module's two groups.  No numeric bound beyond: every gradient finite, features
    follows N through the refinement, the loss falls, color_head.0.weight.grad is not zero."""
    import hunyuanworld_mirror_amd as wm
    g = torch.Generator().manual_seed(21)
    N, W, H = 150, 64, 48
    u = lambda *s: torch.rand(*s, generator=g)
    means = torch.cat([(u(N, 2) - 0.5) * torch.tensor([2.4, 1.8]), 2.0 + 1.5 * u(N, 1)], 1)
    vm = torch.eye(4).repeat(2, 1, 1)
    vm[1, :3, :3] = torch.tensor([[np.cos(0.15), 0, np.sin(0.15)], [0, 1, 0], [-np.sin(0.15), 0, np.cos(0.15)]], dtype=torch.float32)
    vm[1, :3, 3] = torch.tensor([0.2, -0.05, 0.1])
    c2w, Ks = torch.linalg.inv(vm).to(DEV), torch.tensor([[50.0, 0, W / 2], [0, 50.0, H / 2], [0, 0, 1]]).repeat(2, 1, 1).to(DEV)
    true = dict(means=means, quats=torch.randn(N, 4, generator=g), scales=torch.exp(-2.6 + 1.2 * u(N, 3)), opacities=0.2 + 0.6 * u(N))
    rz = wm.Rasterizer()
    with torch.no_grad():
        f = lambda k: true[k].to(DEV)
        target = rz.rasterize_splats(f("means"), f("quats"), f("scales"), f("opacities"), (0.15 + 0.7 * u(2, N, 3)).to(DEV), c2w, Ks, W, H, sh_degree=None)[0]
    params = torch.nn.ParameterDict({"means": means + 0.03 * torch.randn(N, 3, generator=g), "scales": torch.log(true["scales"]), "quats": true["quats"].clone(),
                                     "opacities": torch.logit(true["opacities"]), "colors": torch.zeros(N, 3),
                                     "features": 0.5 * torch.randn(N, 32, generator=g)}).to(DEV)
    torch.manual_seed(3)
    app = wm.AppearanceOptModule(4, 32, 16, 3).to(DEV)
    opts = {k: torch.optim.Adam([params[k]], lr=2e-2) for k in params}
    app_opts = [torch.optim.Adam(app.embeds.parameters(), lr=1e-2), torch.optim.Adam(app.color_head.parameters(), lr=1e-2)]
    strat = wm.DefaultStrategy(refine_start_iter=0, refine_every=5, refine_stop_iter=9, grow_grad2d=0.012, absgrad=False, verbose=False)
    strat.check_sanity(params, opts)
    state = strat.initialize_state(scene_scale=10.0)
    gen = torch.Generator(device=DEV).manual_seed(1)
    ids = torch.tensor([3, 1], device=DEV)
    sizes, losses, w_grad = [], [], []
    for step in range(10):
        dirs = params["means"][None, :, :] - c2w[:, None, :3, 3]
        colors = torch.sigmoid(app(params["features"], ids, dirs, min(step // 3, 3)) + params["colors"])
        assert colors.shape == (2, len(params["means"]), 3)
        rgb, _, _, info = rz.rasterize_splats(params["means"], params["quats"], torch.exp(params["scales"]), torch.sigmoid(params["opacities"]),
                                              colors, c2w, Ks, W, H, sh_degree=None, return_info=True, absgrad=False)
        loss = wm.photometric_loss(rgb, target, 0.2, "valid")[0]
        strat.step_pre_backward(params, opts, state, step, info)
        for o in list(opts.values()) + app_opts:
            o.zero_grad()
        loss.backward()
        for k in params:
            assert params[k].grad is not None and params[k].grad.shape == params[k].shape and bool(torch.isfinite(params[k].grad).all()), (step, k)
        for k, p_ in app.named_parameters():
            assert p_.grad is not None and bool(torch.isfinite(p_.grad).all()), (step, k)
        w_grad.append(float(app.color_head[0].weight.grad.abs().sum()))
        losses.append(float(loss.detach()))
        for o in list(opts.values()) + app_opts:
            o.step()
        strat.step_post_backward(params, opts, state, step, info, generator=gen)
        sizes.append(len(params["means"]))
        assert params["features"].shape == (sizes[-1], 32) and params["colors"].shape == (sizes[-1], 3)
    print("N per step", sizes, "loss", losses, "sum |color_head.0.weight.grad|", w_grad)
    assert len(set(sizes)) > 1 and all(x > 0 for x in w_grad) and losses[-1] < losses[0]
