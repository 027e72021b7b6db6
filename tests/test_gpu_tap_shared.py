"""GPU: the DPT heads' shared tap front (tuning tap_shared, default 1) against the direct form (tap_shared = 0) and fp64.

Direct form, per head:   P_h = round16(xhat * gamma_h + beta_h) @ round16(W_h)^T + b_h + pos
Shared form, all heads:  P_h = round16(xhat) @ round16(W_h diag(gamma_h))^T + (b_h + W_h beta_h) + pos     (one LayerNorm, one GEMM)
with xhat = the LayerNorm of the tap's patch rows without affine.  The reference is the reference's own formula in torch fp64,
LayerNorm(2D, affine) -> Linear -> + pos_embed (dense_head.py:53,204-208), restated here.

Op level (wm_op_dpt_tap_front runs either form on host weights): rel-L2 against fp64 of both forms on the same inputs, gamma ~ N(1, 0.3),
beta ~ N(0, 0.3) so that the fold is no no-op.  One operand's rounding moved and none was added, so the shared form is held to twice the
direct form's error as MEASURED on MI355X (BOUND below = 2 x the direct form's largest rel-L2 over the cases of a type; measured values
in profiles/r12_tap_shared.md); each head's slice must also be bit-identical to the same launch made for that head alone.
Forward level: tap_shared 1 against 0 on three golden fixtures, each within the golden gate of tests/test_gpu_e2e.py, deterministic; and
a handle whose folded weight overflows f16 runs the direct form (bit-identical to tap_shared = 0).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import load_golden, rel_l2
from test_gpu_ops_frontend import BF16, F16, _lib, _p, _rel, _stream, _tdt, dev  # noqa: F401  (dev: module-scoped device fixture)

pytestmark = pytest.mark.gpu

# 2 x the direct form's rel-L2 against fp64, the largest over this file's op-level cases of the type (measured on MI355X:
# profiles/r12_tap_shared.md).  An fp16 operand carries 2^-11 relative rounding, a bf16 one 2^-8: the measured values sit there.
DIRECT_MEASURED = {F16: 3.636e-4, BF16: 2.938e-3}
BOUND = {k: 2 * v for k, v in DIRECT_MEASURED.items()}

PSI = 7   # special rows in front of the patch rows of every view (camera, 4 registers, 2 prior tokens)


def _inputs(n, hw, D2, oc, nh, seed):
    g = torch.Generator().manual_seed(seed)
    P = PSI + hw
    tap = torch.randn(n, P, D2, generator=g) * 2 + 0.5
    tap[:, :PSI] = 1.0e6                                   # special rows: a wrong row map shows
    gam = [1 + 0.3 * torch.randn(D2, generator=g) for _ in range(nh)]
    bet = [0.3 * torch.randn(D2, generator=g) for _ in range(nh)]
    Wp = [torch.randn(oc, D2, generator=g) / D2 ** 0.5 for _ in range(nh)]
    bp = [0.1 * torch.randn(oc, generator=g) for _ in range(nh)]
    pos = 0.1 * torch.randn(hw, oc, generator=g)
    return tap, gam, bet, Wp, bp, pos


def _ref64(tap, gam, bet, Wp, bp, pos, hw):
    x = tap[:, PSI:PSI + hw].double()
    out = []
    for g_, b_, W_, c_ in zip(gam, bet, Wp, bp):
        y = torch.nn.functional.layer_norm(x, (x.shape[-1],), g_.double(), b_.double(), 1e-5)
        out.append((y @ W_.double().t() + c_.double() + pos.double()).reshape(-1, W_.shape[0]))
    return out


def _ptrs(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _front(dev, dt, tap_d, gam, bet, Wp, bp, pos_d, hw, out16, shared, heads=None):
    """wm_op_dpt_tap_front for the heads `heads` (default: all); returns (outputs as float tensors on the CPU, raw bits, ran_shared)"""
    L = _lib()
    idx = list(range(len(gam))) if heads is None else heads
    n, P, D2 = tap_d.shape
    oc = Wp[0].shape[0]
    outs = [torch.zeros(n * hw, oc, dtype=_tdt(dt) if out16 else torch.float32, device=dev) for _ in idx]
    ran = C.c_int(-1)
    st = L.wm_op_dpt_tap_front(dt, _p(tap_d), n, P, PSI, hw, D2, len(idx), oc, _ptrs([gam[i] for i in idx]), _ptrs([bet[i] for i in idx]),
                               _ptrs([Wp[i] for i in idx]), _ptrs([bp[i] for i in idx]), _p(pos_d), out16, shared, _ptrs(outs), C.byref(ran),
                               _stream())
    assert st == 0, st
    torch.cuda.synchronize()
    bits = [o.view(torch.int16 if out16 else torch.int32).cpu() for o in outs]
    return [o.float().cpu() for o in outs], bits, ran.value


# (n views, hw, D2, the four taps' widths): the tiny configuration at 70 px (5 x 5 tokens), the full width at 2 views x 70 x 56 (hw = 20:
# 40 rows, far below one row tile: the masked last band and the row map), and the full width on 14 views (280 rows: two row tiles of
# the ping-pong kernel, the second one partial and not a multiple of its 16-row units)
SHAPES = {"tiny70": (2, 25, 256, (64, 128, 256, 256)), "full70x56": (2, 20, 2048, (256, 512, 1024, 1024)),
          "full14v": (14, 20, 2048, (256, 512, 1024, 1024))}
CASES = [("tiny70", 3, F16, -1), ("tiny70", 4, F16, -1), ("tiny70", 3, BF16, -1), ("tiny70", 4, BF16, -1),
         ("full70x56", 3, F16, -1), ("full70x56", 4, F16, -1), ("full70x56", 3, BF16, -1), ("full70x56", 4, BF16, -1),
         ("full70x56", 3, F16, 4), ("full14v", 3, F16, 4), ("full14v", 4, BF16, 5)]   # gemm_cfg 4 / 5: the ping-pong kernel's epilogue


@pytest.mark.parametrize("shape,nh,dt,cfg", CASES)
def test_tap_front_op_against_fp64(dev, shape, nh, dt, cfg):
    n, hw, D2, ocs = SHAPES[shape]
    L = _lib()
    worst_direct = 0.0
    if cfg >= 0:
        assert L.wm_set_tuning(b"gemm_cfg", cfg) == 0
    try:
        for i, oc in enumerate(ocs):
            out16 = 1 if i < 2 else 0
            tap, gam, bet, Wp, bp, pos = _inputs(n, hw, D2, oc, nh, 1000 * i + 10 * nh + dt)
            ref = _ref64(tap, gam, bet, Wp, bp, pos, hw)
            tap_d, pos_d = tap.to(dev), pos.to(dev)
            direct, _, ran0 = _front(dev, dt, tap_d, gam, bet, Wp, bp, pos_d, hw, out16, 0)
            shared, sbits, ran1 = _front(dev, dt, tap_d, gam, bet, Wp, bp, pos_d, hw, out16, 1)
            assert ran0 == 0 and ran1 == 1
            for k in range(nh):
                ed, es = _rel(direct[k], ref[k]), _rel(shared[k], ref[k])
                print(f"{shape} nh {nh} dt {dt} cfg {cfg} tap {i} head {k}: direct {ed:.3e} shared {es:.3e}")
                worst_direct = max(worst_direct, ed)
                assert np.isfinite(es) and np.isfinite(ed)
                assert ed <= BOUND[dt], (i, k, ed)
                assert es <= BOUND[dt], (i, k, es, BOUND[dt])
                # concatenation changes nothing: the head's slice = the same launch for that head alone, bit for bit
                _, alone, ran = _front(dev, dt, tap_d, gam, bet, Wp, bp, pos_d, hw, out16, 1, heads=[k])
                assert ran == 1 and torch.equal(alone[0], sbits[k]), (i, k)
    finally:
        if cfg >= 0:
            L.wm_set_tuning(b"gemm_cfg", -1)
    print(f"{shape} nh {nh} dt {dt} cfg {cfg}: worst direct {worst_direct:.3e}")


def test_tap_front_op_range_fallback(dev):
    """gamma scaled so that W diag(gamma) overflows f16 (|W gamma| = 1e5 in one element, every operand of the direct form in range):
    the op runs the direct form, bit-identical to shared = 0; the same weights in bf16 are in range and take the shared form."""
    n, hw, D2, oc = 2, 20, 2048, 256
    tap, gam, bet, Wp, bp, pos = _inputs(n, hw, D2, oc, 3, 77)
    gam[1][5] = 1000.0
    Wp[1][3, 5] = 100.0
    tap_d, pos_d = tap.to(dev), pos.to(dev)
    _, b0, ran0 = _front(dev, F16, tap_d, gam, bet, Wp, bp, pos_d, hw, 0, 0)
    _, b1, ran1 = _front(dev, F16, tap_d, gam, bet, Wp, bp, pos_d, hw, 0, 1)
    assert ran0 == 0 and ran1 == 0
    for a, b in zip(b0, b1):
        assert torch.equal(a, b)
    assert _front(dev, BF16, tap_d, gam, bet, Wp, bp, pos_d, hw, 0, 1)[2] == 1


def _forward_both(m, views, flags):
    from test_gpu_e2e import _run
    L = _lib()
    res = {}
    for v in (1, 0, 1):
        assert L.wm_set_tuning(b"tap_shared", v) == 0
        try:
            got = _run(m, views, flags)
        finally:
            L.wm_set_tuning(b"tap_shared", -1)
        got = {k: got[k].clone() for k in ("pts3d", "depth", "normals", "camera_params")}
        if v in res:   # the second run of the shared form: deterministic from run to run
            for k in got:
                assert torch.equal(got[k].view(torch.int32), res[v][k].view(torch.int32)), k
        res[v] = got
    return res


@pytest.mark.parametrize("name", ["tiny_3v_70x56_pose_ray", "tiny_12v_56x70_allpriors", "full_2v_224_noprior"])
def test_forward_shared_against_direct(name):
    """tap_shared 1 against 0 through the whole forward (12 views: two view chunks).  Each form passes the golden gate of
    tests/test_gpu_e2e.py (GROSS on the dense outputs) and the two agree within it; the camera head does not see the change."""
    from test_gpu_e2e import GROSS, _cached_model
    cfg, views, flags, outs, z = load_golden(name)
    res = _forward_both(_cached_model(cfg), views, flags)
    sub = int(z["subsample"]) if "subsample" in z else 1
    assert torch.equal(res[0]["camera_params"], res[1]["camera_params"])
    for k in ("pts3d", "depth", "normals"):
        errs = []
        for v in (0, 1):
            g = res[v][k].cpu().numpy()
            if sub > 1 and g.ndim >= 4 and g.shape[2] == views["img"].shape[-2]:
                g = g[:, :, ::sub, ::sub]
            errs.append(rel_l2(g, outs[k]))
        e = rel_l2(res[1][k].cpu().numpy(), res[0][k].cpu().numpy())
        print(f"{name} {k}: direct vs golden {errs[0]:.2e}, shared vs golden {errs[1]:.2e}, shared vs direct {e:.2e}")
        assert errs[0] < GROSS and errs[1] < GROSS and 0 < e < GROSS, (k, errs, e)


def test_forward_range_fallback():
    """A handle whose depth head's folded weight overflows f16 (gamma[5] = 1000 against projects.2.weight[3, 5] = 100) keeps the whole
    group on the direct form: tap_shared = 1 is then bit-identical to tap_shared = 0 on every head's output (compared as bit patterns:
    the 1e5-sized feature this produces may overflow the f16 operands behind it in both runs alike)."""
    from hunyuanworld_mirror_amd import WorldMirror
    from test_gpu_e2e import _run
    cfg, views, flags, outs, z = load_golden("tiny_3v_70x56_pose_ray")
    m = WorldMirror(arch=cfg).init_synthetic_weights()
    g = np.array(m._host_weights["depth_head.norm.weight"], dtype=np.float32, copy=True)
    w = np.array(m._host_weights["depth_head.projects.2.weight"], dtype=np.float32, copy=True)
    g[5] = 1000.0
    w[3, 5] = 100.0
    m._host_weights["depth_head.norm.weight"] = g
    m._host_weights["depth_head.projects.2.weight"] = w
    m = m.to("cuda:0")
    L = _lib()
    res = {}
    for v in (1, 0):
        assert L.wm_set_tuning(b"tap_shared", v) == 0
        try:
            got = _run(m, views, flags)
        finally:
            L.wm_set_tuning(b"tap_shared", -1)
        res[v] = {k: got[k].clone() for k in ("pts3d", "depth", "normals", "pts3d_conf", "depth_conf", "normals_conf")}
    for k in res[0]:
        assert torch.equal(res[0][k].view(torch.int32), res[1][k].view(torch.int32)), k
