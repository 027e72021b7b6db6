"""GPU: operator-level parity of the kernels AROUND the GEMM / attention / conv kernels of test_gpu_ops.py — the token front end
(im2col, special-token rows, the row-remapping and pixel-shuffle GEMM epilogues, the remapped LayerNorm, bilinear resize with the
position tables, copy2d) and the fp32 camera head (small_attention, adaln, cam_update, cam_matrices, linear_f32) — each through its
own wm_op_* entry point.

Rules every test here follows:
  * reference = plain torch in fp64 on the operands the kernel reads (16-bit operands rounded first, then widened);
  * every output lives in a canvas pre-filled with a NaN bit pattern, with a guard band of at least one row on either side: after
    the launch every element that must be written is written and every element that must not be still holds the pattern;
  * kernels that only move or round data are held to BIT equality; the GEMM epilogues to bit equality with the WM_EPI_F32 epilogue
    of the same tile configuration (itself < 2e-5 relative L2 of fp64) followed by the epilogue's single fp32 operations in torch;
  * kernels with an fp32 reduction or a transcendental have no tolerance fixed in advance: the same operation in torch fp32 on the
    CPU gives e_ref against fp64 (max-abs error / max-abs of the fp64 result; for 16-bit outputs the number of elements whose
    rounded value differs from the rounded fp64 value, and no element off by more than one 16-bit ulp: see _yard16 for how the ulp
    is taken on elements that cancel to nearly zero), and the kernel's error, measured the same way, must be <= 4 e_ref (floors:
    4 * 2^-23, 8 elements).  Each such test prints "e_kernel ... e_ref ..."; the docstrings quote what an MI355X gave.
"""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BF16, F16 = 0, 1
SENT32 = 0x7FC5A5A5   # a quiet NaN no fp32 operation produces
SENT16 = 0x7FC5       # a NaN both as bf16 and as f16


def _lib():
    from hunyuanworld_mirror_amd import _lib
    return _lib.lib()


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _tdt(dt):
    return torch.bfloat16 if dt == BF16 else torch.float16


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp(min=1e-30))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _canvas(shape, dev, bits16=False):
    """(full, body, guard): `body` (int32 / int16, shape `shape`) sits between two guard bands of >= one row (the last dim)."""
    n = math.prod(shape)
    g = (max(shape[-1], 64) + 63) // 64 * 64
    full = torch.full((g + n + g,), SENT16 if bits16 else SENT32, dtype=torch.int16 if bits16 else torch.int32, device=dev)
    return full, full[g:g + n].view(shape), g


def _sent(t):
    return t == (SENT16 if t.dtype == torch.int16 else SENT32)


def _guards_intact(full, g):
    assert bool(_sent(full[:g]).all()) and bool(_sent(full[-g:]).all()), "a guard band was written"


def _written_exactly(body, mask):
    """`mask` (bool, broadcastable to body): True where the kernel must have written, False where the sentinel must remain."""
    s = _sent(body)
    m = mask.to(body.device).expand_as(body)
    assert not bool((s & m).any()), f"{int((s & m).sum())} elements that must be written still hold the sentinel"
    assert not bool((~s & ~m).any()), f"{int((~s & ~m).sum())} elements outside the kernel's region were written"


def _yard32(name, got, ref32, ref64):
    """fp32 result against the yardstick: max-abs error / max-abs of the fp64 result, kernel <= 4 x torch-fp32-on-CPU."""
    got, ref32, ref64 = got.detach().cpu().double(), ref32.detach().cpu().double(), ref64.detach().cpu()
    den = float(ref64.abs().max())
    ek, er = float((got - ref64).abs().max()) / den, float((ref32 - ref64).abs().max()) / den
    print(f"{name}: e_kernel {ek:.3e} e_ref {er:.3e}")
    assert math.isfinite(ek), name
    assert ek <= 4 * max(er, 2.0 ** -23), f"{name}: e_kernel {ek:.3e} > 4 x max(e_ref {er:.3e}, 2^-23)"
    return ek, er


def _ord16(bits):
    b = bits.to(torch.int32)
    return torch.where(b >= 0, b, -(b & 0x7FFF))   # sign-magnitude -> monotone, +0 == -0


def _yard16(name, got_bits, ref32, ref64, dt):
    """16-bit result: elements whose bits differ from the rounded fp64 value, kernel <= 4 x torch-fp32-on-CPU (floor 8), and no element
    off by more than one 16-bit ulp.  "One ulp" is taken on the VALUE: |got - round16(fp64)| <= spacing of the 16-bit format at that
    magnitude + the absolute error the fp32 yardstick allows the unrounded result (4 x max(torch-fp32 max-abs error, 2^-23 max|fp64|)).
    Counted on the bit patterns alone the assertion cannot hold for ANY fp32 evaluation: an element that cancels to nearly zero carries
    the fp32 error of its operands, which is many ulps of its own tiny magnitude (torch fp32 itself is up to 112 bf16 bit steps from the
    rounded fp64 LayerNorm); both bit-step maxima are printed.  For every element of ordinary magnitude the extra term is far below one
    16-bit ulp, so the check is the stated one there."""
    got_bits = got_bits.detach().cpu()
    ref32, ref64 = ref32.detach().cpu(), ref64.detach().cpu()
    r64 = ref64.to(_tdt(dt)).view(torch.int16)
    r32 = ref32.to(_tdt(dt)).view(torch.int16)
    nk, nr = int((got_bits != r64).sum()), int((r32 != r64).sum())
    steps_k, steps_r = int((_ord16(got_bits) - _ord16(r64)).abs().max()), int((_ord16(r32) - _ord16(r64)).abs().max())
    gv, rv = got_bits.view(_tdt(dt)).double(), r64.view(_tdt(dt)).double()
    assert bool(torch.isfinite(gv).all()), name
    mant = 7 if dt == BF16 else 10
    _, ex = torch.frexp(torch.maximum(gv.abs(), rv.abs()))                    # |x| = m 2^ex, m in [0.5, 1): spacing 2^(ex - 1 - mant)
    ulp = torch.ldexp(torch.ones_like(rv), ex - (1 + mant)).clamp(min=2.0 ** -24 if dt == F16 else 0.0)
    abs_tol = 4 * max(float((ref32.double() - ref64).abs().max()), 2.0 ** -23 * float(ref64.abs().max()))
    over = int(((gv - rv).abs() > ulp + abs_tol).sum())
    print(f"{name}: e_kernel {nk} / {got_bits.numel()} rounded differently (max {steps_k} bit steps) e_ref {nr} (max {steps_r} bit steps); "
          f"{over} elements beyond one 16-bit ulp + {abs_tol:.2e}")
    assert over == 0, f"{name}: {over} elements are more than one 16-bit ulp off"
    assert nk <= max(4 * nr, 8), f"{name}: {nk} mismatches > 4 x max(e_ref {nr}, 2)"
    return nk, nr


class _tuning:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        for k, v in self.kv.items():
            assert _lib().wm_set_tuning(k.encode(), v) == 0, k

    def __exit__(self, *exc):
        for k in self.kv:
            _lib().wm_set_tuning(k.encode(), -1)


# ------------------------------------------------------------------------------------------------------------------ im2col
def _patches(img, ps):
    N, Cc, H, W = img.shape
    gh, gw = H // ps, W // ps
    return img[:, :, :gh * ps, :gw * ps].reshape(N, Cc, gh, ps, gw, ps).permute(0, 2, 4, 1, 3, 5).reshape(N * gh * gw, Cc * ps * ps)


IM2COL_SHAPES = [
    (2, 3, 518, 518, 14, 640),    # product RGB patchify: input-indexed kernel, tail [588, 640)
    (3, 1, 154, 210, 14, 256),    # product depth-prior patchify (C = 1): input-indexed kernel, tail [196, 256)
    (1, 3, 56, 70, 14, 588),      # Kpad == K: no tail; input-indexed
    (2, 3, 75, 77, 7, 192),       # odd ps and W, H % ps != 0: OUTPUT-indexed kernel, bottom rows dropped
    (1, 3, 28, 30, 14, 640),      # W % ps != 0: right columns dropped; input-indexed
    (1, 3, 28, 2044, 14, 640),    # wide image, 57 232 B of LDS: input-indexed
    (1, 3, 14, 2340, 14, 640),    # ps * W * 2 = 65 520 B, the last even width within the launcher's 64 KiB condition: input-indexed
    (1, 3, 14, 2342, 14, 640),    # 65 576 B, just over it: output-indexed
]


@pytest.mark.parametrize("dt", [BF16, F16])
@pytest.mark.parametrize("shape,normalize", [(s, nz) for s in IM2COL_SHAPES for nz in (0, 1) if nz == 0 or s[1] == 3])
def test_im2col(dev, shape, normalize, dt):
    """wm_launch_im2col: im2col_rows_kernel (input-indexed; ps, W, K, Kpad even and ps * W * 2 <= 64 KiB) and im2col_kernel
    (output-indexed; the rest) — see IM2COL_SHAPES for which shape takes which.  normalize = 0 only rounds: bit equality.  normalize = 1
    ((x - mean) / std in fp32, then the rounding) goes by the yardstick.  Measured on MI355X: e_kernel == e_ref on every shape (one
    fp32 subtract and one correctly rounded divide: the same bits as torch), e.g. (2, 3, 518, 518, 14, 640): 6 of 1 609 944 elements
    round differently from fp64 in bf16, 46 in f16, for kernel and torch alike; never more than one bit step."""
    N, Cc, H, W, ps, Kpad = shape
    g = torch.Generator().manual_seed(H * 31 + W + normalize)
    img = torch.randn(N, Cc, H, W, generator=g) * 2 + 0.5   # well outside [0, 1], negative included
    K, rows = Cc * ps * ps, N * (H // ps) * (W // ps)
    full, body, gd = _canvas((rows, Kpad), dev, bits16=True)
    dimg = img.to(dev)   # a fresh allocation (the input-indexed kernel reads it with 8-byte loads), alive until the synchronize
    assert _lib().wm_op_im2col(dt, _p(dimg), _p(body), N, Cc, H, W, ps, Kpad, normalize, _stream()) == 0
    torch.cuda.synchronize()
    _guards_intact(full, gd)
    got = body.cpu()
    assert not bool(_sent(got).any()), "every element of [rows][Kpad] must be written"
    assert bool((got[:, K:] == 0).all()), "tail [K, Kpad) must be +0"
    pat = _patches(img, ps)
    if not normalize:
        assert torch.equal(got[:, :K], pat.to(_tdt(dt)).view(torch.int16))
        return
    mean = torch.tensor([0.485, 0.456, 0.406], dtype=torch.float32).repeat_interleave(ps * ps)
    std = torch.tensor([0.229, 0.224, 0.225], dtype=torch.float32).repeat_interleave(ps * ps)
    _yard16(f"im2col normalize {shape} dt{dt}", got[:, :K], (pat - mean) / std, (pat.double() - mean.double()) / std.double(), dt)


@pytest.mark.parametrize("dt", [BF16, F16])
@pytest.mark.parametrize("N,H,W,Kpad", [(2, 37, 41, 192), (1, 5, 3, 192), (1, 1, 9, 160), (3, 70, 56, 192)])
def test_im2col7(dev, N, H, W, Kpad, dt):
    """im2col7_kernel (one kernel, output-indexed): rows = pixels, column c*49 + ky*7 + kx of the zero-padded 7x7 window, zeros in
    [147, Kpad).  Only moves and rounds: bit equality with F.unfold.  The image is followed by 64 floats of a large value inside the
    same allocation, so that a border test that lets ix == W through reads a wrong VALUE, not memory past the tensor."""
    g = torch.Generator().manual_seed(H * 100 + W)
    buf = torch.full((N * 3 * H * W + 64,), 1.0e4)
    buf[:N * 3 * H * W] = torch.randn(N * 3 * H * W, generator=g) * 2 + 0.5
    img = buf[:N * 3 * H * W].view(N, 3, H, W)
    dbuf = buf.to(dev)
    full, body, gd = _canvas((N * H * W, Kpad), dev, bits16=True)
    assert _lib().wm_op_im2col7(dt, _p(dbuf), _p(body), N, H, W, Kpad, _stream()) == 0
    torch.cuda.synchronize()
    _guards_intact(full, gd)
    exp = torch.zeros(N * H * W, Kpad, dtype=_tdt(dt))
    exp[:, :147] = F.unfold(img, 7, padding=3).permute(0, 2, 1).reshape(N * H * W, 147).to(_tdt(dt))
    assert torch.equal(body.cpu(), exp.view(torch.int16))


# ------------------------------------------------------------------------------------------------------------------ token rows
def _table(shape, base):
    """distinct, exactly representable values per element: a wrong slot / token / view / channel index changes the result"""
    return (torch.arange(math.prod(shape), dtype=torch.float32) + base).view(shape)


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("R", [0, 4])
@pytest.mark.parametrize("D", [64, 1024])
def test_dino_tokens(dev, D, R, N):
    """dino_special_kernel: X[n][0] = cls + pos[0] (one fp32 add: bit equality), X[n][1..R] = reg; the hw patch rows keep the sentinel."""
    hw = 5
    T = 1 + R + hw
    cls, reg, pos = _table((D,), 0.25) * 0.5, _table((max(R, 1), D), 100000.0), _table((T, D), 7.5) * 0.25
    full, body, gd = _canvas((N, T, D), dev)
    dcls, dreg, dpos = cls.to(dev), reg.to(dev), pos.to(dev)
    assert _lib().wm_op_dino_tokens(None, _p(dcls), _p(dreg) if R else None, _p(dpos), _p(body), N, hw, R, D, _stream()) == 0
    torch.cuda.synchronize()
    _guards_intact(full, gd)
    mask = (torch.arange(T) < 1 + R).view(1, T, 1)
    _written_exactly(body, mask)
    exp = torch.cat([(cls + pos[0]).view(1, D), reg[:R]], 0).expand(N, 1 + R, D)
    assert torch.equal(body.cpu()[:, :1 + R].view(torch.float32), exp)


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("R", [0, 4])
@pytest.mark.parametrize("D", [64, 1024])
def test_vgt_special(dev, D, R, N):
    """vgt_special_kernel, every branch: cond 0 / 1, pose_tok / ray_tok NULL or not (independently), first_view_global 0 (view 0 takes
    slot 0, the others slot 1) and 3 (a later shard: no view takes slot 0).  The launcher's grid is sized for 3 + R rows per view while
    the kernel's grid-stride loop runs over psi = 1 + R + 2 cond rows: with cond = 0 the surplus blocks must write nothing (the patch
    rows and the guard bands keep the sentinel).  Pure data movement: bit equality."""
    L = _lib()
    cam, reg = _table((2, D), 0.0), _table((2, max(R, 1), D), 50000.0)
    pose, ray = _table((N, D), 200000.0), _table((N, D), 300000.0)
    dcam, dreg, dpose, dray = cam.to(dev), reg.to(dev), pose.to(dev), ray.to(dev)
    for cond in (0, 1):
        psi = 1 + R + 2 * cond
        P = psi + 3
        for has_pose in (0, 1):
            for has_ray in (0, 1):
                for fvg in (0, 3):
                    full, body, gd = _canvas((N, P, D), dev)
                    assert L.wm_op_vgt_special(_p(body), _p(dcam), _p(dreg) if R else None, _p(dpose) if has_pose else None,
                                               _p(dray) if has_ray else None, N, P, R, D, cond, fvg, _stream()) == 0
                    torch.cuda.synchronize()
                    tag = f"D{D} R{R} N{N} cond{cond} pose{has_pose} ray{has_ray} first_view_global{fvg}"
                    _guards_intact(full, gd)
                    _written_exactly(body, (torch.arange(P) < psi).view(1, P, 1))
                    exp = torch.empty(N, psi, D)
                    for n in range(N):
                        slot = 0 if fvg + n == 0 else 1
                        exp[n, 0] = cam[slot]
                        exp[n, 1:1 + R] = reg[slot, :R]
                        if cond:
                            exp[n, 1 + R] = pose[n] if has_pose else 0.0
                            exp[n, 2 + R] = ray[n] if has_ray else 0.0
                    assert torch.equal(body.cpu()[:, :psi].view(torch.float32), exp), tag


# ------------------------------------------------------------------------------------------------------------------ LayerNorm with row remapping
def _ln_inputs(n, hw, R, D, ld_in, seed):
    g = torch.Generator().manual_seed(seed)
    data = torch.randn(n, hw, D, generator=g) * 3 + 50    # offset rows: a one-pass variance would show
    data[..., 3] += 40
    Td = 1 + R + hw
    x = torch.full((n, Td, ld_in), 1.0e6)                   # special rows and the columns beyond D: a wrong row / pitch shows
    x[:, 1 + R:, :D] = data
    return data, x, torch.randn(D, generator=g), torch.randn(D, generator=g)


@pytest.mark.parametrize("n,hw,R,psi,D,ld_in,ld_out", [(8, 1369, 4, 7, 1024, 1024, 1024), (3, 25, 4, 5, 256, 256, 256), (1, 1, 0, 1, 128, 128, 128),
                                                       (2, 150, 4, 7, 2048, 2048, 2048), (3, 25, 4, 5, 256, 512, 320)])
def test_layernorm_remapped_f32(dev, n, hw, R, psi, D, ld_in, ld_out):
    """The product call of the final DINO norm: groups = n, rows_per_group = hw, in row g * Td + 1 + R + q -> out row g * P + psi + q,
    fp32 out: layernorm_kernel<NV> (the general kernel; fp32 output never takes the branch-free one).  Row counts 10952, 75, 1, 300:
    the last block of four rows is partial for 75 and 1.  Rows of the special tokens, rows of no group, columns [D, ld_out) and the guard
    bands keep the sentinel.  Measured on MI355X (e_kernel / e_ref): 3.8e-7 / 4.8e-7 (8 x 1369 x 1024), 4.6e-7 / 7.9e-7 (3 x 25 x 256, both
    pitches), 5.2e-8 / 2.1e-7 (1 x 1 x 128), 1.4e-7 / 2.5e-7 (2 x 150 x 2048)."""
    data, x, w, b = _ln_inputs(n, hw, R, D, ld_in, n * 1000 + D)
    Td, P = 1 + R + hw, psi + hw
    full, body, gd = _canvas((n, P, ld_out), dev)
    dx, dw, db = x.to(dev), w.to(dev), b.to(dev)
    assert _lib().wm_op_layernorm_rows(_p(dx), _p(body), _p(dw), _p(db), D, ld_in, ld_out, 1e-6, n, hw, Td, 1 + R, P, psi, 1, 0,
                                       _stream()) == 0
    torch.cuda.synchronize()
    _guards_intact(full, gd)
    mask = (torch.arange(P) >= psi).view(1, P, 1) & (torch.arange(ld_out) < D).view(1, 1, ld_out)
    _written_exactly(body, mask)
    got = body.cpu().view(torch.float32)[:, psi:, :D]
    _yard32(f"layernorm remapped f32 n{n} hw{hw} D{D} ld_in{ld_in} ld_out{ld_out}", got, F.layer_norm(data, (D,), w, b, 1e-6),
            F.layer_norm(data.double(), (D,), w.double(), b.double(), 1e-6))


@pytest.mark.parametrize("dt", [BF16, F16])
@pytest.mark.parametrize("D", [1024, 2048])
def test_layernorm_remapped_16bit(dev, D, dt):
    """The same remap with a 16-bit output at D = 1024 / 2048, affine: layernorm_fast_kernel<4 / 8> (branch-free, every load up front).
    Measured on MI355X, elements rounded differently from fp64, kernel / torch fp32: D = 1024: 121 / 128 of 307 200 (bf16), 839 / 901 (f16);
    D = 2048: 239 / 272 of 614 400 (bf16), 1538 / 1625 (f16).  Largest bit-pattern distance, on elements that cancel to nearly zero:
    112 / 112, 16 / 34, 22 / 94, 18 / 18 steps — torch fp32 as far off as the kernel, see _yard16."""
    n, hw, R, psi = 2, 150, 4, 7
    data, x, w, b = _ln_inputs(n, hw, R, D, D, D + dt)
    Td, P = 1 + R + hw, psi + hw
    full, body, gd = _canvas((n, P, D), dev, bits16=True)
    dx, dw, db = x.to(dev), w.to(dev), b.to(dev)
    assert _lib().wm_op_layernorm_rows(_p(dx), _p(body), _p(dw), _p(db), D, D, D, 1e-6, n, hw, Td, 1 + R, P, psi, 0, dt,
                                       _stream()) == 0
    torch.cuda.synchronize()
    _guards_intact(full, gd)
    _written_exactly(body, (torch.arange(P) >= psi).view(1, P, 1))
    _yard16(f"layernorm remapped 16-bit D{D} dt{dt}", body.cpu()[:, psi:], F.layer_norm(data, (D,), w, b, 1e-6),
            F.layer_norm(data.double(), (D,), w.double(), b.double(), 1e-6), dt)


# ------------------------------------------------------------------------------------------------------------------ GEMM epilogues
def _gemm_operands(M, N, K, dt, dev, seed):
    g = torch.Generator().manual_seed(seed)
    A = (torch.randn(M, K, generator=g)).to(_tdt(dt)).to(dev)
    W = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(_tdt(dt)).to(dev)
    return A, W, g


def _f32_epilogue(L, dt, A, W, bias, M, N, K):
    """The WM_EPI_F32 result (acc + bias) under the tuning the caller has set, checked against fp64 at the project's bound for it."""
    out = torch.empty(M, N, device=A.device)
    assert L.wm_op_gemm(dt, 0, _p(A), _p(W), _p(out), _p(bias), None, M, N, K, _stream()) == 0
    torch.cuda.synchronize()
    e = _rel(out, A.double() @ W.double().t() + bias.double())
    print(f"WM_EPI_F32 {M}x{N}x{K} dt{dt}: rel L2 vs fp64 {e:.2e}")
    assert e < 2e-5
    return out


ROWMAP_CASES = [
    # groups, rows_per_group, N, K, out_group, out_off, ldc - N, add, accumulate, out16, relu, tile configurations
    (8, 1369, 1024, 640, 1374, 5, 0, 1, 0, 0, 0, (4,)),        # patch embed + pos table into the DINO token buffer
    (2, 1369, 1024, 4096, 1376, 7, 0, 0, 1, 0, 0, (4, 5)),     # depth-prior MLP accumulated into the view tokens
    (3, 25, 384, 256, 32, 5, 8, 1, 1, 0, 0, (0, 1, 4, 5)),     # table AND accumulate; 25-row groups: every tile straddles groups
    (2, 137, 256, 512, 140, 2, 8, 1, 0, 1, 1, (0, 4, 5)),      # 16-bit output + ReLU (DPT projection form), about half the values negative
    (1, 150, 128, 192, 150, 0, 0, 0, 1, 0, 1, (0, 4)),         # ReLU + accumulate, no table (the DPT heads' image merger)
]


@pytest.mark.parametrize("dt", [BF16, F16])
@pytest.mark.parametrize("case", ROWMAP_CASES, ids=[f"g{c[0]}x{c[1]}_N{c[2]}_K{c[3]}" for c in ROWMAP_CASES])
def test_gemm_rowmap_add_epilogue(dev, case, dt):
    """WM_EPI_ROWMAP_ADD against WM_EPI_F32, bit for bit.  Both epilogues of gemm_nt_kernel are reached with the same forced tile
    configuration ("gemm_cfg"; "gemm_pp" = 0 keeps WM_EPI_F32 off the ping-pong kernels, which ROWMAP_ADD never takes), so acc + bias
    has the same bits, and the rest is relu?(.) + add[q] (+ old) in that order, single fp32 adds, then the 16-bit rounding when out16.
    rows_per_group 1369, 25, 137 are no multiple of 16 or 32: a tile straddles two groups.  The add table is the head of an
    allocation of M rows, so that an epilogue indexing it by the GEMM row instead of q reads a wrong value, not past the table."""
    G, rpg, N, K, out_group, out_off, ldpad, has_add, accumulate, out16, relu, cfgs = case
    M, ldc = G * rpg, N + ldpad
    A, W, g = _gemm_operands(M, N, K, dt, dev, M + N + K)
    bias = torch.randn(N, generator=g).to(dev)
    add_buf = torch.randn(M, N, generator=g).to(dev)
    add = add_buf[:rpg]
    rows_out = (G - 1) * out_group + out_off + rpg + 3
    old = torch.randn(rows_out, N, generator=g).to(dev)
    q = torch.arange(M, device=dev) % rpg
    orow = (torch.arange(M, device=dev) // rpg) * out_group + out_off + q
    mask = torch.zeros(rows_out, ldc, dtype=torch.bool, device=dev)
    mask[orow, :N] = True
    L = _lib()
    for cfg in cfgs:
        with _tuning(gemm_cfg=cfg, gemm_pp=0):
            f32 = _f32_epilogue(L, dt, A, W, bias, M, N, K)
            full, body, gd = _canvas((rows_out, ldc), dev, bits16=bool(out16))
            if accumulate:
                body[orow, :N] = old[orow].view(torch.int32)
            assert L.wm_op_gemm_rowmap(dt, _p(A), _p(W), _p(body), _p(bias), _p(add) if has_add else None, M, N, K, ldc, rpg, out_group, out_off,
                                       accumulate, out16, relu, _stream()) == 0
            torch.cuda.synchronize()
        _guards_intact(full, gd)
        _written_exactly(body, mask)
        exp = torch.relu(f32) if relu else f32
        if has_add:
            exp = exp + add[q]
        if accumulate:
            exp = exp + old[orow]
        exp = exp.to(_tdt(dt)).view(torch.int16) if out16 else exp.view(torch.int32)
        assert torch.equal(body[orow, :N], exp), f"cfg {cfg}: {int((body[orow, :N] != exp).sum())} elements differ"


@pytest.mark.parametrize("dt", [BF16, F16])
@pytest.mark.parametrize("n,gh,gw,k,cout,K", [(2, 37, 37, 4, 256, 1024), (1, 5, 4, 2, 512, 1024), (3, 1, 7, 4, 64, 256), (2, 10, 7, 2, 128, 512)])
def test_gemm_convt_epilogue(dev, n, gh, gw, k, cout, K, dt):
    """WM_EPI_CONVT against WM_EPI_F32 (same forced tile configuration, "gemm_pp" = 0), bit for bit: the [M][k*k*cout] matrix with the
    bias repeated per (ii, jj) is the [n][gh][gw][k][k][cout] tensor, the epilogue stores it as [n][gh*k][gw*k][cout].  The first
    shape is also held to fp64 F.conv_transpose2d at 2e-5 relative L2."""
    M, N = n * gh * gw, k * k * cout
    A, W, g = _gemm_operands(M, N, K, dt, dev, M + N + K)
    bias = torch.randn(cout, generator=g).to(dev)
    L = _lib()
    for cfg in ((0, 4, 5) if M * N < 1 << 22 else (4,)):
        with _tuning(gemm_cfg=cfg, gemm_pp=0):
            f32 = _f32_epilogue(L, dt, A, W, bias.repeat(k * k), M, N, K)
            full, body, gd = _canvas((n, gh * k, gw * k, cout), dev)
            assert L.wm_op_gemm_convt(dt, _p(A), _p(W), _p(body), _p(bias), M, N, K, k, cout, gh, gw, _stream()) == 0
            torch.cuda.synchronize()
        _guards_intact(full, gd)
        assert not bool(_sent(body).any())
        exp = f32.view(n, gh, gw, k, k, cout).permute(0, 1, 3, 2, 4, 5).reshape(n, gh * k, gw * k, cout)
        assert torch.equal(body.view(torch.float32), exp), f"cfg {cfg}"
    if (n, gh, k) == (2, 37, 4):
        wt = W.double().view(k, k, cout, K).permute(3, 2, 0, 1)   # torch layout [Cin][Cout][k][k]
        ref = F.conv_transpose2d(A.double().view(n, gh, gw, K).permute(0, 3, 1, 2), wt, bias.double(), stride=k).permute(0, 2, 3, 1)
        e = _rel(body.view(torch.float32), ref)
        print(f"WM_EPI_CONVT vs fp64 conv_transpose2d dt{dt}: rel L2 {e:.2e}")
        assert e < 2e-5


# ------------------------------------------------------------------------------------------------------------------ bilinear with tables, copy2d
BILINEAR_CASES = [
    # N, Hi, Wi, Ho, Wo, C                 kernel (bilinear_tiled_ok: C % 64 == 0, Ho, Wo >= 16, 15 * scale + 3 <= 12)
    (2, 19, 19, 37, 37, 64),             # tiled, x2 - 1
    (1, 37, 28, 70, 56, 128),            # tiled, non-integer factor, two 64-channel chunks
    (2, 9, 11, 33, 40, 128),             # tiled, ragged last tiles
    (1, 1, 9, 20, 30, 64),               # tiled, Hi == 1
    (2, 20, 16, 20, 16, 64),             # plain: Ho == Hi (identity, scale 1)
    (1, 1, 9, 1, 30, 64),                # plain: Hi == Ho == 1
    (3, 10, 10, 23, 17, 72),             # plain: C % 64 != 0, non-integer factor
    (1, 40, 40, 25, 25, 64),             # plain: downsampling
]


@pytest.mark.parametrize("out", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("N,Hi,Wi,Ho,Wo,Cc", BILINEAR_CASES)
def test_bilinear_with_position_tables(dev, N, Hi, Wi, Ho, Wo, Cc, out):
    """bilinear_tiled_kernel / bilinear_kernel (BILINEAR_CASES says which) with the separable tables addx [Wo][C/2], addy [Ho][C/2],
    fp32 output (wm_launch_bilinear) and 16-bit output (wm_launch_bilinear16): F.interpolate(align_corners=True) + the broadcast table.
    Measured on MI355X: fp32 e_kernel between 4.0e-8 and 5.4e-7, never above 1.3 x e_ref (largest pair 5.4e-7 / 1.7e-6 at 37 x 28 -> 70 x 56,
    where the fp32 source coordinate dominates both); 16-bit: kernel mismatches <= torch's on every case but one (16 / 14 of 175 232, f16,
    19 -> 37), largest 1157 / 2141 of 501 760 (f16, 37 x 28 -> 70 x 56)."""
    g = torch.Generator().manual_seed(Hi * 1000 + Wo + Cc)
    x = torch.randn(N, Hi, Wi, Cc, generator=g)
    addx, addy = torch.randn(Wo, Cc // 2, generator=g), torch.randn(Ho, Cc // 2, generator=g)
    tab = torch.cat([addx.view(1, 1, Wo, -1).expand(N, Ho, Wo, -1), addy.view(1, Ho, 1, -1).expand(N, Ho, Wo, -1)], -1)

    def ref(t, tb):
        return F.interpolate(t.permute(0, 3, 1, 2), size=(Ho, Wo), mode="bilinear", align_corners=True).permute(0, 2, 3, 1) + tb

    full, body, gd = _canvas((N, Ho, Wo, Cc), dev, bits16=out != "f32")
    dx, dax, day = x.to(dev), addx.to(dev), addy.to(dev)
    L = _lib()
    if out == "f32":
        st = L.wm_op_bilinear_add(_p(dx), _p(body), N, Hi, Wi, Ho, Wo, Cc, _p(dax), _p(day), _stream())
    else:
        st = L.wm_op_bilinear16(BF16 if out == "bf16" else F16, _p(dx), _p(body), N, Hi, Wi, Ho, Wo, Cc, _p(dax), _p(day),
                                _stream())
    assert st == 0
    torch.cuda.synchronize()
    _guards_intact(full, gd)
    assert not bool(_sent(body).any())
    name = f"bilinear+tables {(N, Hi, Wi, Ho, Wo, Cc)} {out}"
    if out == "f32":
        _yard32(name, body.view(torch.float32), ref(x, tab), ref(x.double(), tab.double()))
    else:
        _yard16(name, body, ref(x, tab), ref(x.double(), tab.double()), BF16 if out == "bf16" else F16)


@pytest.mark.parametrize("rows,cols,ld_src,ld_dst", [(37, 64, 96, 80), (1, 4, 8, 12), (3000, 1024, 2048, 1028)])
def test_copy2d(dev, rows, cols, ld_src, ld_dst):
    """copy2d_kernel with ld_src != ld_dst != cols: bit equality, the gap columns [cols, ld_dst) keep the sentinel."""
    src = torch.randn(rows, ld_src)
    full, body, gd = _canvas((rows, ld_dst), dev)
    dsrc = src.to(dev)
    assert _lib().wm_op_copy2d(_p(dsrc), _p(body), rows, cols, ld_src, ld_dst, _stream()) == 0
    torch.cuda.synchronize()
    _guards_intact(full, gd)
    _written_exactly(body, (torch.arange(ld_dst) < cols).view(1, ld_dst))
    assert torch.equal(body.cpu()[:, :cols], src[:, :cols].contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------ camera head
def _small_attn_ref(qkv, heads, hd):
    S, D = qkv.shape[0], heads * hd
    q, k, v = (qkv[:, i * D:(i + 1) * D].view(S, heads, hd).permute(1, 0, 2) for i in range(3))
    p = torch.softmax(q @ k.transpose(1, 2) / math.sqrt(hd), -1)
    return (p @ v).permute(1, 0, 2).reshape(S, D)


@pytest.mark.parametrize("heads,hd", [(16, 128), (4, 32), (3, 192)])
@pytest.mark.parametrize("S", [1, 2, 8, 63, 64, 65, 200])
def test_small_attention(dev, S, heads, hd):
    """small_attention_kernel (one wave per (query, head)): S around the wave width, hd below, at and above 64 lanes.
    Measured on MI355X: e_kernel 0 (S = 1) to 5.6e-7 (S = 200, 16 x 128) against e_ref 0 to 1.2e-6; e_kernel <= 1.2 x e_ref everywhere."""
    D = heads * hd
    qkv = torch.randn(S, 3 * D, generator=torch.Generator().manual_seed(S * 7 + hd))
    full, body, gd = _canvas((S, D), dev)
    dqkv = qkv.to(dev)
    assert _lib().wm_op_small_attention(_p(dqkv), _p(body), S, heads, hd, _stream()) == 0
    torch.cuda.synchronize()
    _guards_intact(full, gd)
    assert not bool(_sent(body).any())
    _yard32(f"small_attention S{S} heads{heads} hd{hd}", body.view(torch.float32), _small_attn_ref(qkv, heads, hd), _small_attn_ref(qkv.double(), heads, hd))


def test_small_attention_large_scores(dev):
    """q scaled so that the scores reach several hundred: exp(score) overflows fp32, exp(score - max) does not.
    Measured on MI355X (max |score| 693): e_kernel 1.4e-5, e_ref 3.4e-5."""
    S, heads, hd = 64, 16, 128
    D = heads * hd
    qkv = torch.randn(S, 3 * D, generator=torch.Generator().manual_seed(5))
    qkv[:, :D] *= 150.0
    ref64 = _small_attn_ref(qkv.double(), heads, hd)
    smax = float((qkv[:, :D].double().view(S, heads, hd).permute(1, 0, 2) @ qkv[:, D:2 * D].double().view(S, heads, hd).permute(1, 2, 0)).abs().max()) / math.sqrt(hd)
    assert smax > 300, smax
    full, body, gd = _canvas((S, D), dev)
    dqkv = qkv.to(dev)
    assert _lib().wm_op_small_attention(_p(dqkv), _p(body), S, heads, hd, _stream()) == 0
    torch.cuda.synchronize()
    _guards_intact(full, gd)
    got = body.view(torch.float32)
    assert bool(torch.isfinite(got).all()), "the max subtraction must keep the softmax finite"
    _yard32(f"small_attention large scores (max |score| {smax:.0f})", got, _small_attn_ref(qkv, heads, hd), ref64)


def test_small_attention_refuses_more_than_8192_tokens(dev):
    """S * 4 bytes of dynamic LDS: S > 8192 is refused with WM_ERR_INVALID and nothing is launched."""
    full, body, gd = _canvas((16, 64), dev)
    dummy = torch.zeros(64, device=dev)
    assert _lib().wm_op_small_attention(_p(dummy), _p(body), 8193, 1, 64, _stream()) == 1
    torch.cuda.synchronize()
    assert bool(_sent(full).all())


@pytest.mark.parametrize("S", [1, 8, 33])
@pytest.mark.parametrize("D", [2048, 1024, 256, 384, 100])
def test_adaln(dev, D, S):
    """adaln_kernel: D = 2048, 1024, 256 take the register path (D % 256 == 0), D = 384, 100 the generic one.  Rows with a large common
    offset: the variance must come from a second pass over (x - mean).  Measured on MI355X: e_kernel 5.7e-8 .. 1.3e-7, e_ref 5.7e-8 .. 1.0e-7,
    largest ratio 1.7 (D = 384, S = 8: 1.02e-7 / 5.97e-8); all below the 4 x 2^-23 floor."""
    g = torch.Generator().manual_seed(D + S)
    tok = torch.randn(S, D, generator=g) * 2 + 30
    mod = torch.randn(S, 3 * D, generator=g) * 0.5

    def ref(t, m):
        sh, sc, gt = m[:, :D], m[:, D:2 * D], m[:, 2 * D:]
        return gt * (F.layer_norm(t, (D,), None, None, 1e-6) * (1 + sc) + sh) + t

    full, body, gd = _canvas((S, D), dev)
    dtok, dmod = tok.to(dev), mod.to(dev)
    assert _lib().wm_op_adaln(_p(dtok), _p(dmod), _p(body), S, D, 1e-6, _stream()) == 0
    torch.cuda.synchronize()
    _guards_intact(full, gd)
    assert not bool(_sent(body).any())
    _yard32(f"adaln D{D} S{S}", body.view(torch.float32), ref(tok, mod), ref(tok.double(), mod.double()))


@pytest.mark.parametrize("first", [1, 0])
@pytest.mark.parametrize("S", [1, 5, 300])
def test_cam_update(dev, S, first):
    """cam_update_kernel: pred[:, 0:9] = delta (first) or pred + delta (one fp32 add), out = the same with ReLU on columns 7 and 8 only
    (half the fov deltas are negative); pred[:, 9:12] and everything outside [S][9] / [S][12] untouched.  Bit equality."""
    g = torch.Generator().manual_seed(S + first)
    pred0, delta = torch.randn(S, 12, generator=g), torch.randn(S, 12, generator=g)
    pfull, pbody, pg = _canvas((S, 12), dev)
    pbody.copy_(pred0.view(torch.int32))
    ofull, obody, og = _canvas((S, 9), dev)
    ddelta = delta.to(dev)
    assert _lib().wm_op_cam_update(_p(pbody), _p(ddelta), _p(obody), S, first, _stream()) == 0
    torch.cuda.synchronize()
    _guards_intact(pfull, pg)
    _guards_intact(ofull, og)
    v = delta[:, :9] if first else pred0[:, :9] + delta[:, :9]
    assert bool((v[:, 7:] < 0).any()) or S == 1
    exp_pred = torch.cat([v, pred0[:, 9:]], 1)
    exp_out = torch.cat([v[:, :7], torch.relu(v[:, 7:])], 1)
    assert torch.equal(pbody.cpu(), exp_pred.view(torch.int32))
    assert torch.equal(obody.cpu(), exp_out.view(torch.int32))


def _cam_ref(p, H, W):
    """camera_utils' construction: R from the xyzw quaternion (two_s = 2 / |q|^2), c2w = inv([R | t; 0 0 0 1]), K from the two fovs."""
    i, j, k, r = p[:, 3], p[:, 4], p[:, 5], p[:, 6]
    s = 2.0 / (p[:, 3:7] * p[:, 3:7]).sum(-1)
    R = torch.stack([1 - s * (j * j + k * k), s * (i * j - k * r), s * (i * k + j * r), s * (i * j + k * r), 1 - s * (i * i + k * k), s * (j * k - i * r),
                     s * (i * k - j * r), s * (j * k + i * r), 1 - s * (i * i + j * j)], -1).view(-1, 3, 3)
    ext = torch.cat([torch.cat([R, p[:, 0:3, None]], -1), torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=p.dtype).expand(p.shape[0], 1, 4)], -2)
    Km = torch.zeros(p.shape[0], 3, 3, dtype=p.dtype)
    Km[:, 1, 1] = H * 0.5 / torch.tan(p[:, 7] * 0.5)
    Km[:, 0, 0] = W * 0.5 / torch.tan(p[:, 8] * 0.5)
    Km[:, 0, 2], Km[:, 1, 2], Km[:, 2, 2] = W * 0.5, H * 0.5, 1.0
    return torch.linalg.inv(ext), Km


@pytest.mark.parametrize("S,H,W", [(1, 518, 518), (7, 518, 392), (130, 70, 56)])
def test_cam_matrices(dev, S, H, W):
    """cam_matrices_kernel with un-normalised quaternions (norm 0.3 .. 3) and fov in (0.2, 2.5) against fp64 torch.linalg.inv of the 4x4;
    R R^T = I of the returned rotation is held to the same yardstick (the error of torch's fp32 inverse).  Measured on MI355X (e_kernel /
    e_ref) for S = 1, 7, 130: poses 6.5e-8 / 6.1e-8, 2.1e-7 / 9.3e-8, 2.5e-7 / 2.4e-7; intrinsics 9.9e-9 / 7.0e-8, 4.9e-8 / 5.2e-8, 6.4e-8 / 6.4e-8;
    max |R R^T - I| 8.5e-8 / 9.3e-8, 3.4e-7 / 2.6e-7, 5.1e-7 / 6.0e-7."""
    g = torch.Generator().manual_seed(S)
    p = torch.randn(S, 9, generator=g)
    qn = p[:, 3:7] / p[:, 3:7].norm(dim=-1, keepdim=True)
    p[:, 3:7] = qn * (0.3 + 2.7 * torch.rand(S, 1, generator=g))
    p[:, 7:9] = 0.2 + 2.3 * torch.rand(S, 2, generator=g)
    pfull, pose, pg = _canvas((S, 16), dev)
    kfull, intr, kg = _canvas((S, 9), dev)
    dp = p.to(dev)
    assert _lib().wm_op_cam_matrices(_p(dp), _p(pose), _p(intr), S, H, W, _stream()) == 0
    torch.cuda.synchronize()
    _guards_intact(pfull, pg)
    _guards_intact(kfull, kg)
    assert not bool(_sent(pose).any()) and not bool(_sent(intr).any())
    c32, k32 = _cam_ref(p, H, W)
    c64, k64 = _cam_ref(p.double(), H, W)
    gp, gk = pose.view(torch.float32).cpu().view(S, 4, 4), intr.view(torch.float32).cpu().view(S, 3, 3)
    _yard32(f"cam_matrices poses S{S}", gp, c32, c64)
    _yard32(f"cam_matrices intrinsics S{S}", gk, k32, k64)
    eye = torch.eye(3, dtype=torch.float64)
    ek = float((gp[:, :3, :3].double() @ gp[:, :3, :3].double().transpose(1, 2) - eye).abs().max())
    er = float((c32[:, :3, :3].double() @ c32[:, :3, :3].double().transpose(1, 2) - eye).abs().max())
    print(f"cam_matrices R R^T - I S{S}: e_kernel {ek:.3e} e_ref {er:.3e}")
    assert ek <= 4 * max(er, 2.0 ** -23)


LINEAR_SHAPES = [(3, 256, 9, 12), (12, 512, 256, 256), (64, 6144, 2048, 2048), (5, 9, 1024, 1024), (8, 6144, 2048, 2048), (13, 2048, 2048, 2080),
                 (16, 4096, 1024, 1024), (1, 2048, 8192, 8192), (32, 8192, 2048, 2048), (17, 2048, 2048, 2048), (40, 2048, 8192, 8192),
                 (33, 4096, 1024, 1040), (65, 2048, 2048, 2048)]


def _linear_takes_mfma(M, N, K):
    return M <= 64 and N % 16 == 0 and K % 1024 == 0


@pytest.mark.parametrize("M,N,K,ldx,lin_mfma", [s + (-1,) for s in LINEAR_SHAPES] + [s + (0,) for s in LINEAR_SHAPES if _linear_takes_mfma(*s[:3])])
def test_linear_f32_gamma_accumulate_ldy(dev, M, N, K, ldx, lin_mfma):
    """wm_launch_linear_f32 with gamma, with accumulation onto random content, and with ldy = N + 8 (the gap columns keep the sentinel), on
    the shapes of test_gpu_ops.py::test_linear_f32.  Kernels: (3, 256, 9) -> linear_f32_kernel (K % 4 != 0); (12, 512, 256), (5, 9, 1024),
    (65, 2048, 2048) -> linear_f32_stream_kernel; the other shapes (M <= 64, N % 16 == 0, K % 1024 == 0) -> linear_f32_mfma_kernel, and
    with the tuning "lin_mfma" = 0 linear_f32_stream_kernel at those shapes too.  Measured on MI355X over the three variants: generic kernel
    e_kernel 1.1e-7 .. 1.6e-7 (e_ref 1.1e-7 .. 1.7e-7); streaming kernel 5.0e-8 .. 2.0e-7 (e_ref 1.4e-7 .. 7.1e-7), never above e_ref; MFMA
    kernel 1.6e-7 .. 4.0e-7 (e_ref 1.4e-7 .. 6.6e-7), largest ratio 2.5 at (32, 8192, 2048) (4.0e-7 / 1.6e-7): each wave's share of the K sum
    is one sequential chain of MFMA accumulations, torch's sum is blocked."""
    g = torch.Generator().manual_seed(M + N)
    X = torch.full((M, ldx), 1.0e6)
    X[:, :K] = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g) / math.sqrt(K)
    b, gamma = torch.randn(N, generator=g), torch.randn(N, generator=g)
    old = torch.randn(M, N, generator=g)
    Xd, Wd, bd, gd_ = X.to(dev), W.to(dev), b.to(dev), gamma.to(dev)
    act = {0: lambda t: t, 1: F.silu, 2: F.gelu}
    L = _lib()
    #          pre, post, gamma, accumulate, ldy
    variants = [(1, 2, True, False, N), (0, 1, False, True, N), (1, 0, True, True, N + 8)]
    for pre, post, has_gamma, accumulate, ldy in variants:
        full, body, gb = _canvas((M, ldy), dev)
        if accumulate:
            body[:, :N] = old.to(dev).view(torch.int32)
        with _tuning(lin_mfma=lin_mfma):
            assert L.wm_op_linear_f32_ex(_p(Xd), _p(Wd), _p(bd), _p(body), M, N, K, ldx, ldy, pre, post, _p(gd_) if has_gamma else None,
                                         1 if accumulate else 0, _stream()) == 0
            torch.cuda.synchronize()
        _guards_intact(full, gb)
        _written_exactly(body, (torch.arange(ldy) < N).view(1, ldy))

        def ref(x, w, bb, gm, od):
            y = act[post](act[pre](x) @ w.t() + bb)
            if has_gamma:
                y = y * gm
            return od + y if accumulate else y

        _yard32(f"linear_f32 {(M, N, K, ldx)} lin_mfma{lin_mfma} pre{pre} post{post} gamma{int(has_gamma)} acc{int(accumulate)} ldy{ldy}",
                body.cpu().view(torch.float32)[:, :N],
                ref(X[:, :K], W, b, gamma, old), ref(X[:, :K].double(), W.double(), b.double(), gamma.double(), old.double()))
