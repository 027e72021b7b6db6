"""Writes tests/golden/eval_*.npz: the REFERENCE's own color_correct (gsplat's examples/lib_bilagrid.py:56-126), run on the CPU in fp64 and
in fp32 on fp32-valued inputs, and the trainer's canvas and PSNR statements (simple_trainer_worldmirror.py:1040-1054).  Data only.

    python tools/gen_golden_eval.py <reference gsplat examples dir>

lib_bilagrid imports tensorly at module level (only its CP-decomposed 4-D grid uses it); where tensorly is absent a stub module with a
no-op set_backend stands in, as in tools/gen_golden_bilagrid.py.

Files
  eval_a.npz, eval_b.npz   scenes "a" (37 x 52) and "b" (61 x 83) of tests/eval_helper.py: the seed, img, ref, cc64 = the reference's fp64
                           result, e32 = max |its fp32 result - its fp64 result|, margin = the guard's smallest distance of a masked value
                           from a threshold, ratio_genuine = the smallest eigenvalue ratio lambda / lambda_max of any of the 15 Gram matrices.
  eval_ratios.npz          for image sizes 11 x 11 .. 518 x 518: ratio_genuine of a full-rank scene and ratio_spurious = the largest
                           dropped ratio of an exactly collinear system (a grey image: identical columns).  The cut-off lies between them.
  eval_frame.npz           a 23 x 31 batch of 2: colors (unclamped), pixels_u8, the canvas bytes by the trainer's fp32 statements and the
                           PSNR of the clamped render in fp64 (whole batch and per image).
The guard (no ref value and no img_mat value of any iteration within 256 e32 of eps or 1 - eps) is asserted here with the reference's
e32; a scene that violates it gets the next seed."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import eval_helper as EH  # noqa: E402


def load_reference(examples_dir):
    try:
        import tensorly  # noqa: F401
    except ImportError:
        stub = types.ModuleType("tensorly")
        stub.set_backend = lambda *a, **k: None
        sys.modules["tensorly"] = stub
    sys.path.insert(0, examples_dir)
    import lib_bilagrid
    return lib_bilagrid


def main():
    lib = load_reference(sys.argv[1])
    gold = os.path.join(ROOT, "tests", "golden")
    for name in ("a", "b"):
        B, H, W, seed0 = EH.SCENES[name]
        for seed in range(seed0, seed0 + 50):
            img, ref = EH.draw_scene(B, H, W, seed)
            cc64 = lib.color_correct(img.double(), ref.double())
            cc32 = lib.color_correct(img, ref)
            assert cc64.dtype == torch.float64 and cc32.dtype == torch.float32
            e32 = float((cc32.double() - cc64).abs().max())
            info = {}
            ours = EH.color_correct(img.double(), ref.double(), info=info)
            if info["margin"] >= EH.GUARD_FACTOR * e32:
                break
        else:
            raise SystemExit(f"scene {name}: no seed passes the guard")
        print(f"scene {name}: seed {seed}, e32 {e32:.3e}, margin {info['margin']:.3e}, smallest eigenvalue ratio {info['ratio_genuine']:.3e}, "
              f"restatement against the reference {float((ours - cc64).abs().max()):.3e}")
        np.savez(os.path.join(gold, f"eval_{name}.npz"), seed=np.int64(seed), img=img.numpy(), ref=ref.numpy(), cc64=cc64.numpy(),
                 e32=np.float64(e32), margin=np.float64(info["margin"]), ratio_genuine=np.float64(info["ratio_genuine"]))

    sizes = [(11, 11), (23, 31), (37, 52), (61, 83), (128, 128), (300, 300), (518, 518)]
    gen, spu = [], []
    for i, (H, W) in enumerate(sizes):
        img, ref = EH.draw_scene(1, H, W, 900 + i)
        info = {}
        EH.color_correct(img.double(), ref.double(), info=info)
        gen.append(info["ratio_genuine"])
        g = torch.Generator().manual_seed(950 + i)
        grey = (0.1 + 0.8 * torch.rand(1, H, W, 1, generator=g)).float().repeat(1, 1, 1, 3)
        target = torch.stack([0.9 * grey[..., 0] ** 2 + 0.05, 0.8 * grey[..., 1], 0.3 * grey[..., 2] ** 2 + 0.5 * grey[..., 2] + 0.1], dim=-1)
        info = {}
        EH.color_correct(grey.double(), target.double(), info=info)
        spu.append(info["ratio_spurious"])
        print(f"{H} x {W}: genuine {gen[-1]:.3e}, spurious (grey) {spu[-1]:.3e}")
    assert max(spu) < EH.CUTOFF < min(gen)
    np.savez(os.path.join(gold, "eval_ratios.npz"), sizes=np.array(sizes, np.int64), ratio_genuine=np.array(gen), ratio_spurious=np.array(spu),
             cutoff=np.float64(EH.CUTOFF))

    # the trainer's statements, :1021 and :1040-1046 in fp32 as written, the PSNR (torchmetrics' definition, data_range 1) in fp64
    colors, pixels = EH.frame_inputs(2, 23, 31, 77)
    pixels_u8 = torch.round(pixels * 255).to(torch.uint8)
    pixels = pixels_u8.to(torch.float32) / 255.0
    clamped = torch.clamp(colors, 0.0, 1.0)
    canvas = torch.cat([pixels, clamped], dim=2).numpy()
    canvas = (canvas * 255).astype(np.uint8)
    d2 = (clamped.double() - pixels.double()) ** 2
    psnr = float(10.0 * torch.log10(1.0 / d2.mean()))
    psnr_each = (10.0 * torch.log10(1.0 / d2.reshape(2, -1).mean(dim=1))).numpy()
    print(f"frame: psnr {psnr:.6f}, per image {psnr_each}, bytes that differ from the uint8 input: {int((canvas[:, :, :31] != pixels_u8.numpy()).sum())}")
    np.savez(os.path.join(gold, "eval_frame.npz"), colors=colors.numpy(), pixels_u8=pixels_u8.numpy(), canvas=canvas, psnr=np.float64(psnr),
             psnr_each=psnr_each)


if __name__ == "__main__":
    main()
