"""Time of the trainer's per-batch evaluation (Runner.eval :1040-1060) at the trainer's size, 518 x 518, for one image and for a batch of
8 evaluated per image.  Forms:

    fused        hunyuanworld_mirror_amd.eval_metrics (csrc/evalmetrics.hip + the SSIM kernel), without and with colour correction
    torch        the same steps as torch ops in fp32 on the same GPU: clamp, cat, * 255 -> uint8, the PSNR from (a - b)^2 .mean(), SSIM by the
                 same fused_ssim kernel (it is shared, not compared), and for colour correction tests/eval_helper.py's restatement of the
                 reference's composition: the [P,10] feature matrix, three masked copies, torch.linalg.lstsq, 5 iterations
    torch_normal the colour correction in normal-equation form (Gram matrix + torch.linalg.solve in fp64), timed in any case and the
                 baseline where the device's lstsq is unusable for these systems

Timed the way tools/bench_bilagrid.py does: the forms interleaved, round after round, a host clock around `--inner` calls that end in a
device synchronise; the first round warms every form up and is dropped; per form the median and the spread as one JSON line.  The
lstsq forms run last, and an exception from them ends the run there (the line says so).

    python tools/bench_eval_metrics.py [--rounds 7] [--inner 5] [--skip-lstsq] [--tag NAME]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hunyuanworld_mirror_amd as wm  # noqa: E402
import eval_helper as EH  # noqa: E402


def torch_frame(colors, pixels):
    """the loose ops: -> psnr [B], ssim [B], canvas, clamped"""
    c = torch.clamp(colors, 0.0, 1.0)
    canvas = (torch.cat([pixels, c], dim=2) * 255).to(torch.uint8)
    psnr = torch.stack([10.0 * torch.log10(1.0 / ((c[b] - pixels[b]) ** 2).mean()) for b in range(c.shape[0])])
    ssim = torch.stack([wm.fused_ssim(c[b:b + 1].permute(0, 3, 1, 2), pixels[b:b + 1].permute(0, 3, 1, 2), padding="valid", train=False)
                        for b in range(c.shape[0])])
    return psnr, ssim, canvas, c


def torch_eval(colors, pixels, cc_fn):
    psnr, ssim, canvas, c = torch_frame(colors, pixels)
    out = [psnr, ssim, canvas]
    if cc_fn is not None:
        for b in range(c.shape[0]):
            cc = cc_fn(c[b], pixels[b])[None]
            out.append(10.0 * torch.log10(1.0 / ((cc - pixels[b:b + 1]) ** 2).mean()))
            out.append(wm.fused_ssim(cc.permute(0, 3, 1, 2), pixels[b:b + 1].permute(0, 3, 1, 2), padding="valid", train=False))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--tag", default="")
    ap.add_argument("--skip-lstsq", action="store_true", help="leave the (slow) torch.linalg.lstsq forms out")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    H = W = 518

    def timed(fn):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(a.inner):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / a.inner

    def report(form, B, ts, **extra):
        print(json.dumps(dict(tag=a.tag, form=form, images=B, size=H, rounds=a.rounds, inner=a.inner, ms_median=round(statistics.median(ts), 4),
                              ms_min=round(min(ts), 4), ms_max=round(max(ts), 4), **extra)), flush=True)

    scenes = {}
    for B in (1, 8):
        img, ref = EH.draw_scene(B, H, W, 1000 + B)
        g = torch.Generator().manual_seed(B)
        render = img + 0.3 * (torch.rand(img.shape, generator=g) < 0.02) * torch.randn(img.shape, generator=g)     # a few values leave [0, 1]
        scenes[B] = (render.to(dev), ref.to(dev))

    forms = {
        "fused": lambda c, p: wm.eval_metrics(c, p, canvas=True, per_image=True),
        "fused_cc": lambda c, p: wm.eval_metrics(c, p, color_corrected=True, canvas=True, per_image=True),
        "fused_color_correct_only": lambda c, p: wm.color_correct(c, p, per_image=True),
        "torch": lambda c, p: torch_eval(c, p, None),
        "torch_normal_cc": lambda c, p: torch_eval(c, p, EH.color_correct_normal),
        "torch_normal_color_correct_only": lambda c, p: [EH.color_correct_normal(c[b], p[b]) for b in range(c.shape[0])],
    }
    with torch.no_grad():
        for B, (c, p) in scenes.items():
            ts = {f: [] for f in forms}
            for r in range(a.rounds + 1):
                for f, fn in forms.items():
                    t = timed(lambda: fn(c, p))
                    if r > 0:
                        ts[f].append(t)
            for f in forms:
                report(f, B, ts[f])
            cl = torch.clamp(c, 0, 1)
            d = (wm.color_correct(cl, p, per_image=True) - torch.stack([EH.color_correct_normal(cl[b], p[b]) for b in range(B)])).abs().max()
            print(json.dumps(dict(tag=a.tag, images=B, color_correct_max_abs_fused_vs_torch_normal=float(d))), flush=True)
        if a.skip_lstsq:
            return
        # the reference's composition on the device: lstsq on the masked [P,10] systems (ROCm: the full-rank gels driver only)
        late = {"torch_lstsq_cc": lambda c, p: torch_eval(c, p, EH.color_correct_lstsq),
                "torch_lstsq_color_correct_only": lambda c, p: [EH.color_correct_lstsq(c[b], p[b]) for b in range(c.shape[0])]}
        for B, (c, p) in scenes.items():
            for f, fn in late.items():
                try:
                    ts = [timed(lambda: fn(c, p)) for _ in range(a.rounds + 1)][1:]
                    cl = torch.clamp(c, 0, 1)
                    d = (wm.color_correct(cl, p, per_image=True) - torch.stack([EH.color_correct_lstsq(cl[b], p[b]) for b in range(B)])).abs().max()
                    report(f, B, ts, color_correct_max_abs_fused_vs_this=float(d))
                except Exception as e:      # noqa: BLE001  (the line records it; nothing more is started on the device)
                    print(json.dumps(dict(tag=a.tag, form=f, images=B, unusable=f"{type(e).__name__}: {str(e)[:300]}")), flush=True)
                    return


if __name__ == "__main__":
    main()
