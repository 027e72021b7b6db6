"""Forward and forward + backward time of the appearance module at the trainer's configuration (feature_dim 32, embed_dim 16, width 64,
depth 2, sh_degree 3): C cameras x N Gaussians.  Forms:

    fused   hunyuanworld_mirror_amd.AppearanceOptModule (csrc/appearance.hip)
    torch   the same module composed of torch ops in fp32 on the same GPU (tests/appearance_helper.py: embedding lookup, F.normalize, the
            SH basis, torch.cat, three matmuls) -- what examples/utils.py does on this hardware

Timed with device events around each call, the two forms interleaved round after round on the same inputs; the first `--warmup` rounds
warm every form up and are dropped.  Per form and size the median and the spread (min .. max), and whether the fused form was the faster
one in EVERY round, as one JSON line each.  The backward is driven by a fixed upstream gradient; features, dirs and every parameter
require grad.  After the timing the two forms' gradients are compared with each other and, at sizes up to --fp64-up-to, each with the
same composition run in fp64 on the device.

    python tools/bench_appearance.py [--cameras 8] [--sizes 262144,1048576] [--rounds 9] [--warmup 2] [--tag NAME]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hunyuanworld_mirror_amd as wm  # noqa: E402
import appearance_helper as AH  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cameras", type=int, default=8)
    ap.add_argument("--sizes", default="262144,1048576")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--degree", type=int, default=3)
    ap.add_argument("--fp64-up-to", type=int, default=262144, help="sizes up to this many Gaussians are also run in fp64 (about 10 GB at 2^18 x 8)")
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    Cn, n_img = a.cameras, 64
    g = torch.Generator().manual_seed(5)
    state = AH.random_state(n_img, 3, g)
    module = wm.AppearanceOptModule(n_img, 32, 16, 3)
    module.load_state_dict(state)
    module = module.to(dev)
    params = {k: v.to(dev).requires_grad_(True) for k, v in state.items()}
    ids = torch.randint(0, n_img, (Cn,), generator=g).to(dev)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for N in (int(s) for s in a.sizes.split(",")):
        features = torch.randn(N, 32, generator=g).to(dev).requires_grad_(True)
        dirs = (torch.randn(Cn, N, 3, generator=g) * 2.0).to(dev).requires_grad_(True)
        v_out = torch.randn(Cn, N, 3, generator=g).to(dev)
        forms = {"fused": lambda: module(features, ids, dirs, a.degree), "torch": lambda: AH.forward(params, features, ids, dirs, a.degree)}

        def forward_only(f):
            with torch.no_grad():
                forms[f]()

        def both(f):
            for t in (features, dirs, *params.values(), *module.parameters()):
                t.grad = None
            forms[f]().backward(v_out)

        t_f, t_fb = {f: [] for f in forms}, {f: [] for f in forms}
        for r in range(a.warmup + a.rounds):
            for f in forms:
                tf, tfb = timed(lambda: forward_only(f)), timed(lambda: both(f))
                if r >= a.warmup:
                    t_f[f].append(tf); t_fb[f].append(tfb)
        for f in forms:
            print(json.dumps(dict(tag=a.tag, form=f, cameras=Cn, gaussians=N, degree=a.degree, rounds=a.rounds,
                                  forward_ms_median=round(statistics.median(t_f[f]), 3), forward_ms_min=round(min(t_f[f]), 3),
                                  forward_ms_max=round(max(t_f[f]), 3), fwd_bwd_ms_median=round(statistics.median(t_fb[f]), 3),
                                  fwd_bwd_ms_min=round(min(t_fb[f]), 3), fwd_bwd_ms_max=round(max(t_fb[f]), 3))), flush=True)
        both("fused")
        got = {"fused": dict(v_features=features.grad.clone(), v_dirs=dirs.grad.clone(), **{k: p.grad.clone() for k, p in module.named_parameters()})}
        both("torch")
        got["torch"] = dict(v_features=features.grad.clone(), v_dirs=dirs.grad.clone(), **{k: p.grad.clone() for k, p in params.items()})
        rel = lambda x, y: float((x.double() - y.double()).abs().max() / y.double().abs().max())
        line = dict(tag=a.tag, gaussians=N,
                    fused_faster_in_every_round_forward=all(x < y for x, y in zip(t_f["fused"], t_f["torch"])),
                    fused_faster_in_every_round_fwd_bwd=all(x < y for x, y in zip(t_fb["fused"], t_fb["torch"])),
                    max_rel_fused_vs_torch={k: rel(got["fused"][k], got["torch"][k]) for k in got["torch"]})
        if N <= a.fp64_up_to:
            # the same inputs through the composition in fp64 on the device: each form's own error at the timed size
            ref = AH.gradients(state, features, ids, dirs, v_out, a.degree, torch.float64, device=dev)
            for f in forms:
                line[f"max_rel_{f}_vs_fp64"] = {k: rel(got[f][k], ref[k]) for k in got[f]}
            del ref
        print(json.dumps(line), flush=True)
        del got
        del features, dirs, v_out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
