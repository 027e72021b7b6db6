"""Times of the MCMC strategy's kernels at N = 1 000 000 (profiles/r08_mcmc.md):
  noise    wm_mcmc_inject_noise against the same formula as gsplat composes it from torch ops (ops.py:343-369, with the torch form of the
           covariance) on the same device; both draw their noise outside the timed window.  Device events around batches of calls.
  refine   one relocation + growth (relocate with 5 % dead, then sample_add of min(cap_max, int(1.05 N)) - N) on means, scales,
           quats, opacities, sh0, shN [N,15,3] with two Adam moments each: wall time around a stream synchronisation.
Prints one JSON line per measurement: median, min, max in ms.

    python tools/bench_mcmc.py [--n 1000000] [--iters 20]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hunyuanworld_mirror_amd import strategy_mcmc as S  # noqa: E402


def splats(N, dev, dead_fraction):
    g = torch.Generator().manual_seed(7)
    u = lambda *s: torch.rand(*s, generator=g)
    opac = 10 ** (-2.2 + 2.1 * u(N))
    opac[u(N) < dead_fraction] = 1e-3
    p = {"means": torch.randn(N, 3, generator=g), "scales": torch.log(10 ** (-2.2 + 1.4 * u(N, 3))), "quats": torch.randn(N, 4, generator=g),
         "opacities": torch.logit(opac), "sh0": u(N, 1, 3), "shN": torch.randn(N, 15, 3, generator=g) * 0.1}
    return {k: t.to(dev) for k, t in p.items()}


def torch_noise(p, noise, scaler):
    """inject_noise_to_position as the reference composes it"""
    opacities = torch.sigmoid(p["opacities"].flatten())
    scales = torch.exp(p["scales"])
    q = torch.nn.functional.normalize(p["quats"], p=2, dim=-1)
    w, x, y, z = torch.unbind(q, dim=-1)
    R = torch.stack([1 - 2 * (y ** 2 + z ** 2), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x ** 2 + z ** 2),
                     2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x ** 2 + y ** 2)], dim=-1).reshape(-1, 3, 3)
    M = R * scales[..., None, :]
    covars = torch.einsum("...ij,...kj -> ...ik", M, M)
    nz = noise * (1 / (1 + torch.exp(-100 * ((1 - opacities) - 0.995)))).unsqueeze(-1) * scaler
    p["means"].add_(torch.einsum("bij,bj->bi", covars, nz))


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4)}


def event_time(fn, iters, batch):
    for _ in range(3):
        fn()
    out = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(batch):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / batch)
    return stats(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    N = a.n
    p = splats(N, dev, 0.0)
    noise = torch.randn(N, 3, device=dev)
    args = (p["means"], p["quats"], p["scales"], p["opacities"], noise, 80.0)
    # alternate the two, so that both see the same machine
    for rnd in range(2):
        r = event_time(lambda: S.mcmc_inject_noise(*args), a.iters, 50)
        r.update(what="wm_mcmc_inject_noise", N=N, round=rnd, GBps=round(68.0 * N / (r["median_ms"] * 1e-3) / 1e9, 1))
        print(json.dumps(r), flush=True)
        r = event_time(lambda: torch_noise(p, noise, 80.0), a.iters, 10)
        r.update(what="torch ops", N=N, round=rnd)
        print(json.dumps(r), flush=True)
    del p, noise, args
    times, info = [], None
    for i in range(3 + 5):
        p = splats(N, dev, 0.05)
        params = {k: torch.nn.Parameter(t) for k, t in p.items()}
        opts = {k: torch.optim.Adam([params[k]], lr=1e-3) for k in params}
        for k in params:
            opts[k].state[params[k]] = {"step": torch.tensor(1.0), "exp_avg": torch.ones_like(params[k]), "exp_avg_sq": torch.ones_like(params[k])}
        strat = S.MCMCStrategy(cap_max=2 * N)
        gen = torch.Generator(device=dev).manual_seed(i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n_rel = strat._relocate_gs(params, opts, gen)
        n_new = strat._add_new_gs(params, opts, gen)
        torch.cuda.synchronize()
        if i >= 3:
            times.append((time.perf_counter() - t0) * 1e3)
        info = dict(relocated=n_rel, added=n_new)
    r = stats(times)
    r.update(what="relocate + sample_add", N=N, **info)
    print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
