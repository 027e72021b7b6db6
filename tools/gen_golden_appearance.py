"""Writes tests/golden/appearance_{a,b}.npz: the REFERENCE's own AppearanceOptModule (gsplat's examples/utils.py:51-114), run on the CPU in
fp64 on fp32-valued inputs.  Data only: the state dict, features, embed_ids, dirs, the upstream gradient v_out; the output and every
gradient (features, dirs, the seven parameter tensors); the ReLU margin.

    python tools/gen_golden_appearance.py <reference root>

examples/utils.py imports sklearn and matplotlib at module level (its colour-map and k-nn helpers use them); where they are absent, stub
modules stand in.  Its forward imports gsplat.cuda._torch_impl._eval_sh_bases_fast, which is plain torch.  The forward allocates its
basis buffer with torch.zeros(...) in the DEFAULT dtype, so under .double() alone the basis values would be rounded to fp32 on the way
in (a 5e-9 relative effect on the output): the module is therefore run with torch's default dtype set to float64, which makes every
intermediate fp64.

Scenes
  a   n = 5 images, C = 3 with embed_ids [4, 0, 4] (a repeated id; rows 1, 2, 3 unused), N = 300, module degree 3 called at degree 3.
  b   the same module (another draw of its parameters) called at degree 1 (bands 4..15 unused) with embed_ids None, C = 2, N = 257.
ReLU has a kink: a hidden pre-activation that fp32 rounding can push across zero changes a gradient by a finite amount.  Asserted here and
again by tests/test_appearance_cpu.py: no hidden pre-activation of any pair lies within margin = 16 x the largest fp32-against-fp64
difference of those pre-activations (measured here, stored in the file) of zero.  A scene that violates it gets the next seed."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import appearance_helper as AH  # noqa: E402


def load_reference(ref):
    for name, attrs in (("sklearn", ()), ("sklearn.neighbors", ("NearestNeighbors",)), ("matplotlib", ("colormaps",)), ("matplotlib.pyplot", ())):
        try:
            importlib.import_module(name)
        except ImportError:
            stub = types.ModuleType(name)
            for a in attrs:
                setattr(stub, a, None)
            sys.modules[name] = stub
    sys.path[:0] = [ref, os.path.join(ref, "submodules", "gsplat")]
    spec = importlib.util.spec_from_file_location("gsplat_examples_utils", os.path.join(ref, "submodules", "gsplat", "examples", "utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.AppearanceOptModule


SCENES = {"a": dict(n=5, C=3, N=300, module_degree=3, degree=3, ids=(4, 0, 4)),
          "b": dict(n=5, C=2, N=257, module_degree=3, degree=1, ids=None)}


def run(Module, sc, cfg):
    assert torch.get_default_dtype() == torch.float64      # the forward's torch.zeros(...) buffers follow it (see the header)
    m = Module(cfg["n"], AH.FEATURE_DIM, AH.EMBED_DIM, cfg["module_degree"]).double()
    m.load_state_dict({k: v.double() for k, v in sc["state"].items()})
    f = sc["features"].double().requires_grad_(True)
    d = sc["dirs"].double().requires_grad_(True)
    out = m(f, sc["ids"], d, cfg["degree"])
    assert out.dtype == torch.float64 and out.shape == d.shape
    (out * sc["v_out"].double()).sum().backward()
    res = dict(out=out.detach(), v_features=f.grad, v_dirs=d.grad)
    for k, p in m.named_parameters():
        res["grad." + k] = torch.zeros_like(p) if p.grad is None else p.grad
    assert sorted(k[5:] for k in res if k.startswith("grad.")) == sorted(AH.KEYS)
    return res


def main():
    Module = load_reference(sys.argv[1])
    gold = os.path.join(ROOT, "tests", "golden")
    for name, cfg in SCENES.items():
        sc = AH.random_scene(cfg["n"], cfg["C"], cfg["N"], cfg["module_degree"], cfg["degree"], cfg["ids"], seed0=0 if name == "a" else 100000)
        lo, err = AH.relu_margin(sc["state"], sc["features"], sc["ids"], sc["dirs"], cfg["degree"])
        assert lo >= sc["margin"] == 16 * err
        torch.set_default_dtype(torch.float64)
        try:
            res = run(Module, sc, cfg)
        finally:
            torch.set_default_dtype(torch.float32)
        f32 = AH.forward({k: v.float() for k, v in sc["state"].items()}, sc["features"], sc["ids"], sc["dirs"], cfg["degree"])
        print(f"scene {name}: seed {sc['seed']}, smallest |pre-activation| {lo:.3e}, margin {sc['margin']:.3e}, "
              f"fp32 output error {AH.max_rel(f32.numpy(), res['out'].numpy()):.3e}")
        data = {"state." + k: v.numpy() for k, v in sc["state"].items()}
        data.update(features=sc["features"].numpy(), dirs=sc["dirs"].numpy(), v_out=sc["v_out"].numpy(),
                    embed_ids=np.asarray(cfg["ids"] if cfg["ids"] is not None else [], np.int64), has_ids=np.bool_(cfg["ids"] is not None),
                    degree=np.int64(cfg["degree"]), module_degree=np.int64(cfg["module_degree"]), seed=np.int64(sc["seed"]),
                    margin=np.float64(sc["margin"]))
        data.update({k: v.numpy() for k, v in res.items()})
        np.savez(os.path.join(gold, f"appearance_{name}.npz"), **data)


if __name__ == "__main__":
    main()
