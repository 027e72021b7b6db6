"""What the passes around the fast cross-view attention kernel cost per call: the recompute pass (the general kernel launched over the
same grid, every block leaving at its flag) and the combine pass of the tail split.  Needs a library built with
`make -C hunyuanworld-mirror_amd/csrc stamps` (-DWM_ATTN_TIMING_EXPERIMENT; WM_HIP_LIB=...libwm_hip_stamps.so): there the tuning
`attn_debug_skip` = 1 skips the recompute pass, 2 the combine pass, 3 both (wrong results).  python tools/attn_launch_cost.py [views].  Timing only."""
import ctypes as C, json, sys
import torch
sys.path.insert(0, '.')
from hunyuanworld_mirror_amd import _lib
L = _lib.lib(); dev = torch.device('cuda:0')
p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
H = 16
for nv in [int(x) for x in sys.argv[1:]] or [8, 32]:
    M = nv * 1376
    g = torch.Generator(device="cpu").manual_seed(1)
    q = (torch.randn(H, M, 64, generator=g) * 0.125 * 1.4427 * 1.5).to(torch.bfloat16).to(dev)
    k = (torch.randn(1, H, M, 64, generator=g) * 1.5).to(torch.bfloat16).to(dev)
    v = torch.randn(1, H, M, 64, generator=g).to(torch.bfloat16).to(dev)
    o = torch.empty(M, H * 64, device=dev, dtype=torch.int16)
    po = torch.empty(8, M, H * 64, device=dev); pml = torch.empty(8, H, M, 2, device=dev)
    flags = torch.zeros((int(L.wm_op_attention_flag_count(M, M, H)),), device=dev, dtype=torch.int32)
    def run():
        assert L.wm_op_attention_ex(0, p(q), p(k), p(v), p(o), H, M, M, 1, 0, 0, p(po), p(pml), p(flags), s) == 0
    for _ in range(10): run()
    torch.cuda.synchronize()
    for skip in (0, 1, 2, 3):
        assert L.wm_set_tuning(b"attn_debug_skip", skip) == 0
        res = []
        for rep in range(3):
            n = 40 if nv <= 8 else 10
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n): run()
            e1.record(); torch.cuda.synchronize()
            res.append(round(e0.elapsed_time(e1) / n * 1e3, 1))
        print(json.dumps({"views": nv, "skip": skip, "us_per_call": res}), flush=True)
    L.wm_set_tuning(b"attn_debug_skip", -1)
