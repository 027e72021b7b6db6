"""CPU: the C-ABI library loads, exports every symbol include/wm_hip.h declares, and its host-side
helpers (no GPU needed) match torch: bicubic-antialias pos-embed resample, 16-bit rounding."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

LIB = os.path.join(ROOT, "hunyuanworld-mirror_amd", "libwm_hip.so")


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build()
    return C.CDLL(LIB)


def test_exports_match_header(L):
    hdr = open(os.path.join(ROOT, "include", "wm_hip.h")).read()
    names = set(re.findall(r"\b(wm_[a-z0-9_]+)\s*\(", hdr))
    names -= {"wm_status"}
    from hunyuanworld_mirror_amd import _lib
    assert names == set(_lib.EXPORTS), names ^ set(_lib.EXPORTS)
    for n in names:
        assert hasattr(L, n), n


_C_SCALARS = {"int": C.c_int, "int32_t": C.c_int, "wm_status": C.c_int, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t,
              "int64_t": C.c_int64, "unsigned long long": C.c_ulonglong}


def _ctype_matches(decl, ctype):
    """Does the ctypes class `ctype` pass what the C declaration `decl` (a parameter with its name, or a return type) takes?"""
    if "*" in decl or "[" in decl:
        if ctype is C.c_char_p:
            return re.match(r"const\s+char\s*\*", decl) is not None
        return ctype is C.c_void_p or (isinstance(ctype, type) and issubclass(ctype, C._Pointer))
    return ctype is _C_SCALARS[decl]      # an unknown scalar type is a KeyError: teach the table, do not skip


def test_ctypes_table_matches_header_prototypes(L):
    """Every prototype of include/wm_hip.h against the argtypes / restype that _lib.lib() declares: the same number of arguments, a
    pointer where the header has one (`*` or `[]`), the same scalar type elsewhere, and the same return class (ctypes' default c_int
    where restype is unset).  An entry without argtypes fails, and so does a prototype the pattern below cannot read."""
    raw = open(os.path.join(ROOT, "include", "wm_hip.h")).read()
    names = set(re.findall(r"\b(wm_[a-z0-9_]+)\s*\(", raw)) - {"wm_status"}       # as test_exports_match_header finds them
    hdr = re.sub(r"/\*.*?\*/", " ", raw, flags=re.S)
    hdr = re.sub(r"//[^\n]*", " ", hdr)
    hdr = re.sub(r"^\s*#[^\n]*", " ", hdr, flags=re.M)
    protos = {m.group(2): (m.group(1), m.group(3)) for m in re.finditer(r"([^;{}()]*?)\b(wm_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", hdr)}
    assert set(protos) == names, set(protos) ^ names
    from hunyuanworld_mirror_amd import _lib
    lib = _lib.lib()
    bad = []
    for name, (ret, args) in sorted(protos.items()):
        fn = getattr(lib, name)
        params = [" ".join(a.split()) for a in args.split(",")]
        params = [] if params == ["void"] else params
        if fn.argtypes is None:
            bad.append(f"{name}: no argtypes")
            continue
        if len(fn.argtypes) != len(params):
            bad.append(f"{name}: {len(fn.argtypes)} argtypes, {len(params)} parameters")
            continue
        for i, (p, t) in enumerate(zip(params, fn.argtypes)):
            # a scalar parameter is `[const] type name`: drop the qualifier and the name
            decl = p if ("*" in p or "[" in p) else " ".join(w for w in p.split()[:-1] if w != "const")
            if not _ctype_matches(decl, t):
                bad.append(f"{name}: argument {i} `{p}` declared as {t.__name__}")
        ret = " ".join(w for w in ret.split() if w != "extern")
        if ret == "void":
            ok = fn.restype is None
        else:
            ok = fn.restype is not None and _ctype_matches(ret, fn.restype)
        if not ok:
            bad.append(f"{name}: returns `{ret}`, restype {getattr(fn.restype, '__name__', fn.restype)}")
    assert not bad, "\n".join(bad)


def test_shipped_library_reads_no_wm_environment_switch(L):
    """The product build must not be steerable from the environment (a WM_ATTN_DEBUG_SKIP in the shipped library could
    return wrong results).  The environment layer that every historical WM_* switch went through is gone from the sources — neither its
    accessor nor the build flag that enabled it may come back anywhere under csrc/, the Makefile included — so no such name may be
    left among the library's strings.  (getenv itself is still imported: rocPRIM's headers in raster / splat_prune.)"""
    data = open(LIB, "rb").read()
    names = set(m.decode() for m in re.findall(rb"WM_[A-Z][A-Z0-9_]{3,}", data))
    names -= {"WM_OK"}
    envlike = sorted(n for n in names if not n.startswith(("WM_ERR", "WM_EPI", "WM_T_", "WM_ACT", "WM_TUNE", "WM_RCCL")))
    assert not envlike, envlike
    src = os.path.join(ROOT, "hunyuanworld-mirror_amd", "csrc")
    retired = ("wm_" + "env", "WM_DIAG_" + "ENV")    # (spelled in two parts: this file is searched for them too)
    for f in os.listdir(src):
        path = os.path.join(src, f)
        if not os.path.isfile(path) or f.endswith((".o", ".so")):
            continue
        text = open(path, errors="replace").read()
        if f.endswith((".hip", ".cpp")):
            assert "getenv(" not in text, f
        for name in retired:
            assert name not in text, (f, name)


def test_orchestrator_internals_are_not_exported(L):
    """The orchestrator's translation units share their types and functions through csrc/wm_model.h, in the namespace wm_host with hidden
    visibility: none of it may reach the library's dynamic symbol table, which holds the C ABI (the entries wm_host_to_16 and
    wm_host_resample_pos are C names, not members of the namespace)."""
    import shutil
    import subprocess
    nm = shutil.which("nm") or shutil.which("llvm-nm")
    if nm is None and os.path.exists("/opt/rocm/llvm/bin/llvm-nm"):
        nm = "/opt/rocm/llvm/bin/llvm-nm"
    if nm is None:
        pytest.skip("neither nm nor llvm-nm on this machine")
    out = subprocess.run([nm, "-D", "--defined-only", "-C", LIB], check=True, capture_output=True, text=True).stdout
    assert "wm_set_tuning" in out, "the symbol listing does not show the C ABI either"
    leaked = [l for l in out.splitlines() if "wm_host::" in l]
    assert not leaked, leaked
    raw = subprocess.run([nm, "-D", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    assert not [l for l in raw.splitlines() if "7wm_host" in l], "mangled names of the namespace"


def test_forward_files_create_no_queue():
    """The forward records, waits and launches: the sources that hold the forward path create no stream and no event (wm_reserve and the
    communicator-init entries do) and allocate nothing."""
    src = os.path.join(ROOT, "hunyuanworld-mirror_amd", "csrc")
    for f in ("wm_model.cpp", "wm_backbone.cpp", "wm_heads.cpp"):
        text = open(os.path.join(src, f)).read()
        for call in ("hipStreamCreate", "hipEventCreateWithFlags", "hipMalloc", "hipHostMalloc"):
            assert call not in text, (f, call)


# the key strings of wm_set_tuning before the table became a single list (wm_model.cpp of that commit): tests, tools and bench.py
# call them by these spellings
TUNING_KEYS_BEFORE_TABLE = ["gemm_cfg", "gemm_pp", "gemm_mfma16", "attn_qb", "op_ldpad", "attn_splits", "conv_fuse_up", "conv_narrow", "conv_bn",
                            "conv_rs", "lin_mfma", "conv_tpx", "attn_tail", "gemm_group", "comm_overlap", "heads_concurrent", "rcu_mid16", "gemm_sched",
                            "force_gather", "attn_op_policy", "comm_p2p", "ln_rpw", "ln_fuse", "heads_main", "conv_gemm", "resid_prefetch", "up1_gather",
                            "tconv", "up1_comp"]


def test_tuning_table_is_one_list(L):
    """wm_kernels.h declares the tuning keys once (WM_TUNE_KEYS: enum name, key string); the enum, the name array of wm_set_tuning
    and the all-unset initialiser are generated from it.  Every listed key is accepted (setting -1 = not set changes nothing), an
    unknown key is refused with -1, INTEGRATION.md documents every key, and none of the 29 earlier key strings has been lost."""
    hdr = open(os.path.join(ROOT, "hunyuanworld-mirror_amd", "csrc", "wm_kernels.h")).read()
    body = hdr[hdr.index("#define WM_TUNE_KEYS(X)"):]
    body = body[:body.index("#define WM_TUNE_ENUM")]
    pairs = re.findall(r'^\s*X\((\w+),\s*"(\w+)"\)', body, flags=re.M)
    keys = [k for _, k in pairs]
    assert len(keys) >= 29 and len(set(keys)) == len(keys) and len(set(n for n, _ in pairs)) == len(pairs), pairs
    assert len(pairs) == body.count("X("), "a line of the table the pattern does not read"
    assert len(TUNING_KEYS_BEFORE_TABLE) == 29
    assert set(TUNING_KEYS_BEFORE_TABLE) <= set(keys), set(TUNING_KEYS_BEFORE_TABLE) - set(keys)
    assert keys[:29] == TUNING_KEYS_BEFORE_TABLE      # and in their order: new keys are appended
    L.wm_set_tuning.restype = C.c_int
    L.wm_set_tuning.argtypes = [C.c_char_p, C.c_int]
    for k in keys:
        assert L.wm_set_tuning(k.encode(), -1) == 0, k
    assert L.wm_set_tuning(b"no_such_key", -1) == -1
    assert L.wm_set_tuning(b"", -1) == -1 and L.wm_set_tuning(None, -1) == -1
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for k in keys:
        assert "`" + k + "`" in doc, k
    assert [doc.index("| `" + k + "` |") for k in keys] == sorted(doc.index("| `" + k + "` |") for k in keys), "INTEGRATION.md: table order"


def test_config_struct_layout_matches_header():
    from hunyuanworld_mirror_amd import _lib
    assert C.sizeof(_lib.wm_config) == 4 * (4 + 6 + 4 + 4 + 1 + 2 + 3 + 1 + 4 + 2)
    assert C.sizeof(_lib.wm_outputs) == 8 * 21


@pytest.mark.parametrize("gh,gw", [(5, 4), (4, 5), (3, 3), (16, 16), (7, 5)])
def test_host_pos_resample_matches_torch(L, gh, gw):
    gs, D = 5, 8
    g = torch.Generator().manual_seed(gh * 10 + gw)
    src = torch.randn(gs * gs, D, generator=g)
    out = np.empty((gh * gw, D), np.float32)
    L.wm_host_resample_pos.restype = None
    L.wm_host_resample_pos(C.c_void_p(src.numpy().ctypes.data), gs, D, gh, gw, C.c_void_p(out.ctypes.data))
    ref = torch.nn.functional.interpolate(src.reshape(1, gs, gs, D).permute(0, 3, 1, 2), size=(gh, gw), mode="bicubic",
                                          antialias=True).permute(0, 2, 3, 1).reshape(gh * gw, D)
    assert np.abs(out - ref.numpy()).max() < 2e-6


def test_host_to_16(L):
    x = torch.randn(1000) * 100
    x[0], x[1], x[2] = float("nan"), float("inf"), 0.0
    out = np.empty(1000, np.uint16)
    L.wm_host_to_16.restype = None
    for dt, tdt in ((0, torch.bfloat16), (1, torch.float16)):
        L.wm_host_to_16(C.c_void_p(x.numpy().ctypes.data), C.c_void_p(out.ctypes.data), C.c_size_t(1000), dt)
        ref = x.to(tdt).view(torch.int16).numpy().view(np.uint16)
        ok = (out == ref) | (np.isnan(x.numpy()))
        assert ok.all()
        assert np.isnan(torch.from_numpy(out.view(np.int16)).view(tdt).float()[0])


def test_product_path_has_no_cpu_fallback():
    from hunyuanworld_mirror_amd import WorldMirror, WMConfig
    m = WorldMirror(arch=WMConfig.tiny())
    with pytest.raises(RuntimeError):
        m.to("cpu")
    with pytest.raises(RuntimeError):
        m({"img": torch.rand(1, 1, 3, 70, 70)})


def test_param_spec_counts():
    from hunyuanworld_mirror_amd import WMConfig, param_spec
    n = sum(int(np.prod(s)) for s in param_spec(WMConfig()).values())
    assert abs(n - 1.230e9) / 1.230e9 < 2e-3          # 1.230 B parameters without GS
    n_gs = sum(int(np.prod(s)) for s in param_spec(WMConfig(enable_gs=True)).values())
    assert abs(n_gs - 1.263e9) / 1.263e9 < 2e-3


def test_from_pretrained_local_dir(tmp_path):
    """WorldMirror.from_pretrained(<local dir>) (infer.py:95 / app.py:104 with a local path; PyTorchModelHubMixin layout:
    config.json = ctor kwargs, model.safetensors): fp32 and bf16 tensors, an unexpected key (ignored) and a missing key
    (reported, left at its init value) — no GPU needed, the weights stay on the host until .to()."""
    import json
    import torch
    from safetensors.torch import save_file
    from hunyuanworld_mirror_amd import WorldMirror, WMConfig
    from hunyuanworld_mirror_amd.weights import iter_params
    cfg = WMConfig.tiny()
    kw = dict(img_size=cfg.img_size, patch_size=cfg.patch_size, embed_dim=cfg.embed_dim, gs_dim=cfg.gs_dim, enable_cond=True, enable_cam=True,
              enable_pts=True, enable_depth=True, enable_norm=True, enable_gs=False, patch_embed="dinov2_vitl14_reg", fixed_patch_embed=False,
              sampling_strategy="uniform", dpt_gradient_checkpoint=False, condition_strategy=["token", "pow3r", "token"],
              enable_interpolation=False, max_resolution=2044)
    sd = {k: torch.from_numpy(v.copy()) for k, v in iter_params(cfg)}
    names = sorted(sd)
    dropped, as_bf16 = names[3], names[5]
    ref_bf16 = sd[as_bf16].to(torch.bfloat16)
    sd[as_bf16] = ref_bf16
    del sd[dropped]
    sd["not.a.parameter"] = torch.zeros(3)
    d = tmp_path / "ckpt"
    d.mkdir()
    # metadata keys that huggingface_hub adds to config.json: PyTorchModelHubMixin filters config.json to the constructor's
    # signature (worldmirror.py:13,16), so they must not reach the constructor
    (d / "config.json").write_text(json.dumps({**kw, "model_type": "worldmirror", "library_name": "pytorch", "_hub_version": "0.x"}))
    save_file(sd, str(d / "model.safetensors"))
    m = WorldMirror.from_pretrained(str(d), arch=cfg)   # arch: the scaled-down test architecture behind the same kwargs
    assert dropped not in m._host_weights and "not.a.parameter" not in m._host_weights
    assert np.array_equal(m._host_weights[as_bf16], ref_bf16.float().numpy())
    k0 = names[0]
    assert np.array_equal(m._host_weights[k0], sd[k0].numpy())
    with pytest.raises(FileNotFoundError):
        WorldMirror.from_pretrained("tencent/HunyuanWorld-Mirror")   # a hub name: no network here, local directories only
