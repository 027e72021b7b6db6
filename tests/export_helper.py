"""A vectorised torch restatement of gsplat's export_splats ("ply", "splat", "ply_compressed"; gsplat/exporter.py) and of save_gs_ply
(src/utils/save_utils.py), in fp32 in the reference's operation order, on whatever device the tensors are on.  Pinned to the
reference's own bytes through tests/golden/export_{a,b,c}.npz (tools/gen_golden_export.py, tests/test_export_cpu.py); the reference
for the GPU tests at sizes the goldens do not hold; the torch composition tools/bench_export.py times.

Where the reference leaves the answer undefined this file takes the definitions of csrc/export.hip:
  * a chunk quantity with max == min packs as field 0 (the reference: 0 / 0 = NaN, then an undefined integer cast)
  * no kept row gives a valid file with zero elements (the reference: torch.min of an empty tensor raises)
  * a non-finite opacity drops that row alone (the reference's `.any(dim=0)` on the 1-D opacities drops every row)

There is no golden for save_gs_ply: the reference writes it through the `plyfile` package, which is not available here, so its header
is restated from the PLY format (one element `vertex`, `property float <name>` per column), not pinned to the package's output.

compare() holds two files of one format to each other by the rule of the tests: every byte equal except the fields whose value goes
through a norm or an exponential (last-ulp rounding differs between libraries)."""
import math
import os

import numpy as np
import torch

C0 = 0.28209479177387814
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CHUNK = 256
CHUNK_PROPS = ["min_x", "min_y", "min_z", "max_x", "max_y", "max_z", "min_scale_x", "min_scale_y", "min_scale_z", "max_scale_x", "max_scale_y",
               "max_scale_z", "min_r", "min_g", "min_b", "max_r", "max_g", "max_b"]
FORMATS = ("ply", "splat", "ply_compressed")
NAMES = ("means", "scales", "quats", "opacities", "sh0", "shN")


def load_golden(name):
    return np.load(os.path.join(GOLDEN, f"export_{name}.npz"))


def scene_tensors(z, device="cpu"):
    return [torch.from_numpy(z[k]).to(device) for k in NAMES]


# ------------------------------------------------------------------ headers
def header(fmt, n, K):
    if fmt == "splat":
        return b""
    if fmt == "ply":
        props = ["x", "y", "z"] + [f"f_dc_{j}" for j in range(3)] + [f"f_rest_{j}" for j in range(3 * K)] + ["opacity"]
        props += [f"scale_{j}" for j in range(3)] + [f"rot_{j}" for j in range(4)]
        return float_header(n, props)
    lines = ["ply", "format binary_little_endian 1.0", f"element chunk {(n + CHUNK - 1) // CHUNK}"] + [f"property float {p}" for p in CHUNK_PROPS]
    lines += [f"element vertex {n}"] + [f"property uint packed_{p}" for p in ("position", "rotation", "scale", "color")]
    lines += [f"element sh {n}"] + [f"property uchar f_rest_{j}" for j in range(3 * K)] + ["end_header"]
    return ("\n".join(lines) + "\n").encode()


def float_header(n, props):
    return ("\n".join(["ply", "format binary_little_endian 1.0", f"element vertex {n}"] + [f"property float {p}" for p in props] + ["end_header"])
            + "\n").encode()


GS_PLY_PROPS = ["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2", "opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1",
                "rot_2", "rot_3"]


# ------------------------------------------------------------------ stages
def keep_mask(means, scales, quats, opacities, sh0, shN, fmt):
    """rows whose every number is finite; ply_compressed: and sigmoid(opacity) > 1 / 255"""
    N = means.shape[0]
    ok = torch.isfinite(opacities)
    for t in (means, scales, quats, sh0.reshape(N, -1), shN.reshape(N, -1)):
        ok = ok & torch.isfinite(t).all(dim=1)
    if fmt == "ply_compressed":
        ok = ok & (torch.sigmoid(opacities) > 1 / 255)
    return ok


def _part1by2(x):
    x = x & 0x000003FF
    x = (x ^ (x << 16)) & 0xFF0000FF
    x = (x ^ (x << 8)) & 0x0300F00F
    x = (x ^ (x << 4)) & 0x030C30C3
    x = (x ^ (x << 2)) & 0x09249249
    return x


def morton_codes(centers):
    lo, hi = centers.min(dim=0).values, centers.max(dim=0).values
    length = hi - lo
    length = torch.where(length == 0, torch.ones_like(length), length)
    q = ((centers - lo) / length * 1024).floor().to(torch.int32).to(torch.int64)
    return (_part1by2(q[:, 2]) << 2) + (_part1by2(q[:, 1]) << 1) + _part1by2(q[:, 0])


def morton_order(centers):
    """positions of the rows in Morton order; equal codes stay in row order"""
    return torch.argsort(morton_codes(centers), stable=True)


def _pack_unorm(v, bits):
    t = (1 << bits) - 1
    p = torch.clamp((v * t + 0.5).floor(), min=0, max=t)
    return torch.where(torch.isnan(p), torch.zeros_like(p), p).to(torch.int64)


def _normalise(v, lo, hi):
    rng = hi - lo
    safe = torch.where(rng == 0, torch.ones_like(rng), rng)
    return torch.where(rng == 0, torch.zeros_like(v), (v - lo) / safe)


def _bytes(t, dtype):
    return t.detach().cpu().numpy().astype(dtype).tobytes()


def _pack_rotation(q):
    q = q / torch.linalg.norm(q, dim=-1, keepdim=True)
    big = torch.argmax(torch.abs(q), dim=-1)
    lead = q.gather(1, big[:, None])
    q = torch.where(lead < 0, -q, q)
    others = torch.tensor([[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]], dtype=torch.long, device=q.device)[big]
    comp = q.gather(1, others)
    packed = _pack_unorm(comp * (math.sqrt(2) * 0.5) + 0.5, 10)
    return (big.to(torch.int64) << 30) | (packed[:, 0] << 20) | (packed[:, 1] << 10) | packed[:, 2]


# ------------------------------------------------------------------ bodies (of kept rows; shN [n,K,3])
def body_ply(means, scales, quats, opacities, sh0, shN):
    n = means.shape[0]
    rest = shN.permute(0, 2, 1).reshape(n, 3 * shN.shape[1])
    return _bytes(torch.cat([means, sh0.reshape(n, 3), rest, opacities[:, None], scales, quats], dim=1).float(), "<f4")


def body_splat(means, scales, quats, opacities, sh0, shN):
    n = means.shape[0]
    if n == 0:
        return b""
    colors = torch.cat([sh0.reshape(n, 3) * C0 + 0.5, torch.sigmoid(opacities)[:, None]], dim=1)
    colors = (colors * 255).clamp(0, 255).to(torch.uint8)
    rots = ((quats / torch.linalg.norm(quats, dim=1, keepdim=True)) * 128 + 128).clamp(0, 255)
    rots = torch.where(torch.isnan(rots), torch.zeros_like(rots), rots).to(torch.uint8)
    order = morton_order(means)
    rec = np.zeros((n, 32), np.uint8)
    rec[:, 0:12] = means[order].detach().cpu().numpy().astype("<f4").view(np.uint8).reshape(n, 12)
    rec[:, 12:24] = torch.exp(scales)[order].detach().cpu().numpy().astype("<f4").view(np.uint8).reshape(n, 12)
    rec[:, 24:28] = colors[order].cpu().numpy()
    rec[:, 28:32] = rots[order].cpu().numpy()
    return rec.tobytes()


def body_ply_compressed(means, scales, quats, opacities, sh0, shN):
    n, K = means.shape[0], shN.shape[1]
    if n == 0:
        return b""
    order = morton_order(means)
    colors = sh0.reshape(n, 3) * C0 + 0.5
    vals = torch.cat([means, scales, colors], dim=1)[order]                 # [n, 9] in Morton order
    nc = (n + CHUNK - 1) // CHUNK
    pad = nc * CHUNK - n
    live = torch.cat([torch.ones(n, dtype=torch.bool, device=means.device), torch.zeros(pad, dtype=torch.bool, device=means.device)]).reshape(nc, CHUNK, 1)
    padded = torch.cat([vals, vals.new_zeros(pad, 9)]).reshape(nc, CHUNK, 9)
    lo = torch.where(live, padded, torch.full_like(padded, float("inf"))).amin(dim=1)        # [nc, 9]
    hi = torch.where(live, padded, torch.full_like(padded, float("-inf"))).amax(dim=1)
    lo[:, 3:6] = lo[:, 3:6].clamp(-20, 20)
    hi[:, 3:6] = hi[:, 3:6].clamp(-20, 20)
    chunk_floats = torch.cat([lo[:, 0:3], hi[:, 0:3], lo[:, 3:6], hi[:, 3:6], lo[:, 6:9], hi[:, 6:9]], dim=1)
    chunk_of = torch.arange(n, device=means.device) // CHUNK
    nrm = _normalise(vals, lo[chunk_of], hi[chunk_of])
    pos = (_pack_unorm(nrm[:, 0], 11) << 21) | (_pack_unorm(nrm[:, 1], 10) << 11) | _pack_unorm(nrm[:, 2], 11)
    scl = (_pack_unorm(nrm[:, 3], 11) << 21) | (_pack_unorm(nrm[:, 4], 10) << 11) | _pack_unorm(nrm[:, 5], 11)
    alpha = 1 / (1 + torch.exp(-opacities[order]))
    col = (_pack_unorm(nrm[:, 6], 8) << 24) | (_pack_unorm(nrm[:, 7], 8) << 16) | (_pack_unorm(nrm[:, 8], 8) << 8) | _pack_unorm(alpha, 8)
    rot = _pack_rotation(quats[order])
    verts = torch.stack([pos, rot, scl, col], dim=1)
    rest = shN.permute(0, 2, 1).reshape(n, 3 * K)[order]
    shq = torch.clamp(torch.trunc((rest / 8 + 0.5) * 256), 0, 255).to(torch.uint8)
    return _bytes(chunk_floats, "<f4") + _bytes(verts, "<u4") + _bytes(shq, np.uint8)


BODIES = {"ply": body_ply, "splat": body_splat, "ply_compressed": body_ply_compressed}


def export_splats(means, scales, quats, opacities, sh0, shN, format="ply"):
    """-> (file bytes, rows kept)"""
    keep = keep_mask(means, scales, quats, opacities, sh0, shN, format)
    kept = [t[keep].float() for t in (means, scales, quats, opacities, sh0, shN)]
    n = int(keep.sum())
    return header(format, n, shN.shape[1]) + BODIES[format](*kept), n


def save_gs_ply(means, scales, rotations, rgbs, opacities):
    """-> (file bytes, rows kept): rows with max scale <= the 0.95 quantile of the max scales; zero normals, log scales"""
    largest = scales.max(dim=-1)[0]
    keep = largest <= torch.quantile(largest, 0.95, dim=0)
    m, s, q, c, o = (t[keep] for t in (means, scales, rotations, rgbs, opacities))
    data = torch.cat([m.float(), torch.zeros_like(m).float(), c, o[..., None], s.log(), q], dim=1)
    return float_header(m.shape[0], GS_PLY_PROPS) + _bytes(data, "<f4"), int(keep.sum())


# ------------------------------------------------------------------ comparison by the rule of the tests
def split(data, fmt, K):
    """file bytes -> (header bytes, n, sections as numpy arrays)"""
    if fmt == "splat":
        return b"", len(data) // 32, {"records": np.frombuffer(data, np.uint8).reshape(-1, 32)}
    end = data.index(b"end_header\n") + len(b"end_header\n")
    head, body = data[:end], data[end:]
    n = int([l for l in head.decode().split("\n") if l.startswith("element vertex")][0].split()[2])
    if fmt == "ply":
        return head, n, {"rows": np.frombuffer(body, "<u4").reshape(n, 14 + 3 * K)}
    nc = (n + CHUNK - 1) // CHUNK
    assert len(body) == nc * 72 + n * 16 + n * 3 * K, (len(body), n, K)
    return head, n, {"chunks": np.frombuffer(body, "<u4", nc * 18), "verts": np.frombuffer(body, "<u4", n * 4, nc * 72).reshape(n, 4),
                     "sh": np.frombuffer(body, np.uint8, n * 3 * K, nc * 72 + n * 16)}


def ulp_distance(a_bits, b_bits):
    """distance in units of the last place between fp32 numbers given as their uint32 bit patterns"""
    def ordered(u):
        u = u.astype(np.int64)
        return np.where(u & 0x80000000, 0x80000000 - u, u)
    return np.abs(ordered(a_bits) - ordered(b_bits))


def flip_cap(n):
    return max(1, n // 1000)           # max(1, 0.1 % of the splats)


def compare(got, ref, fmt, K, float_ulp=4):
    """Holds `got` to `ref`.  Identical: headers, record order, chunk bounds, packed position / scale / colour, sh bytes, the whole ply body.
    Integer exceptions (off by at most one unit, in at most flip_cap(n) fields per file): the three 10-bit rotation fields and the opacity
    byte of ply_compressed; the four rotation bytes and the alpha byte of .splat.  Float exception: exp(scale) of .splat within float_ulp.
    -> dict(n, flips, max_ulp)"""
    hg, ng, sg = split(got, fmt, K)
    hr, nr, sr = split(ref, fmt, K)
    assert hg == hr, (hg[-200:], hr[-200:])
    assert ng == nr and len(got) == len(ref), (ng, nr, len(got), len(ref))
    flips, max_ulp = 0, 0
    if fmt == "ply":
        assert np.array_equal(sg["rows"], sr["rows"]), f"{int((sg['rows'] != sr['rows']).sum())} ply floats differ"
    elif fmt == "splat":
        a, b = sg["records"], sr["records"]
        assert np.array_equal(a[:, 0:12], b[:, 0:12]), "means / record order differ"
        assert np.array_equal(a[:, 24:27], b[:, 24:27]), "colour bytes differ"
        if ng:
            d = ulp_distance(np.ascontiguousarray(a[:, 12:24]).view("<u4"), np.ascontiguousarray(b[:, 12:24]).view("<u4"))
            max_ulp = int(d.max())
            assert max_ulp <= float_ulp, f"exp(scale) off by {max_ulp} ulp"
        d = np.abs(a[:, 27:32].astype(np.int64) - b[:, 27:32].astype(np.int64))
        assert d.max(initial=0) <= 1, f"alpha / rotation byte off by {int(d.max())}"
        flips = int((d != 0).sum())
    else:
        assert np.array_equal(sg["chunks"], sr["chunks"]), "chunk bounds differ"
        assert np.array_equal(sg["sh"], sr["sh"]), "sh bytes differ"
        a, b = sg["verts"].astype(np.int64), sr["verts"].astype(np.int64)
        assert np.array_equal(a[:, 0], b[:, 0]), "packed positions / record order differ"
        assert np.array_equal(a[:, 2], b[:, 2]), "packed scales differ"
        assert np.array_equal(a[:, 3] >> 8, b[:, 3] >> 8), "packed colours differ"
        assert np.array_equal(a[:, 1] >> 30, b[:, 1] >> 30), "largest rotation component differs"
        fields = [((a[:, 1] >> s) & 1023, (b[:, 1] >> s) & 1023) for s in (20, 10, 0)] + [(a[:, 3] & 255, b[:, 3] & 255)]
        for x, y in fields:
            d = np.abs(x - y)
            assert d.max(initial=0) <= 1, f"rotation / opacity field off by {int(d.max())}"
            flips += int((d != 0).sum())
    assert flips <= flip_cap(ng), f"{flips} fields off by one, cap {flip_cap(ng)} for {ng} splats"
    return {"n": ng, "flips": flips, "max_ulp": max_ulp}
