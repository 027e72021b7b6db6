"""Inputs shared by tests/test_geometry_cpu.py and tests/test_geometry_edges_gpu.py (plain numpy / torch on the host, no GPU)."""
import numpy as np
import torch

VOXEL = 0.002          # prune_gs's default voxel size


def prune_boundary_coords():
    """fp32(k * 0.002) for k in [-3000, 3000] with both neighbouring floats: 18 003 coordinates at and next to voxel boundaries,
    where floor(m / v) is decided by the last bit of the quotient (k = 0 gives +-the smallest denormal)."""
    c = (np.arange(-3000, 3001, dtype=np.float64) * VOXEL).astype(np.float32)
    return np.stack([np.nextafter(c, np.float32(-np.inf)), c, np.nextafter(c, np.float32(np.inf))], 1).reshape(-1)


def voxel_true_quotient(m, voxel=VOXEL):
    """floor of the correctly rounded fp32 quotient: what the reference's `means / voxel_size` takes on the CPU"""
    return np.floor(np.asarray(m, np.float32) / np.float32(voxel)).astype(np.int64)


def voxel_by_reciprocal(m, voxel=VOXEL):
    """floor of m * fp32(1 / v): what a kernel that trades the division for a multiplication would take"""
    return np.floor(np.asarray(m, np.float32) * (np.float32(1.0) / np.float32(voxel))).astype(np.int64)


def _attributes(n, g, weights):
    return {"quats": torch.randn(n, 4, generator=g), "scales": torch.rand(n, 3, generator=g) * 0.05, "opacities": torch.rand(n, generator=g),
            "sh": torch.randn(n, 1, 3, generator=g), "weights": weights}


def prune_boundary_splats(axis):
    """The boundary coordinates on `axis` (shuffled, so that index order is not voxel order), the other two axes mid-voxel; distinct weights."""
    g = torch.Generator().manual_seed(100 + axis)
    c = torch.from_numpy(prune_boundary_coords())
    n = c.numel()
    means = torch.empty(n, 3)
    means[:] = torch.tensor([0.301, -0.701, 1.101])          # 150.5, -350.5 and 550.5 voxels: far from a boundary
    means[:, axis] = c[torch.randperm(n, generator=g)]
    weights = (1.0 + torch.randperm(n, generator=g).float()) / n          # distinct, in (0, 1]
    return dict(means=means, **_attributes(n, g, weights))


def prune_order_splats():
    """4096 splats inside a 0.0005 cube (8 voxels at most), weights over six decades: fp32 sums depend on the order of the additions"""
    n = 4096
    g = torch.Generator().manual_seed(4096)
    means = (torch.rand(n, 3, generator=g) - 0.5) * 0.0005 + torch.tensor([0.3, -0.7, 1.1])
    weights = 10.0 ** (torch.rand(n, generator=g) * 6.0 - 3.0)
    return dict(means=means, **_attributes(n, g, weights))


def prune_small_splats(n, one_voxel):
    """n splats, each in a voxel of its own along x (negative and positive voxel indices) or all inside one voxel"""
    g = torch.Generator().manual_seed(7 * n + int(one_voxel))
    if one_voxel:
        means = torch.tensor([-0.301, 0.701, -1.101]) + (torch.rand(n, 3, generator=g) - 0.5) * 0.0008
    else:
        means = torch.empty(n, 3)
        means[:, 0] = (torch.randperm(n, generator=g).float() - n // 2) * 0.002 + 0.001
        means[:, 1:] = (torch.rand(n, 2, generator=g) - 0.5) * 0.1
    return dict(means=means, **_attributes(n, g, torch.rand(n, generator=g) + 1e-3))
