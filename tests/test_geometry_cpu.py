"""Post-path geometry, host side: the oracles the GPU edge tests (tests/test_geometry_edges_gpu.py) compare against are themselves
held against the reference's own statements, and the fixtures are shown to be able to tell a right kernel from a wrong one.

  create_confidence_mask   oracle/geometry_ref against torch.topk on masked_fill(conf <= 1e-5, -inf), the reference's two lines
                           (infer.py:41, :53), on inputs whose K-th value is not tied: NaN of both signs, +-inf, negatives, 1e-5f and
                           its successor, denormals.
  K                        the kept count for (n, p) pairs, among them the four where an fp32 image of p = 33.3 moves K by one.
  prune_gs                 on the boundary fixture floor(m / v) and floor(m * (1 / v)) differ, so the fixture can tell the two apart;
                           the oracle's torch division is the true quotient."""
import numpy as np
import pytest
import torch

import geometry_fixtures as F
from oracle import geometry_ref as G
from oracle import worldmirror_ref as WR


def _bits(u):
    return np.array([u], np.uint32).view(np.float32)[0]


NEG_NAN, POS_NAN = _bits(0xFFC00000), _bits(0x7FC00000)          # 0xFFC00000 is what 0.0 / 0.0 gives on x86


def _reference_mask(conf, percent):
    """infer.py:39-57, its own statements"""
    conf_flat = torch.from_numpy(conf).flatten()
    conf_flat = conf_flat.masked_fill(conf_flat <= 1e-5, float("-inf"))
    N = conf_flat.numel()
    if percent > 0:
        keep_from_percent = int(np.ceil(N * (100.0 - percent) / 100.0))
    else:
        keep_from_percent = N
    K = max(1, keep_from_percent)
    topk_idx = torch.topk(conf_flat, K, largest=True, sorted=False).indices
    conf_mask = torch.zeros_like(conf_flat, dtype=torch.bool)
    conf_mask[topk_idx] = True
    return conf_mask.numpy(), K


def _tie_free_conf():
    g = torch.Generator().manual_seed(11)
    body = np.unique(torch.randn(2000, generator=g).numpy())          # distinct values, about half of them negative
    body = body[torch.randperm(len(body), generator=g).numpy()]
    one_e5 = np.float32(1e-5)
    tiny = np.float32(1e-45)                                          # the smallest denormal
    special = np.array([np.inf, -np.inf, one_e5, np.nextafter(one_e5, np.float32(1)), tiny, -tiny, _bits(0x007FFFFF), 0.0, -0.0], np.float32)
    conf = np.concatenate([body[:700], [NEG_NAN], body[700:1400], special, [POS_NAN], body[1400:]]).astype(np.float32)
    assert np.signbit(conf[700]) and np.isnan(conf[700]) and not np.signbit(conf[1410]) and np.isnan(conf[1410])
    return conf


@pytest.mark.parametrize("percent", [0.0, "all_live", 60.0, 80.0, 99.9, 99.95])
def test_oracle_confidence_mask_is_torch_topk(percent):
    conf = _tie_free_conf()
    n_nan = int(np.isnan(conf).sum())
    n_live = int((np.isnan(conf) | (conf > np.float32(1e-5))).sum())          # everything else (negatives too) is one tied group at -inf
    if percent == "all_live":          # K = n_live: the successor of 1e-5f, the smallest live value, is the K-th
        percent = 100.0 * (1.0 - (n_live - 0.5) / conf.size)
        assert G.confidence_mask_count(conf.size, percent) == n_live
    want, K = _reference_mask(conf, percent)
    assert K == conf.size or n_nan <= K <= n_live, "the K-th value must not be tied, or topk's choice is unspecified"
    got = G.create_confidence_mask(conf, percent)
    assert got.sum() == K
    assert np.array_equal(got, want), percent
    if percent == 99.95:
        assert K == 2 and np.array_equal(np.nonzero(got)[0], [700, 1410]), "the two NaNs, either sign, rank above +inf"
    if percent == 99.9:
        assert K == 3 and got[np.nonzero(np.isposinf(conf))[0][0]]
    # 1e-5f is invalid, its successor valid: the successor is kept as soon as K reaches the live values, 1e-5f only with the -inf group
    succ, e5 = int(np.nonzero(conf == np.nextafter(np.float32(1e-5), np.float32(1)))[0][0]), int(np.nonzero(conf == np.float32(1e-5))[0][0])
    assert got[succ] == (K >= n_live) and got[e5] == (K == conf.size)


def test_oracle_breaks_nan_ties_by_lowest_index():
    """all NaNs are one value: at K = 1 the first one in index order is kept, whatever its sign"""
    for first, second in ((NEG_NAN, POS_NAN), (POS_NAN, NEG_NAN)):
        conf = np.linspace(1.0, 2.0, 3000).astype(np.float32)
        conf[0], conf[40], conf[2000] = np.inf, first, second
        assert G.confidence_mask_count(conf.size, 99.99) == 1
        assert np.array_equal(np.nonzero(G.create_confidence_mask(conf, 99.99))[0], [40])


K_TABLE = [  # (n, p, K); the first four: p = 33.3 is below its fp32 image 33.299999237..., which gives K + 1
    (1000, 33.3, 667), (10000, 33.3, 6670), (100000, 33.3, 66700), (1000000, 33.3, 667000),
    (1000, 30.0, 700), (1000, 0.0, 1000), (1000, 100.0, 1), (1000, 150.0, 1), (1000, -5.0, 1000), (1, 50.0, 1), (7, 99.99, 1),
    (10007, 55.5, 4454), (1000, 66.6, 335), (5000, 1e-9, 5000), (4097, 30.0, 2868), (1048577, 30.0, 734004),
]


@pytest.mark.parametrize("n,p,K", K_TABLE)
def test_kept_count_is_the_reference_formula_in_double(n, p, K):
    want = max(1, int(np.ceil(n * (100.0 - p) / 100.0)) if p > 0 else n)          # infer.py:46-50 in Python floats
    assert want == K
    assert G.confidence_mask_count(n, p) == K
    if n <= 100000:
        conf = np.arange(1, n + 1, dtype=np.float32)
        assert int(G.create_confidence_mask(conf, p).sum()) == K


def test_fp32_percent_moves_the_count():
    """why the entry takes a double: the four pairs above are sharp"""
    for n, p, K in K_TABLE[:4]:
        p32 = float(np.float32(p))
        assert int(np.ceil(n * (100.0 - p32) / 100.0)) == K + 1


def test_prune_boundary_fixture_is_sharp():
    m = F.prune_boundary_coords()
    assert m.size == 18003 and (m < 0).any() and (m > 0).any()
    true_q, recip = F.voxel_true_quotient(m), F.voxel_by_reciprocal(m)
    differ = int((true_q != recip).sum())
    print(f"floor(m / v) != floor(m * (1 / v)) at {differ} of {m.size} boundary coordinates")
    assert differ >= 1
    # the oracle's own quotient (torch on the CPU, worldmirror_ref.prune_gs's first line) is the true one
    assert np.array_equal((torch.from_numpy(m) / F.VOXEL).floor().long().numpy(), true_q)
    for axis in range(3):
        sp = F.prune_boundary_splats(axis)
        assert len(torch.unique(sp["weights"])) == m.size
        K = WR.prune_gs(sp)["means"].shape[0]
        assert K == len(np.unique(true_q)), (axis, K)
