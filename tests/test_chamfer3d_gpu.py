"""lasr_amd.chamfer3D on the GPU: the tiled search against fused_ops.nearest_point bit for bit at every split count, ties across
splits, the reference's own chamfer3D outputs (tests/golden/side_reference_kernels.npz, held as
tests/test_side_kernels_vs_reference_vectors.py holds nearest_point) and the backward against float64 autograd."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_restated as ir                          # noqa: E402
from lasr_amd import _lib                          # noqa: E402

pytestmark = pytest.mark.gpu
T = _lib.NN_TILE
Z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'side_reference_kernels.npz'))
N_CH = len({k.split('/')[1] for k in Z.files if k.startswith('chamfer/')})
FORWARD_SHAPES = [(1, 1, 1), (2, 63, 1), (1, 65, T - 1), (1, 64, T), (2, 257, T + 1), (1, 300, 2 * T + 3)]


def _clouds(N, P, Q, dev, seed=0):
    g = torch.Generator().manual_seed(seed + 1000 * P + Q)
    return torch.randn(N, P, 3, generator=g).to(dev), torch.randn(N, Q, 3, generator=g).to(dev)


@pytest.mark.parametrize('splits', [0, 1, 2, 7])
@pytest.mark.parametrize('N, P, Q', FORWARD_SHAPES)
def test_forward_equals_nearest_point_bit_for_bit(cuda, N, P, Q, splits):
    from lasr_amd.chamfer3D import dist_chamfer_3D as dc
    from lasr_amd.nnutils import fused_ops
    a, b = _clouds(N, P, Q, cuda)
    d1, d2, i1, i2 = dc.chamfer_3DFunction.apply(a, b, splits)
    r1, j1 = fused_ops.nearest_point(a, b)
    r2, j2 = fused_ops.nearest_point(b, a)
    assert i1.dtype == torch.int32 and i2.dtype == torch.int32 and d1.shape == (N, P) and d2.shape == (N, Q)
    assert torch.equal(d1, r1) and torch.equal(i1.long(), j1)
    assert torch.equal(d2, r2) and torch.equal(i2.long(), j2)
    e1, k1 = dc.nn_tiled(a, b, splits=splits)                       # the one-directional entry point
    assert torch.equal(e1, r1) and torch.equal(k1.long(), j1)


def test_module_call_shape_is_the_reference_s(cuda):
    from lasr_amd.chamfer3D import dist_chamfer_3D
    a, b = _clouds(2, 70, 90, cuda)
    out = dist_chamfer_3D.chamfer_3DDist()(a, b)
    assert len(out) == 4 and [tuple(o.shape) for o in out] == [(2, 70), (2, 90), (2, 70), (2, 90)]
    assert out[2].dtype == torch.int32 and int(out[2].max()) < 90 and int(out[3].max()) < 70


def test_ties_across_splits_take_the_lowest_index(cuda):
    from lasr_amd.chamfer3D import dist_chamfer_3D as dc
    from lasr_amd.nnutils import fused_ops
    a, b = _clouds(1, 300, T, cuda, seed=5)
    b = torch.cat([b, b], 1).contiguous()                           # b[k + T] = b[k]: every minimum occurs in both splits
    d, i = dc.nn_tiled(a, b, splits=2)
    assert int(i.max()) < T
    r, j = fused_ops.nearest_point(a, b)
    assert torch.equal(d, r) and torch.equal(i.long(), j)


def test_transform_is_applied_to_the_query(cuda):
    """a R + T formed in the kernel in fp32 without contraction: the same bits as the three products and sums written out."""
    from lasr_amd.chamfer3D import dist_chamfer_3D as dc
    from lasr_amd.nnutils import fused_ops
    a, b = _clouds(2, 130, T + 5, cuda, seed=7)
    R = torch.stack([torch.from_numpy(ir.rotation((1, 2, 3), 0.4, np.float32)), torch.from_numpy(ir.rotation((0, 1, 0), -1.0, np.float32))]).to(cuda)
    Tr = torch.tensor([[0.1, -0.2, 0.3], [1., 0., -1.]], device=cuda)
    at = torch.stack([((a[..., 0] * R[:, None, 0, k] + a[..., 1] * R[:, None, 1, k]) + a[..., 2] * R[:, None, 2, k]) + Tr[:, None, k]
                      for k in range(3)], -1)
    for splits in (1, 3):
        d, i = dc.nn_tiled(a, b, R, Tr, splits=splits)
        r, j = fused_ops.nearest_point(at, b)
        assert torch.equal(i.long(), j) and torch.equal(d, r)


def test_nan_rows_report_index_zero(cuda):
    from lasr_amd.chamfer3D import dist_chamfer_3D as dc
    from lasr_amd.nnutils import fused_ops
    a, b = _clouds(1, 10, 2 * T, cuda)
    a[0, 3, 1] = float('nan')
    for splits in (1, 2):
        d, i = dc.nn_tiled(a, b, splits=splits)
        r, j = fused_ops.nearest_point(a, b)
        assert int(i[0, 3]) == 0 and torch.equal(i.long(), j) and torch.equal(d, r)


@pytest.mark.parametrize('k', range(N_CH))
def test_forward_equals_the_reference_s_chamfer3d_vectors(cuda, k):
    from lasr_amd.chamfer3D import dist_chamfer_3D
    g = lambda n: Z['chamfer/%d/%s' % (k, n)]                             # noqa: E731
    a, b = torch.from_numpy(g('xyz1')).to(cuda), torch.from_numpy(g('xyz2')).to(cuda)
    d1, d2, i1, i2 = dist_chamfer_3D.chamfer_3DDist()(a, b)
    assert np.array_equal(i1.cpu().numpy(), g('idx1')) and np.array_equal(i2.cpu().numpy(), g('idx2'))
    assert np.abs(d1.cpu().numpy() - g('dist1')).max() <= 2e-6 and np.abs(d2.cpu().numpy() - g('dist2')).max() <= 2e-6


def _backward_case(name, dev):
    if name == 'collision':                                         # 500 xyz2 points that all choose xyz1[0]
        g = torch.Generator().manual_seed(11)
        x1 = torch.randn(1, 40, 3, generator=g) * 3
        x2 = x1[:, :1] + 0.01 * torch.randn(1, 500, 3, generator=g)
        return x1.to(dev), x2.to(dev)
    N, P, Q = name
    return _clouds(N, P, Q, dev, seed=3)


@pytest.mark.parametrize('case', [(2, 100, 37), (1, 65, 2 * T + 3), 'collision'], ids=str)
def test_backward_against_float64_autograd(cuda, case):
    """Bound: 1e-5 of the largest entry (the project's bound for gradients against fp64)."""
    from lasr_amd.chamfer3D import dist_chamfer_3D
    x1, x2 = _backward_case(case, cuda)
    g = torch.Generator().manual_seed(21)
    g1, g2 = torch.randn(x1.shape[:2], generator=g).to(cuda), torch.randn(x2.shape[:2], generator=g).to(cuda)
    grads = []
    for _ in range(2):
        a, b = x1.clone().requires_grad_(True), x2.clone().requires_grad_(True)
        d1, d2, i1, i2 = dist_chamfer_3D.chamfer_3DDist()(a, b)
        assert not i1.requires_grad and not i2.requires_grad and d1.requires_grad and d2.requires_grad
        ((g1 * d1).sum() + (g2 * d2).sum()).backward()
        grads.append((a.grad, b.grad))
    if case == 'collision':
        assert int(i2.max()) == 0
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])
    w1, w2 = ir.chamfer_backward(x1, x2, i1, i2, g1, g2)
    for got, want in ((grads[0][0], w1), (grads[0][1], w2)):
        err = float((got.double().cpu() - want).abs().max())
        scale = float(want.abs().max())
        print('%s: max |grad - fp64| = %.3g of max |grad| = %.3g' % (case, err, scale))
        assert err <= 1e-5 * scale


def test_one_sided_gradient(cuda):
    """Only dist1 used: the gradient of dist2 arrives as None / zeros and the result is the dist1 term alone."""
    from lasr_amd.chamfer3D import dist_chamfer_3D
    x1, x2 = _clouds(1, 50, 60, cuda, seed=9)
    a, b = x1.clone().requires_grad_(True), x2.clone().requires_grad_(True)
    d1, _, i1, i2 = dist_chamfer_3D.chamfer_3DDist()(a, b)
    d1.sum().backward()
    w1, w2 = ir.chamfer_backward(x1, x2, i1, i2, torch.ones(1, 50), torch.zeros(1, 60))
    assert float((a.grad.double().cpu() - w1).abs().max()) <= 1e-5 * float(w1.abs().max())
    assert float((b.grad.double().cpu() - w2).abs().max()) <= 1e-5 * float(w2.abs().max())
