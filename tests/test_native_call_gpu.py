"""_lib.call on the device: the stream is read at call time (an operator run inside torch.cuda.stream(...) lands on that stream and
gives the bits of the default-stream run), tensor views stand in for hand-computed pointers, None goes over as NULL."""
import numpy as np
import pytest
import torch

from lasr_amd import _lib
from lasr_amd.nnutils import fused_ops, image_losses

pytestmark = pytest.mark.gpu


def _rand(cuda, seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(cuda)


def _quat(cuda):
    q = _rand(cuda, 1, 5, 4).requires_grad_()
    R = fused_ops.quat_to_rotmat(q)
    g, = torch.autograd.grad(R, q, _rand(cuda, 2, 5, 3, 3))
    return R.detach(), g


def _mask_loss(cuda):
    pred = _rand(cuda, 3, 2, 2, 16, 16).requires_grad_()
    masks = (_rand(cuda, 4, 2, 16, 16) > 0).float()
    occ = (_rand(cuda, 5, 2, 16, 16) > -1).float()
    tab = image_losses.mask_loss_table(pred, masks, occ)
    g, = torch.autograd.grad(tab, pred, _rand(cuda, 6, 2, 2))
    return tab.detach(), g


def _fill(cuda):
    return fused_ops.fill_planes(_rand(cuda, 7, 2, 4, 8, 8), [0.25, -1., 3., 0.]),


def _chamfer(cuda):
    a, b = _rand(cuda, 8, 2, 5, 3).requires_grad_(), _rand(cuda, 9, 2, 7, 3).requires_grad_()
    d = fused_ops.chamfer(a, b)                                   # the b -> a indices sit behind the view nn[N * P:]
    ga, gb = torch.autograd.grad(d, [a, b], _rand(cuda, 10, 2))
    return d.detach(), ga, gb


@pytest.mark.parametrize('op', [_quat, _mask_loss, _fill, _chamfer])
def test_side_stream_run_equals_default_stream_run(cuda, op):
    ref = op(cuda)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        out = op(cuda)
    side.synchronize()
    assert len(out) == len(ref) and all(torch.equal(o, r) for o, r in zip(out, ref))


def test_chamfer_through_the_view_matches_torch(cuda):
    a, b = _rand(cuda, 8, 2, 5, 3), _rand(cuda, 9, 2, 7, 3)
    d2 = ((a[:, :, None] - b[:, None]) ** 2).sum(-1)
    ref = d2.min(2)[0].mean(1) + d2.min(1)[0].mean(1)
    np.testing.assert_allclose(fused_ops.chamfer(a, b).cpu().numpy(), ref.cpu().numpy(), rtol=1e-5, atol=1e-6)


def test_none_goes_over_as_null(cuda):
    # mean_shape without symmetry (flip = mask = None): tests/test_ops_gpu.py's restatement at H = 2, Vp = 6
    H, Vp, R = 2, 6, 3
    mv, tx = _rand(cuda, 11, H, Vp, 3), _rand(cuda, 12, H, Vp, 3)
    ov, ot = fused_ops.mean_shape(mv, tx, None, None, R, 0)
    assert torch.equal(ov, mv[None].repeat(R, 1, 1, 1).view(R * H, Vp, 3))
    rt = tx.cpu().sigmoid()[None].repeat(R, 1, 1, 1).view(R * H, Vp, 3)
    np.testing.assert_allclose(ot.cpu().numpy(), rt.numpy(), rtol=2e-6, atol=1e-7)


def test_tensor_of_another_gpu_is_refused_before_the_launch(cuda, monkeypatch):
    if torch.cuda.device_count() < 2:
        pytest.skip('needs two devices')
    entered, real = [], _lib.lib()

    class Handle:
        def __getattr__(self, name):
            fn = getattr(real, name)

            def rec(*args):
                entered.append(name)
                return fn(*args)
            rec.argtypes = fn.argtypes
            return rec
    monkeypatch.setattr(_lib, '_lib', Handle())
    q, R = torch.zeros(1, 4, device=cuda), torch.zeros(1, 9, device='cuda:1')
    with pytest.raises(ValueError) as e:
        _lib.call('lasr_quat_to_rotmat_forward', q, R, 1)
    assert 'lasr_quat_to_rotmat_forward' in str(e.value) and entered == []
