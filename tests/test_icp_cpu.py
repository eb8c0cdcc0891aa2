"""ICP and chamfer3D without a GPU: known answers of the restatement the GPU tests compare against (tests/icp_restated.py), the
3x3 alignment the device runs against a LAPACK SVD (lasr_icp_kabsch_host is the same code built for the host), the host-side
argument checks of the new entry points and the --icp option of scripts/eval_mesh.py."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_restated as ir                          # noqa: E402


@pytest.mark.parametrize('dtype, bound', [(np.float64, 1e-12), (np.float32, 1e-5)])
def test_restatement_recovers_a_known_transform(dtype, bound):
    """Recorded here: 3 iterations at both precisions; |R - R0|, |T - t0| 5e-16 in float64, 3.4e-7 in float32."""
    X, Y, R0, t0 = ir.recovery_case()
    R, T, rmse, it, converged = ir.icp(X[None], Y[None], 10, 1e-6, dtype)
    eR, eT = np.abs(R[0] - R0).max(), np.abs(T[0] - t0).max()
    print('%s: %d iterations, |R - R0| = %.3g, |T - t0| = %.3g, rmse = %.3g' % (np.dtype(dtype).name, it, eR, eT, rmse[0]))
    assert converged and it <= 10
    assert eR <= bound and eT <= bound


def test_restatement_batch_stops_when_every_element_has():
    X, Y, _, _ = ir.recovery_case()
    A, B = ir.ellipsoid_case()
    Xb = np.stack([ir.pad_to(X, 500), A])
    Yb = np.stack([ir.pad_to(Y, 703), B])
    _, _, _, it_b, conv_b = ir.icp(Xb, Yb, 200, 1e-6)
    _, _, _, it_0, _ = ir.icp(Xb[:1], Yb[:1], 200, 1e-6)
    _, _, _, it_1, _ = ir.icp(Xb[1:], Yb[1:], 200, 1e-6)
    assert conv_b and it_b >= max(it_0, it_1) and it_0 < it_1


def _moments(x, y):
    return np.concatenate([x.sum(0), y.sum(0), (x[:, :, None] * y[:, None, :]).sum(0).ravel()]).astype(np.float64)


def _kabsch_host(x, y):
    from lasr_amd import _lib
    m = np.ascontiguousarray(_moments(x, y))
    R, T = np.zeros(9, np.float32), np.zeros(3, np.float32)
    rc = _lib.lib().lasr_icp_kabsch_host(m.ctypes.data, x.shape[0], R.ctypes.data, T.ctypes.data)
    assert rc == 0
    return R.reshape(3, 3), T


@pytest.mark.parametrize('case', ['generic', 'reflection', 'planar', 'identity', 'offset'])
def test_device_alignment_code_equals_a_lapack_svd(case):
    """The Jacobi SVD + Kabsch of csrc/chamfer.hip, built for the host, against numpy's: both exact to double rounding, the result
    rounded to fp32, so 2e-6 (a few fp32 ulps of entries <= 1 and translations of a few units)."""
    rng = np.random.default_rng(3)
    x = rng.standard_normal((200, 3))
    if case == 'generic':
        y = x @ ir.rotation((1, -2, 0.5), 1.1).T + rng.standard_normal((200, 3)) * 0.1 + [0.3, -2., 1.]
    elif case == 'reflection':                                     # the best orthogonal map is a reflection: det correction acts
        y = x * [1, 1, -1] + rng.standard_normal((200, 3)) * 0.05
    elif case == 'planar':                                          # smallest singular value exactly 0
        x[:, 2] = 0
        y = x @ ir.rotation((0, 0, 1), 0.4).T
    elif case == 'identity':
        y = x.copy()
    else:                                                           # far from the origin: the centring must not cancel
        x = x + 50.
        y = x @ ir.rotation((3, 1, 2), 0.2).T + [1., 2., 3.]
    R, T = _kabsch_host(x, y)
    Rn, Tn = ir.kabsch(x, y)
    assert abs(np.linalg.det(R.astype(np.float64)) - 1) <= 1e-5
    tol = 2e-6 * max(1., np.abs(Tn).max())
    assert np.abs(R - Rn).max() <= 2e-6 and np.abs(T - Tn).max() <= tol, (np.abs(R - Rn).max(), np.abs(T - Tn).max())


def _emulated_device_icp(X, Y, iters, thr):
    """The device loop's arithmetic on the host: fp32 transform (products and sums in the kernel's order) and fp32 search, the
    fifteen sums in double, lasr_icp_kabsch_host (the device's alignment code), the RMSE in double from the fp32 R, T."""
    X, Y = X.astype(np.float32), Y.astype(np.float32)
    R, T, prev = np.eye(3, dtype=np.float32), np.zeros(3, np.float32), None
    for it in range(1, iters + 1):
        xt = ((X[:, 0:1] * R[0] + X[:, 1:2] * R[1]) + X[:, 2:3] * R[2]) + T
        tgt = Y[ir.nearest(xt, Y)].astype(np.float64)
        R, T = _kabsch_host(X.astype(np.float64), tgt)
        rmse = np.sqrt((((X.astype(np.float64) @ R.astype(np.float64) + T.astype(np.float64)) - tgt) ** 2).sum(1).mean())
        relative = 1. if prev is None else (prev - rmse) / prev
        prev = rmse
        if relative <= thr:
            return R, T, rmse, it, True
    return R, T, rmse, it, False


def test_emulated_device_arithmetic_stays_inside_the_gpu_test_s_tolerance():
    """What tests/test_icp_gpu.py asks of the device, asked here of a host emulation of its arithmetic, so that the tolerance rule
    (16 x the float32 - float64 gap of the restatement, at least 1e-6) is known to be reachable before a GPU is involved.
    Recorded here on tests/icp_restated.py's ellipsoid pair, 30 iterations: restatement gap 9.1e-8 (R), 3.9e-8 (T), 5.8e-9 (rmse);
    emulation against float64 2.6e-8, 5.4e-9, 6.4e-10; both stop at iteration 27 with relative_rmse_thr = 1e-6."""
    X, Y = ir.ellipsoid_case()
    R64, T64, e64, _, _ = ir.icp(X[None], Y[None], 30, -1.)
    R32, T32, e32, _, _ = ir.icp(X[None], Y[None], 30, -1., np.float32)
    R, T, e, it, conv = _emulated_device_icp(X, Y, 30, -1.)
    gaps = [np.abs(R32 - R64).max(), np.abs(T32 - T64).max(), np.abs(e32 - e64).max()]
    errs = [np.abs(R - R64[0]).max(), np.abs(T - T64[0]).max(), abs(e - e64[0])]
    print('gap %.3g %.3g %.3g; emulation %.3g %.3g %.3g' % tuple(gaps + errs))
    assert it == 30 and not conv
    for g, err in zip(gaps, errs):
        assert err <= max(16 * g, 1e-6)
    assert _emulated_device_icp(X, Y, 10000, 1e-6)[3:] == (ir.icp(X[None], Y[None], 10000, 1e-6)[3], True)


def test_new_entry_points_check_their_arguments_on_the_host():
    """Bad sizes and null pointers are refused before anything touches a device (the pointers below are never dereferenced)."""
    from lasr_amd import _lib
    h = _lib.lib()
    p, n = 1 << 20, None
    big = (1 << 27) + 1
    assert h.lasr_chamfer3d_workspace_bytes(2, 100, 50) >= 8 * 2 * 150
    assert h.lasr_chamfer3d_workspace_bytes(-1, 5, 5) == 0 and h.lasr_chamfer3d_workspace_bytes(1, big, 5) == 0
    ok = [p, p, n, n, p, p, p, 1 << 20, 1, 5, 7, 0, n]                         # lasr_nn_tiled
    for k, v in ((8, -1), (8, 65536), (9, -1), (9, big), (10, 0), (10, big), (11, -1), (11, 65536), (0, n), (1, n), (4, n), (5, n),
                 (2, p), (3, p)):
        bad = list(ok)
        bad[k] = v
        assert h.lasr_nn_tiled(*bad) == -1, (k, v)
    assert h.lasr_nn_tiled(p, p, n, n, p, p, n, 0, 1, 5, 7, 2, n) == -1         # two splits need a workspace
    assert h.lasr_nn_tiled(p, p, n, n, p, p, p, 8, 1, 5, 7, 2, n) == -3         # ... of 8 N P bytes
    assert h.lasr_nn_tiled(n, n, n, n, n, n, n, 0, 0, 5, 7, 0, n) == 0 and h.lasr_nn_tiled(n, n, n, n, n, n, n, 0, 3, 0, 7, 0, n) == 0
    ok = [p, p, p, p, p, p, p, 1 << 20, 1, 5, 7, 0, n]                         # lasr_chamfer3d_forward
    for k, v in ((8, -1), (9, 0), (10, 0), (9, big), (11, -1), (0, n), (1, n), (2, n), (3, n), (4, n), (5, n), (6, n)):
        bad = list(ok)
        bad[k] = v
        assert h.lasr_chamfer3d_forward(*bad) == -1, (k, v)
    bad = list(ok)
    bad[7] = 8
    assert h.lasr_chamfer3d_forward(*bad) == -3
    assert h.lasr_chamfer3d_forward(n, n, n, n, n, n, n, 0, 0, 5, 7, 0, n) == 0
    ok = [p] * 12 + [1, 5, 7, n]                                                # lasr_chamfer3d_backward
    for k, v in [(12, -1), (13, 0), (14, 0), (14, big)] + [(k, n) for k in range(12)]:
        bad = list(ok)
        bad[k] = v
        assert h.lasr_chamfer3d_backward(*bad) == -1, (k, v)
    assert h.lasr_chamfer3d_backward(*([n] * 12), 0, 5, 7, n) == 0
    need = h.lasr_icp_workspace_bytes(2, 300, 200)
    assert need >= 2 * 300 * 12 + 2 * 2 * 15 * 8
    assert h.lasr_icp_workspace_bytes(0, 5, 5) == 0 and h.lasr_icp_workspace_bytes(_lib.ICP_MAX_BATCH + 1, 5, 5) == 0
    assert h.lasr_icp_workspace_bytes(1, 0, 5) == 0 and h.lasr_icp_workspace_bytes(1, 5, 0) == 0
    ok = [p, p, p, p, p, need, 2, 300, 200, n]                                  # lasr_icp_init
    for k, v in [(6, 0), (6, 65), (7, 0), (8, 0), (8, big)] + [(k, n) for k in range(5)]:
        bad = list(ok)
        bad[k] = v
        assert h.lasr_icp_init(*bad) == -1, (k, v)
    bad = list(ok)
    bad[5] = need - 1
    assert h.lasr_icp_init(*bad) == -3
    ok = [p, p, p, p, p, p, p, need, 2, 300, 200, 4, 1e-6, 0, n]                # lasr_icp_iterate
    for k, v in [(8, 0), (9, 0), (10, 0), (11, -1), (11, _lib.ICP_MAX_CHUNK + 1), (13, -1), (13, 65536)] + [(k, n) for k in range(7)]:
        bad = list(ok)
        bad[k] = v
        assert h.lasr_icp_iterate(*bad) == -1, (k, v)
    bad = list(ok)
    bad[7] = need - 1
    assert h.lasr_icp_iterate(*bad) == -3
    assert h.lasr_icp_kabsch_host(n, 5, p, p) == -1 and h.lasr_icp_kabsch_host(p, 0, p, p) == -1


def test_python_layer_refuses_what_it_does_not_do():
    import torch
    from lasr_amd.chamfer3D import dist_chamfer_3D
    from lasr_amd.nnutils.icp import iterative_closest_point
    x, y = torch.zeros(1, 5, 3), torch.zeros(1, 7, 3)
    with pytest.raises(TypeError):
        dist_chamfer_3D.chamfer_3DDist()(x, y)
    with pytest.raises(TypeError):
        dist_chamfer_3D.nn_tiled(x, y)
    with pytest.raises(TypeError):
        iterative_closest_point(x, y)
    with pytest.raises(ValueError):
        iterative_closest_point(x, y, estimate_scale=True)
    with pytest.raises(ValueError):
        iterative_closest_point(x, y, allow_reflection=True)
    with pytest.raises(ValueError):
        iterative_closest_point([torch.zeros(5, 3), torch.zeros(6, 3)], [torch.zeros(7, 3), torch.zeros(7, 3)])
    with pytest.raises(ValueError):
        iterative_closest_point(x, torch.zeros(2, 7, 3))


def test_tile_size_of_the_header_is_the_python_mirror_s():
    from lasr_amd import _lib
    from lasr_amd.chamfer3D import dist_chamfer_3D
    ops = open(os.path.join(ROOT, 'include', 'lasr_ops.h')).read()
    for name, have in (('LASR_NN_TILE', _lib.NN_TILE), ('LASR_ICP_MAX_BATCH', _lib.ICP_MAX_BATCH), ('LASR_ICP_MAX_CHUNK', _lib.ICP_MAX_CHUNK)):
        assert int(re.search(r'#define\s+%s\s+(\d+)' % name, ops).group(1)) == have
    assert dist_chamfer_3D.NN_TILE == _lib.NN_TILE


def test_eval_mesh_icp_option():
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    import eval_mesh
    base = ['--testdir', 't', '--gtdir', 'g']
    assert eval_mesh.parse_args(base).icp == 'fast'
    assert eval_mesh.parse_args(base + ['--icp', 'reference']).icp == 'reference'
    assert eval_mesh.parse_args(base + ['--icp', 'fast']).icp == 'fast'
    with pytest.raises(SystemExit):
        eval_mesh.parse_args(base + ['--icp', 'pytorch3d'])
    with pytest.raises(ValueError):
        eval_mesh.evaluate_pair(None, None, icp='other')
