"""lasr_amd.nnutils.icp on the GPU against the float64 restatement of tests/icp_restated.py.

Tolerance of the comparisons with the restatement: 16 x the gap between its float32 and its float64 run on the same input, but no
less than 1e-6; the test computes the gap from the two restatements.  On the CPU the gap on the ellipsoid pair is 9.1e-8 (R),
3.9e-8 (T), 5.8e-9 (rmse).  The device-against-float64 figures each test prints have NOT been recorded yet: no MI355X run of this
file exists so far (DESIGN section 4.9 says the same); a host emulation of the device's arithmetic (tests/test_icp_cpu.py) lands at
2.6e-8, 5.4e-9, 6.4e-10."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_restated as ir                          # noqa: E402

pytestmark = pytest.mark.gpu
_cache = {}


def restated(name, X, Y, max_iterations, thr, dtype):
    """One run of the restatement per (case, precision), shared by the tests."""
    key = (name, max_iterations, thr, np.dtype(dtype).name)
    if key not in _cache:
        _cache[key] = ir.icp(X, Y, max_iterations, thr, dtype)
    return _cache[key]


def tolerances(name, X, Y, max_iterations, thr):
    R64, T64, e64, _, _ = restated(name, X, Y, max_iterations, thr, np.float64)
    R32, T32, e32, _, _ = restated(name, X, Y, max_iterations, thr, np.float32)
    gaps = [float(np.abs(a.astype(np.float64) - b).max()) for a, b in ((R32, R64), (T32, T64), (e32, e64))]
    return gaps, [max(16 * g, 1e-6) for g in gaps]


def on_gpu(X, Y, dev):
    return torch.from_numpy(np.asarray(X, np.float32)).to(dev), torch.from_numpy(np.asarray(Y, np.float32)).to(dev)


def test_recovers_a_known_transform(cuda):
    from lasr_amd.nnutils.icp import iterative_closest_point
    X, Y, R0, t0 = ir.recovery_case()
    x, y = on_gpu(X[None], Y[None], cuda)
    sol = iterative_closest_point(x, y, max_iterations=100)
    eR = float(np.abs(sol.RTs.R[0].double().cpu().numpy() - R0).max())
    eT = float(np.abs(sol.RTs.T[0].double().cpu().numpy() - t0).max())
    print('recovery: %d iterations, |R - R0| = %.3g, |T - t0| = %.3g, rmse = %.3g' % (sol.iterations, eR, eT, float(sol.rmse[0])))
    assert sol.converged is True and sol.iterations <= 10
    assert eR <= 1e-5 and eT <= 1e-5
    assert torch.equal(sol.RTs.s, torch.ones(1, device=cuda))
    assert float((sol.Xt[0] - (x[0] @ sol.RTs.R[0] + sol.RTs.T[0])).abs().max()) <= 1e-6


def test_thirty_iterations_on_clouds_that_do_not_match(cuda):
    """Prints the float32 - float64 gap of the restatement and the device - float64 error; not yet recorded from an MI355X."""
    from lasr_amd.nnutils.icp import iterative_closest_point
    X, Y = ir.ellipsoid_case()
    gaps, tol = tolerances('ellipsoid', X[None], Y[None], 30, -1.)
    R64, T64, e64, it64, conv64 = restated('ellipsoid', X[None], Y[None], 30, -1., np.float64)
    assert it64 == 30 and not conv64
    x, y = on_gpu(X[None], Y[None], cuda)
    sol = iterative_closest_point(x, y, max_iterations=30, relative_rmse_thr=-1.)
    assert sol.iterations == 30 and sol.converged is False
    err = [float(np.abs(sol.RTs.R.double().cpu().numpy() - R64).max()), float(np.abs(sol.RTs.T.double().cpu().numpy() - T64).max()),
           float(np.abs(sol.rmse.double().cpu().numpy() - e64).max())]
    print('ellipsoid, 30 iterations: fp32-fp64 gap R %.3g T %.3g rmse %.3g; device-fp64 R %.3g T %.3g rmse %.3g' % tuple(gaps + err))
    assert err[0] <= tol[0] and err[1] <= tol[1] and err[2] <= tol[2]


def test_stop_flag_and_chunking(cuda):
    from lasr_amd.nnutils.icp import iterative_closest_point
    X, Y = ir.ellipsoid_case()
    x, y = on_gpu(X[None], Y[None], cuda)
    runs = [iterative_closest_point(x, y, max_iterations=10000, relative_rmse_thr=1e-6, chunk=c) for c in (1, 64, 64)]
    _, _, _, it64, conv64 = restated('ellipsoid', X[None], Y[None], 10000, 1e-6, np.float64)
    print('ellipsoid to convergence: %d iterations on the device, %d in the float64 restatement' % (runs[0].iterations, it64))
    assert conv64
    for s in runs:
        assert s.converged is True and s.iterations < 10000
    assert runs[0].iterations == it64            # same stop test on both sides: another count would be another trajectory
    for s in runs[1:]:
        assert s.iterations == runs[0].iterations
        assert torch.equal(s.RTs.R, runs[0].RTs.R) and torch.equal(s.RTs.T, runs[0].RTs.T) and torch.equal(s.rmse, runs[0].rmse)
    forced = iterative_closest_point(x, y, max_iterations=10000, relative_rmse_thr=1e-6, splits=1)   # the split count changes no bit
    assert forced.iterations == runs[0].iterations and torch.equal(forced.RTs.R, runs[0].RTs.R) and torch.equal(forced.rmse, runs[0].rmse)


def test_batch_stops_when_every_element_has_converged(cuda):
    from lasr_amd.nnutils.icp import iterative_closest_point
    X, Y, _, _ = ir.recovery_case()
    A, B = ir.ellipsoid_case()
    Xb, Yb = np.stack([ir.pad_to(X, 500), A]), np.stack([ir.pad_to(Y, 703), B])
    R64, T64, e64, it64, conv64 = restated('batch', Xb, Yb, 10000, 1e-6, np.float64)
    assert conv64
    # the tolerance from a fixed iteration count on both precisions: the float32 restatement may stop at another iteration
    gaps, tol = tolerances('batch_fixed', Xb, Yb, it64, -1.)
    x, y = on_gpu(Xb, Yb, cuda)
    sol = iterative_closest_point(x, y, max_iterations=10000, relative_rmse_thr=1e-6)
    err = [float(np.abs(sol.RTs.R.double().cpu().numpy() - R64).max()), float(np.abs(sol.RTs.T.double().cpu().numpy() - T64).max()),
           float(np.abs(sol.rmse.double().cpu().numpy() - e64).max())]
    print('batch: %d iterations (restatement %d); fp32-fp64 gap R %.3g T %.3g rmse %.3g; device-fp64 R %.3g T %.3g rmse %.3g'
          % tuple([sol.iterations, it64] + gaps + err))
    assert sol.converged is True and sol.iterations == it64
    assert err[0] <= tol[0] and err[1] <= tol[1] and err[2] <= tol[2]


def test_through_the_evaluation(cuda):
    """A rotated copy of a mesh aligned onto the original: both alignments sit at the sampling floor."""
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    import eval_mesh
    from lasr_amd import synth
    v, f = synth.geodesic_sphere(6)
    gv = torch.from_numpy(v * np.array([1., 0.7, 0.5], np.float32)).to(cuda)
    f = torch.from_numpy(f).to(cuda)
    pv = gv @ torch.from_numpy(ir.rotation((1, 1, 0), 0.1, np.float32)).to(cuda)
    info = {}
    ref = eval_mesh.evaluate_pair((pv, f), (gv, f), n=2000, icp='reference', aligned=info)
    fast = eval_mesh.evaluate_pair((pv, f), (gv, f), n=2000, icp='fast')
    same = eval_mesh.evaluate_pair((gv, f), (gv, f), n=2000, icp='fast')
    print('Chamfer distance, n = 2000: reference %.5f (%d iterations, converged %s), fast %.5f, unrotated %.5f'
          % (ref, info['icp_iterations'], info['icp_converged'], fast, same))
    assert np.isfinite(ref) and ref <= 1.1 * fast
