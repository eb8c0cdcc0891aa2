"""Rigid ICP with its state on the device (include/lasr_ops.h: lasr_icp_*, lasr_amd/csrc/chamfer.hip).

    sol = iterative_closest_point(X, Y, max_iterations=10000)       # the reference's call, /root/reference/scripts/eval_mesh.py:156
    sol.converged, sol.rmse, sol.Xt, sol.RTs.R, sol.RTs.T, sol.RTs.s, sol.iterations

restates pytorch3d.ops.iterative_closest_point for estimate_scale=False (pytorch3d is not installed here: parity unpinned).  The
iterations are enqueued `chunk` at a time with no synchronisation inside a chunk; after each chunk the host reads the 4-byte stop
flag.  A chunk that converges early costs only kernels that return at once, and the result does not depend on `chunk`."""
from collections import namedtuple

import torch

from .. import _lib

SimilarityTransform = namedtuple('SimilarityTransform', ['R', 'T', 's'])
ICPSolution = namedtuple('ICPSolution', ['converged', 'rmse', 'Xt', 'RTs', 'iterations'])


def _cloud(x, name):
    if isinstance(x, (list, tuple)):
        if len({tuple(t.shape) for t in x}) > 1:
            raise ValueError('%s: clouds of different lengths are not supported (pad them to one length)' % name)
        x = torch.stack(list(x))
    if not torch.is_tensor(x):
        raise ValueError('%s: expected a [N,P,3] tensor' % name)
    if x.dim() != 3 or x.shape[2] != 3:
        raise ValueError('%s: expected a [N,P,3] tensor, got %s' % (name, tuple(x.shape)))
    return x


def iterative_closest_point(X, Y, max_iterations=100, relative_rmse_thr=1e-6, estimate_scale=False, allow_reflection=False, chunk=32,
                            splits=0):
    """X [N,P,3], Y [N,Q,3] on the GPU -> ICPSolution(converged, rmse [N], Xt = X R + T [N,P,3], RTs(R [N,3,3], T [N,3], s = 1 [N]),
    iterations).  Stops after the iteration in which the relative decrease of the RMSE is at most relative_rmse_thr for every batch
    element, or after max_iterations.  splits: passed to the nearest-neighbour search (0: chosen by the library)."""
    if estimate_scale:
        raise ValueError('estimate_scale=True is not supported (the reference calls with estimate_scale=False)')
    if allow_reflection:
        raise ValueError('allow_reflection=True is not supported')
    X, Y = _cloud(X, 'X'), _cloud(Y, 'Y')
    if X.shape[0] != Y.shape[0]:
        raise ValueError('X and Y need the same batch size, got %d and %d' % (X.shape[0], Y.shape[0]))
    _lib.need_cuda(X, Y)
    if max_iterations < 0 or chunk < 1:
        raise ValueError('max_iterations must be >= 0 and chunk >= 1')
    N, P, Q = X.shape[0], X.shape[1], Y.shape[1]
    if N < 1 or N > _lib.ICP_MAX_BATCH or P < 1 or Q < 1:
        raise ValueError('need 1 <= N <= %d clouds with at least one point each' % _lib.ICP_MAX_BATCH)
    dtype = X.dtype
    Xf, Yf = _lib.f32(X.detach(), Y.detach())
    dev = Xf.device
    h = _lib.lib()
    R = torch.empty(N, 3, 3, dtype=torch.float32, device=dev)
    T = torch.empty(N, 3, dtype=torch.float32, device=dev)
    rmse = torch.empty(N, 2, dtype=torch.float64, device=dev)
    status = torch.empty(2, dtype=torch.int32, device=dev)
    nbytes = h.lasr_icp_workspace_bytes(N, P, Q)
    if nbytes == 0:
        raise ValueError('clouds of %d and %d points are beyond what lasr_icp_iterate takes' % (P, Q))
    ws = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
    chunk = min(int(chunk), _lib.ICP_MAX_CHUNK)
    _lib.call('lasr_icp_init', R, T, rmse, status, ws, nbytes, N, P, Q)
    done, converged = 0, False
    while done < max_iterations and not converged:
        n = min(chunk, max_iterations - done)
        _lib.call('lasr_icp_iterate', Xf, Yf, R, T, rmse, status, ws, nbytes, N, P, Q, n, float(relative_rmse_thr), splits)
        done += n
        converged = bool(status[0].item())                      # the one host read of a chunk: 4 bytes
    iterations = int(status[1].item())
    Xt = torch.baddbmm(T[:, None], Xf, R)
    return ICPSolution(converged, rmse[:, 0].to(dtype), Xt.to(dtype), SimilarityTransform(R.to(dtype), T.to(dtype),
                                                                                          torch.ones(N, dtype=dtype, device=dev)), iterations)
