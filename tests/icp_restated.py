"""Restatements the ICP and chamfer3D tests compare against (not collected): the iteration of pytorch3d.ops.iterative_closest_point
as DESIGN section 4.9 states it, in numpy at a chosen precision, and the chamfer3D backward as float64 autograd with the indices
fixed.  Written from those definitions; nothing here calls the code under test."""
import numpy as np
import torch


def rotation(axis, angle, dtype=np.float64):
    """Rodrigues: the matrix M with (M v) = v turned by `angle` about `axis` (column-vector convention)."""
    k = np.asarray(axis, np.float64)
    k = k / np.linalg.norm(k)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return (np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)).astype(dtype)


def recovery_case():
    """(X, Y, R0, t0), float64: X R0 + t0 is a permutation of Y, R0 a 0.05 rad turn about (1, 2, 3)."""
    rng = np.random.default_rng(0)
    Y = rng.random((300, 3))
    perm = rng.permutation(300)
    R0 = rotation((1, 2, 3), 0.05)
    t0 = np.array([0.01, -0.005, 0.003])
    X = (Y[perm] - t0) @ R0.T
    return X, Y, R0, t0


def _ellipsoid(rng, n):
    u = rng.standard_normal((n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    return u * np.array([1.0, 0.6, 0.4]), u


def ellipsoid_case():
    """(X [500,3], Y [703,3]), float64: samples of one ellipsoid, X turned 0.3 rad about (0, 1, 1) and shifted, Y with an 8 %
    sinusoidal bump; no point of X has an exact partner in Y."""
    rng = np.random.default_rng(1)
    x, _ = _ellipsoid(rng, 500)
    X = x @ rotation((0, 1, 1), 0.3).T + np.array([0.1, 0.05, -0.08])
    y, u = _ellipsoid(rng, 703)
    Y = y * (1 + 0.08 * np.sin(5 * u[:, :1]) * np.cos(4 * u[:, 1:2]))
    return X, Y


def pad_to(x, n):
    """Repeat the points of x [P,3] cyclically up to n points."""
    return x[np.arange(n) % x.shape[0]]


def nearest(a, b):
    """Index of the nearest b point of every a point, lowest index on ties (in the arrays' precision)."""
    d = ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)
    return d.argmin(1)


def kabsch(x, y):
    """R, T minimising sum |x R + T - y|^2 over rotations: centred covariance x^T y / P, SVD, R = U diag(1, 1, det(U V^T)) V^T."""
    mx, my = x.mean(0), y.mean(0)
    cov = (x - mx).T @ (y - my) / x.shape[0]
    U, _, Vt = np.linalg.svd(cov)
    E = np.eye(3, dtype=x.dtype)
    E[2, 2] = np.linalg.det(U @ Vt)
    R = U @ E @ Vt
    return R, my - mx @ R


def icp(X, Y, max_iterations, thr, dtype=np.float64):
    """X [N,P,3], Y [N,Q,3] -> R [N,3,3], T [N,3], rmse [N], iterations, converged; stops after the iteration in which
    (previous rmse - rmse) / previous rmse <= thr for every batch element (1 on the first iteration)."""
    X, Y = np.asarray(X, dtype), np.asarray(Y, dtype)
    N = X.shape[0]
    R = np.stack([np.eye(3, dtype=dtype)] * N)
    T = np.zeros((N, 3), dtype)
    rmse = np.zeros(N, dtype)
    prev = None
    converged, it = False, 0
    for it in range(1, max_iterations + 1):
        for n in range(N):
            tgt = Y[n][nearest(X[n] @ R[n] + T[n], Y[n])]
            R[n], T[n] = kabsch(X[n], tgt)
            rmse[n] = np.sqrt((((X[n] @ R[n] + T[n]) - tgt) ** 2).sum(1).mean())
        with np.errstate(divide='ignore', invalid='ignore'):
            relative = np.ones(N, dtype) if prev is None else (prev - rmse) / prev
        prev = rmse.copy()
        if (relative <= thr).all():
            converged = True
            break
    return R, T, rmse, it, converged


def chamfer_backward(x1, x2, idx1, idx2, g1, g2):
    """d/dx1, d/dx2 of sum g1 |x1 - x2[idx1]|^2 + sum g2 |x2 - x1[idx2]|^2 with the indices fixed: float64 autograd on the CPU.
    x1 [N,P,3], x2 [N,Q,3], idx1 [N,P], idx2 [N,Q], g1 [N,P], g2 [N,Q] (any device / dtype) -> two float64 CPU tensors."""
    a = x1.detach().double().cpu().requires_grad_(True)
    b = x2.detach().double().cpu().requires_grad_(True)
    i1 = idx1.cpu().long()[..., None].expand(-1, -1, 3)
    i2 = idx2.cpu().long()[..., None].expand(-1, -1, 3)
    d1 = ((a - torch.gather(b, 1, i1)) ** 2).sum(-1)
    d2 = ((b - torch.gather(a, 1, i2)) ** 2).sum(-1)
    ((g1.double().cpu() * d1).sum() + (g2.double().cpu() * d2).sum()).backward()
    return a.grad, b.grad
