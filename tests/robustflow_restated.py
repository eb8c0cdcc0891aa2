"""Restatement of the variational optical flow with the gradient-constancy term (include/lasr_ops.h: lasr_rflow_*, DESIGN.md
section 4.16) in plain numpy, in the style of tests/varflow_restated.py, whose fixtures, pyramid, expand, gradient, warp_positions,
_lerp4, weights and sor it uses unchanged.  The kernels of lasr_amd/csrc/robustflow.hip and the passes of preprocess/robust_flow.py
are compared against this file, not the other way round.

Brox et al. 2004 add to brightness constancy I2(p + w) = I1(p) the constancy of the image gradient, grad I2(p + w) = grad I1(p),
which an additive change of the lighting leaves untouched and a multiplicative one scales; Bruhn & Weickert 2005 give each of the
two data terms its own robust penalty.  Per pyramid level and warp:
  1. derivative planes of both levels, per channel: Ix, Iy = gradient(I); Ixx, Ixy = gradient(Ix); _, Iyy = gradient(Iy) (the
     central difference with a replicated border applied twice: the border clamps twice);
  2. two motion tensors, both zero where p + uv leaves the frame: Jb, the tensor of varflow_restated.tensor, and Jg, the sum over
     the channels of the outer products of the rows (Ixx, Ixy, Ixt) and (Ixy, Iyy, Iyt), with Ixx = 0.5 (I2xx(p + uv) + I1xx) and
     likewise Ixy, Iyy, and Ixt = I2x(p + uv) - I1x, Iyt = I2y(p + uv) - I1y;
  3. psi_b = 0.5 / sqrt(max(r2(Jb, d), 0) + eps^2), psi_g likewise from Jg, psi_s as in varflow_restated.weights; the solver sees
     J = (beta psi_b) Jb + (gamma psi_g) Jg and psi = (1, psi_s), and varflow_restated.sor runs unchanged on them.
Every function takes the working precision `dt` and computes in it alone, in a fixed operation order.
"""
import functools

import numpy as np

import varflow_restated as vr
from varflow_restated import _lerp4, expand, gradient, pyramid, sor, warp_positions, weights as vf_weights

GAMMA, BETA = 5., 1.                                # the values the issue's prototype derived on the fixtures (not on footage)
PLANES = 6                                          # I, Ix, Iy, Ixx, Ixy, Iyy
RELIGHTINGS = ('gain', 'ramp', 'shadow')


def check_terms(gamma, beta):
    g, b = float(gamma), float(beta)
    assert np.isfinite(g) and np.isfinite(b) and g >= 0 and b >= 0 and (g > 0 or b > 0), (gamma, beta)
    return g, b


def derivs(I, dt=np.float64):
    """A level [H,W,3] in dt -> its derivative record [H,W,3,6] = (I, Ix, Iy, Ixx, Ixy, Iyy) per channel."""
    I = np.asarray(I).astype(dt)
    Ix, Iy = gradient(I, dt)
    Ixx, Ixy = gradient(Ix, dt)
    _, Iyy = gradient(Iy, dt)
    return np.stack([I, Ix, Iy, Ixx, Ixy, Iyy], -1).astype(dt)


def tensor(R1, R2, uv, dt=np.float64):
    """The records of I1 and I2 [H,W,3,6], uv [2,H,W] -> (Jb, Jg), each [6,H,W] = (J11, J12, J22, J13, J23, J33), valid folded in."""
    R1, R2, uv = np.asarray(R1).astype(dt), np.asarray(R2).astype(dt), np.asarray(uv).astype(dt)
    H, W = uv.shape[1:]
    X, Y, valid = warp_positions(uv, dt)
    Xc, Yc = np.clip(X, dt(0), dt(W - 1)), np.clip(Y, dt(0), dt(H - 1))
    fx, fy = np.floor(Xc), np.floor(Yc)
    x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    tx, ty = (Xc - fx).astype(dt), (Yc - fy).astype(dt)
    half = dt(0.5)

    def sample(c, q):
        f = R2[..., c, q]
        return _lerp4(f[y0, x0], f[y0, x1], f[y1, x0], f[y1, x1], tx, ty, dt)
    Jb, Jg = [None] * 6, [None] * 6
    for c in range(3):
        Ix = half * (sample(c, 1) + R1[..., c, 1])
        Iy = half * (sample(c, 2) + R1[..., c, 2])
        It = sample(c, 0) - R1[..., c, 0]
        terms = (Ix * Ix, Ix * Iy, Iy * Iy, Ix * It, Iy * It, It * It)
        Jb = [t if j is None else j + t for j, t in zip(Jb, terms)]
        Ixx = half * (sample(c, 3) + R1[..., c, 3])
        Ixy = half * (sample(c, 4) + R1[..., c, 4])
        Iyy = half * (sample(c, 5) + R1[..., c, 5])
        Ixt = sample(c, 1) - R1[..., c, 1]
        Iyt = sample(c, 2) - R1[..., c, 2]
        terms = (Ixx * Ixx + Ixy * Ixy, Ixx * Ixy + Ixy * Iyy, Ixy * Ixy + Iyy * Iyy, Ixx * Ixt + Ixy * Iyt, Ixy * Ixt + Iyy * Iyt,
                 Ixt * Ixt + Iyt * Iyt)
        Jg = [t if j is None else j + t for j, t in zip(Jg, terms)]
    zero = dt(0)
    return (np.stack([np.where(valid, j, zero) for j in Jb]).astype(dt), np.stack([np.where(valid, j, zero) for j in Jg]).astype(dt))


def weights(Jb, Jg, uv, d, eps=1e-3, beta=BETA, gamma=GAMMA, dt=np.float64):
    """-> (J [6,H,W] = (beta psi_b) Jb + (gamma psi_g) Jg, psi [2,H,W] = (1, psi_s))."""
    Jb, Jg = np.asarray(Jb).astype(dt), np.asarray(Jg).astype(dt)
    pb = vf_weights(Jb, uv, d, eps, dt)
    pg = vf_weights(Jg, uv, d, eps, dt)
    wb, wg = dt(beta) * pb[0], dt(gamma) * pg[0]
    J = np.stack([wb * Jb[q] + wg * Jg[q] for q in range(6)]).astype(dt)
    return J, np.stack([np.ones_like(pb[1]), pb[1]]).astype(dt)


def flow_planar(imgA, imgB, dt=np.float64, trace=None, gamma=GAMMA, beta=BETA, **over):
    """The whole estimate A -> B on planar fields.  -> uv [2,H,W] in dt.  trace, a list, receives one dict per (level, warp):
    level, warp, I1, I2, R1, R2, uv (before the warp), Jb, Jg, J, psi and d_in of the last weight pass, d (after it)."""
    p = vr.params(**over)
    gamma, beta = check_terms(gamma, beta)
    A, B = pyramid(imgA, dt), pyramid(imgB, dt)
    RA, RB = [derivs(a, dt) for a in A], [derivs(b, dt) for b in B]
    uv = np.zeros((2,) + A[-1].shape[:2], dt)
    for lev in range(len(A) - 1, -1, -1):
        R1, R2 = RA[lev], RB[lev]
        if lev != len(A) - 1:
            uv = expand(uv, R1.shape[0], R1.shape[1], dt)
        for k in range(int(p['NW'])):
            Jb, Jg = tensor(R1, R2, uv, dt)
            d = np.zeros_like(uv)
            for _ in range(int(p['NO'])):
                d_in = d
                J, psi = weights(Jb, Jg, uv, d, p['eps'], beta, gamma, dt)
                d = sor(J, psi, uv, d, p['alpha'], p['omega'], p['NI'], dt)
            if trace is not None:
                trace.append(dict(level=lev, warp=k, I1=A[lev], I2=B[lev], R1=R1, R2=R2, uv=uv, Jb=Jb, Jg=Jg, J=J, psi=psi, d_in=d_in, d=d))
            uv = (uv + d).astype(dt)
    return uv


def flow(imgA, imgB, dt=np.float64, trace=None, gamma=GAMMA, beta=BETA, **over):
    """-> [H,W,2] in dt."""
    return np.ascontiguousarray(np.moveaxis(flow_planar(imgA, imgB, dt, trace, gamma, beta, **over), 0, -1))


# ---- fixtures: the pairs of varflow_restated with the second frame relit ----------------------------------------------------------

def relight(img, kind):
    """uint8 [H,W,3] -> uint8: gain 0.75 f + 30; ramp f (0.7 + 0.4 x / (W - 1)) + 10; shadow 0.6 f where x + y > (H + W) / 2."""
    f = np.asarray(img).astype(np.float64)
    H, W = f.shape[:2]
    ys, xs = np.mgrid[0:H, 0:W]
    if kind == 'gain':
        out = 0.75 * f + 30
    elif kind == 'ramp':
        out = f * (0.7 + 0.4 * xs / (W - 1))[..., None] + 10
    elif kind == 'shadow':
        out = f * np.where(xs + ys > (H + W) / 2, 0.6, 1.)[..., None]
    else:
        raise KeyError(kind)
    return vr.quantise(out)


@functools.lru_cache(maxsize=None)
def fixture(name, kind=None):
    """The pair `name` of varflow_restated, its imgB relit by `kind` (None: unchanged); truth and masks are those of the pair."""
    p = vr.fixture(name)
    if kind is None:
        return p
    return vr.Pair('%s/%s' % (name, kind), p.imgA, relight(p.imgB, kind), p.truth_ab, p.truth_ba, p.maskA, p.maskB)


@functools.lru_cache(maxsize=None)
def restated(name, kind=None, dtype='float64'):
    """(flow [H,W,2], trace) of the fixture at gamma = 5, beta = 1 and the default parameters, computed once; read-only."""
    pair = fixture(name, kind)
    trace = []
    f = flow(pair.imgA, pair.imgB, np.dtype(dtype).type, trace)
    return f, trace


@functools.lru_cache(maxsize=None)
def brightness_only(name, kind=None):
    """flow [H,W,2] of varflow_restated.flow (brightness constancy alone) on the same pair, float64."""
    pair = fixture(name, kind)
    return vr.flow(pair.imgA, pair.imgB)
