"""Float64 restatement of the motion segmentation (include/lasr_ops.h) in numpy, and the analytic fixtures
tests/test_motionseg_cpu.py and tests/test_motionseg_gpu.py share.  Nothing here imports the package: the kernels of
lasr_amd/csrc/motionseg.hip and the passes of lasr_amd/nnutils/motionseg.py are compared against this file, not the other way round.

Per-pixel arithmetic runs in the working precision `dt` (float64 by default; float32 gives the spread the GPU tolerances are
derived from, and is the operation order the kernels follow); everything summed over pixels is float64 whatever dt is.  Fields
are [H,W], flows [H,W,2] = (x, y) in pixels.  The mean field, the sigmoid, the bilinear taps and the Sequence fixture are those of
tests/maskprop_restated.py.
"""
import functools

import numpy as np
from scipy import ndimage

import maskprop_restated as mr

MOMENTS, BINS, STATE = 28, 1024, 12
MODELS = {'translation': 0, 'affine': 1, 'quadratic': 2}
DEFAULTS = dict(tau=1., model='quadratic', iters=8, k_sigma=3., sigma_min=0.25, ridge=1e-9, kappa=4., U=6., gap=1, min_share=0.01,
                max_share=0.5, min_spacing=10, min_score=1., n_keys=1)
ENABLED = {0: (0, 3), 1: (0, 1, 2, 3, 4, 5), 2: tuple(range(8))}
# the monomials X^i Y^j with i + j <= 4 by degree, then by j: slot d (d + 1) / 2 + j
EXPONENTS = [(d - j, j) for d in range(5) for j in range(d + 1)]
SLOT = {e: k for k, e in enumerate(EXPONENTS)}
# the model's basis: u_m = B_u . theta, v_m = B_v . theta; an entry is the exponent pair of its monomial or None for 0
B_U = [(0, 0), (1, 0), (0, 1), None, None, None, (2, 0), (1, 1)]
B_V = [None, None, None, (0, 0), (1, 0), (0, 1), (1, 1), (0, 2)]
TH, SIGMA, MED, N, STATUS = slice(0, 8), 8, 9, 10, 11


class NoMovingObject(ValueError):
    pass


def params(**over):
    p = dict(DEFAULTS)
    unknown = set(over) - set(p)
    assert not unknown, unknown
    p.update(over)
    return p


def model_id(model):
    return MODELS[model] if isinstance(model, str) else int(model)


def confidence(f_ab, f_ba, tau=1., dt=np.float64):
    """conf [H,W] in dt of the pair a -> b: q = p + f_ab(p); outside [0,W-1] x [0,H-1] or not finite: 0, else
    exp(-|f_ab(p) + bilinear(f_ba, q)|^2 / (2 tau^2)); a result that is not a number is 0."""
    H, W = f_ab.shape[:2]
    f_ab, f_ba = f_ab[..., :2].astype(dt), f_ba[..., :2].astype(dt)
    ys, xs = np.mgrid[0:H, 0:W]
    fx, fy = f_ab[..., 0], f_ab[..., 1]
    with np.errstate(invalid='ignore', over='ignore'):
        qx, qy = xs.astype(dt) + fx, ys.astype(dt) + fy
        inside = (qx >= 0) & (qx <= W - 1) & (qy >= 0) & (qy <= H - 1)
        qxc, qyc = np.where(inside, qx, dt(0)), np.where(inside, qy, dt(0))
        ex = fx + mr.bilinear(f_ba[..., 0], qxc, qyc, dt)
        ey = fy + mr.bilinear(f_ba[..., 1], qxc, qyc, dt)
        inv = dt(1) / (dt(2) * dt(tau) * dt(tau))
        c = np.exp(-(ex * ex + ey * ey) * inv)
        return np.where(inside & (c >= 0), c, dt(0)).astype(dt)


def coords(H, W):
    """Normalised pixel coordinates, float64 [H,W] each: s = 0.5 max(H, W), X = (x - 0.5 (W-1)) / s, Y = (y - 0.5 (H-1)) / s."""
    s = 0.5 * max(H, W)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    return (xs - 0.5 * (W - 1)) / s, (ys - 0.5 * (H - 1)) / s


def model_flow(theta, X, Y, dt=np.float64):
    """(u_m, v_m) in dt at the coordinates X, Y (rounded to dt), the sums evaluated from left to right."""
    th = np.asarray(theta, np.float64)[:8].astype(dt)
    X, Y = X.astype(dt), Y.astype(dt)
    um = th[0] + th[1] * X + th[2] * Y + th[6] * (X * X) + th[7] * (X * Y)
    vm = th[3] + th[4] * X + th[5] * Y + th[6] * (X * Y) + th[7] * (Y * Y)
    return um, vm


def initial_state():
    S = np.zeros(STATE, np.float64)
    S[SIGMA] = np.inf
    return S


def _skipped(flow, conf):
    return ~(conf > 0) | ~np.isfinite(flow[..., 0]) | ~np.isfinite(flow[..., 1])


def residual2(flow, state, dt=np.float64):
    """r^2 [H,W] in dt against state's theta (garbage where the flow is not finite: the callers skip those pixels)."""
    H, W = flow.shape[:2]
    X, Y = coords(H, W)
    um, vm = model_flow(state[TH], X, Y, dt)
    with np.errstate(invalid='ignore', over='ignore'):
        du, dv = flow[..., 0].astype(dt) - um, flow[..., 1].astype(dt) - vm
        return du * du + dv * dv


def weights(r2, conf, state, dt=np.float64):
    """conf for sigma = inf, else the Geman-McClure weight conf / (1 + r^2 / sigma^2)^2, in dt."""
    if np.isinf(state[SIGMA]):
        return conf.astype(dt)
    sig = dt(state[SIGMA])
    with np.errstate(invalid='ignore', over='ignore'):
        t = dt(1) + r2 / (sig * sig)
        return (conf.astype(dt) / (t * t)).astype(dt)


def moments(flow, conf, state, dt=np.float64):
    """-> (M float64 [28], hist int64 [1024]) of one IRLS iteration from `state`.  M: sum w X^i Y^j over EXPONENTS (15), then
    sum w u X^i Y^j and sum w v X^i Y^j for i + j <= 2 (6 + 6), then sum w (u^2 + v^2).  hist: the pixels with conf >= 0.5 by
    min(floor(16 sqrt(r^2)), 1023).  A pixel with conf not > 0 or a flow that is not finite is skipped, not weighted by 0."""
    H, W = flow.shape[:2]
    conf = conf.astype(dt)
    keep = ~_skipped(flow, conf)
    r2 = residual2(flow, state, dt)
    w = weights(r2, conf, state, dt)[keep].astype(np.float64)
    X, Y = coords(H, W)
    X, Y = X[keep], Y[keep]
    u, v = flow[..., 0][keep].astype(dt).astype(np.float64), flow[..., 1][keep].astype(dt).astype(np.float64)
    M = np.zeros(MOMENTS, np.float64)
    mono = [X ** i * Y ** j for i, j in EXPONENTS]
    for k in range(15):
        M[k] = (w * mono[k]).sum()
    for k in range(6):
        M[15 + k] = (w * u * mono[k]).sum()
        M[21 + k] = (w * v * mono[k]).sum()
    M[27] = (w * (u * u + v * v)).sum()
    sel = keep & (conf >= dt(0.5))
    with np.errstate(invalid='ignore', over='ignore'):
        b = np.floor(dt(16) * np.sqrt(r2[sel]))
    b = np.where(b < 1023, b, 1023).astype(np.int64)
    return M, np.bincount(b, minlength=BINS).astype(np.int64)


def near_integer(flow, conf, state, tol=1e-5):
    """The pixels of the histogram whose float64 16 r lies within tol of an integer >= 1 (r >= 0: nothing rounds below bin 0),
    the only ones on which a float32 evaluation may pick the neighbouring bin.  -> their number."""
    conf = conf.astype(np.float64)
    sel = ~_skipped(flow, conf) & (conf >= 0.5)
    v = 16. * np.sqrt(residual2(flow, state)[sel])
    k = np.rint(v)
    return int(((np.abs(v - k) <= tol) & (k >= 1) & (k <= 1023)).sum())


def assemble(M):
    """The 8 x 8 normal matrix sum w (B_u B_u^T + B_v B_v^T) and its right-hand side sum w (u B_u + v B_v), from the moments only."""
    A, b = np.zeros((8, 8), np.float64), np.zeros(8, np.float64)
    for i in range(8):
        for j in range(8):
            for B in (B_U, B_V):
                if B[i] is not None and B[j] is not None:
                    A[i, j] += M[SLOT[(B[i][0] + B[j][0], B[i][1] + B[j][1])]]
        if B_U[i] is not None:
            b[i] += M[15 + SLOT[B_U[i]]]
        if B_V[i] is not None:
            b[i] += M[21 + SLOT[B_V[i]]]
    return A, b


def cholesky_solve(A, b):
    """-> (ok, x) with A x = b by A = L L^T in float64; ok is False when a pivot is not > 0."""
    n = len(b)
    L = np.zeros((n, n), np.float64)
    for j in range(n):
        d = A[j, j]
        for k in range(j):
            d -= L[j, k] * L[j, k]
        if not d > 0:
            return False, np.zeros(n)
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, n):
            s = A[i, j]
            for k in range(j):
                s -= L[i, k] * L[j, k]
            L[i, j] = s / L[j, j]
    y = np.zeros(n, np.float64)
    for i in range(n):
        s = b[i]
        for k in range(i):
            s -= L[i, k] * y[k]
        y[i] = s / L[i, i]
    x = np.zeros(n, np.float64)
    for i in range(n - 1, -1, -1):
        s = y[i]
        for k in range(i + 1, n):
            s -= L[k, i] * x[k]
        x[i] = s / L[i, i]
    return True, x


def solve(M, hist, state, model=2, k_sigma=3., sigma_min=0.25, ridge=1e-9):
    """The state after one iteration.  Switched-off parameters: row and column of the identity, right-hand side 0; then
    ridge trace(A) / 8 on the diagonal; then the Cholesky solution of the STEP, A d = b - A0 theta_in with A0 the matrix before the
    ridge, theta = theta_in + d (the fixed point is the un-ridged solution, so the ridge guards the pivots without biasing the
    fit).  n = the histogram's total.  A pivot not > 0 or n = 0: status 1, theta, sigma and med stay.  Else med = (the first bin
    at which the cumulative count reaches ceil(n / 2) + 0.5) / 16 and sigma = max(k_sigma med, sigma_min): the scale is lagged, the
    histogram is of the residuals against theta_in.  k_sigma, sigma_min and ridge are rounded to float32, as the C ABI takes them."""
    out = np.array(state, np.float64)
    k_sigma, sigma_min, ridge = (np.float64(np.float32(v)) for v in (k_sigma, sigma_min, ridge))
    n = int(np.asarray(hist).sum())
    out[N] = n
    A, b = assemble(M)
    on = ENABLED[model_id(model)]
    th = np.array(state[TH], np.float64)
    for k in range(8):
        if k not in on:
            A[k, :], A[:, k], b[k], th[k] = 0, 0, 0, 0
            A[k, k] = 1
    rhs = b - A @ th
    for k in range(8):
        if k not in on:
            rhs[k] = 0
    tr = 0.
    for k in range(8):
        tr += A[k, k]
    A = A + np.eye(8) * (ridge * tr / 8)
    ok, d = cholesky_solve(A, rhs)
    if not ok or n == 0 or not np.isfinite(d).all():
        out[STATUS] = 1
        return out
    cum = np.cumsum(np.asarray(hist, np.int64))
    med = (int(np.argmax(cum >= (n + 1) // 2)) + 0.5) / 16
    out[TH] = th + d
    out[SIGMA], out[MED], out[STATUS] = max(k_sigma * med, sigma_min), med, 0
    return out


def fit(flow, conf, p=None, dt=np.float64, states=None):
    """`iters` IRLS iterations from theta = 0, sigma = inf.  -> the state; `states`, a list, receives every iteration's."""
    p = p or params()
    S = initial_state()
    for _ in range(int(p['iters'])):
        M, h = moments(flow, conf, S, dt)
        S = solve(M, h, S, p['model'], p['k_sigma'], p['sigma_min'], p['ridge'])
        if states is not None:
            states.append(S.copy())
    return S


def evidence(flow, conf, state, kappa=4., U=6., dt=np.float64):
    """e = conf clamp(r^2 / sigma^2 - kappa, -U, U) in dt, 0 where the pixel is skipped."""
    conf = conf.astype(dt)
    skip = _skipped(flow, conf)
    r2 = residual2(flow, state, dt)
    sig = dt(state[SIGMA])
    with np.errstate(invalid='ignore', over='ignore'):
        e = conf * np.clip(r2 / (sig * sig) - dt(kappa), -dt(U), dt(U))
    return np.where(skip, dt(0), e).astype(dt)


def largest_component(fg):
    """bool [H,W] -> its largest 8-connected component (the lowest label among equals); all False when fg is empty."""
    lab, n = ndimage.label(fg, structure=np.ones((3, 3), int))
    if n == 0:
        return np.zeros(fg.shape, bool)
    area = np.bincount(lab.ravel(), minlength=n + 1)
    area[0] = 0
    return lab == int(np.argmax(area))


def score(u, P, fits_ok, p):
    """The score of a frame from its summed evidence u and its mask P (host arithmetic, float64)."""
    share = float(P.mean())
    if not fits_ok or not p['min_share'] <= share <= p['max_share']:
        return 0.
    u = u.astype(np.float64)
    edge = P & ~ndimage.binary_erosion(P, structure=np.ones((3, 3), bool), border_value=0)
    rim = np.zeros(P.shape, bool)
    rim[0, :], rim[-1, :], rim[:, 0], rim[:, -1] = True, True, True, True
    b = min(1., float((P & rim).sum()) / float(edge.sum()))
    return float((u[P].mean() - u[~P].mean()) * (1 - b))


def select_keys(scores, p):
    """Greedy by descending score, ties to the lower index; a frame within min_spacing of a chosen key is skipped; stops at n_keys
    or at the first score below min_score.  -> the sorted list of key frames; raises NoMovingObject when it is empty."""
    keys = []
    for t in sorted(range(len(scores)), key=lambda t: (-scores[t], t)):
        if len(keys) >= int(p['n_keys']) or scores[t] < p['min_score']:
            break
        if all(abs(t - k) >= int(p['min_spacing']) for k in keys):
            keys.append(t)
    if not keys:
        raise NoMovingObject('no frame scores %g or more (best %.3g)' % (p['min_score'], max(scores) if len(scores) else 0.))
    return sorted(keys)


def segment(frames, flow_of, dt=np.float64, **over):
    """frames uint8 [T,H,W,3], flow_of(a, b) = the flow a -> b.  -> (masks [T,H,W] bool, soft [T,H,W] in dt = q after the mean
    field, scores [T], report with the summed evidence per frame and the state of every ordered pair)."""
    p, mp = params(**over), mr.params()
    T, g = len(frames), int(p['gap'])
    masks, soft, scores, us, states = [], [], [], [], {}
    for t in range(T):
        u, ok, pairs = np.zeros(frames[t].shape[:2], dt), True, 0
        for s in (t - g, t + g):
            if not 0 <= s < T:
                continue
            f = flow_of(t, s)
            c = confidence(f, flow_of(s, t), p['tau'], dt)
            S = fit(f, c, p, dt)
            u = (u + evidence(f, c, S, p['kappa'], p['U'], dt)).astype(dt) if pairs else evidence(f, c, S, p['kappa'], p['U'], dt)
            ok, pairs = ok and S[STATUS] == 0, pairs + 1
            states[(t, s)] = S
        q = mr.sigmoid(u, dt)
        for _ in range(int(mp['K'])):
            q = mr.meanfield(frames[t], u, q, mp, dt)
        P = largest_component(q > 0.5)
        masks.append(P)
        soft.append(q)
        us.append(u)
        scores.append(score(u, P, ok and pairs > 0, p))
    return np.stack(masks), np.stack(soft), np.array(scores), dict(params=p, u=np.stack(us), states=states)


def auto_keys(frames, flow_of, dt=np.float64, **over):
    masks, _, scores, rep = segment(frames, flow_of, dt, **over)
    return {t: masks[t] for t in select_keys(list(scores), rep['params'])}


# ---- fixtures ---------------------------------------------------------------------------------------------------------------------

THETA = (2.5, 0.8, -0.3, -1.0, 0.3, 0.6, 0.2, -0.15)


class FlowCase:
    """Direct flow fields: the background follows the 8-parameter model `theta` from every frame to the next (the flow back is
    its inverse, by fixed-point iteration, so the pair is consistent to rounding), and an ellipse of axes `axes` moves by `rel`
    px per frame on top of the background's flow at its first centre.  flow(a, b) for |a - b| = 1 on the grid of a; float64, rounded by the caller."""

    def __init__(self, H, W, T, c0, axes, rel=(4.5, 1.0), theta=THETA, noise=0., seed=0, obj=True):
        self.H, self.W, self.T, self.theta = H, W, T, np.array(theta, np.float64)
        X, Y = coords(H, W)
        self._X, self._Y = X, Y
        ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
        self._xs, self._ys = xs, ys
        ux, uy = self._model(float(c0[0]), float(c0[1]))        # the background's flow under the object in frame 0
        self.vel = np.array([ux + rel[0], uy + rel[1]])
        self.masks = []
        for t in range(T):
            c = np.array(c0, float) + t * self.vel
            m = ((xs - c[0]) / axes[0]) ** 2 + ((ys - c[1]) / axes[1]) ** 2 <= 1
            self.masks.append(m if obj else np.zeros((H, W), bool))
        self.masks = np.stack(self.masks)
        rng = np.random.default_rng(seed)
        self._noise = {}
        if noise:
            for a in range(T):
                for b in (a - 1, a + 1):
                    if 0 <= b < T:
                        self._noise[(a, b)] = np.stack([mr.smooth_noise(rng, (H, W), 8, noise) for _ in range(2)], -1)

    def _model(self, x, y):
        s = 0.5 * max(self.H, self.W)
        X, Y = (x - 0.5 * (self.W - 1)) / s, (y - 0.5 * (self.H - 1)) / s
        th = self.theta
        return (th[0] + th[1] * X + th[2] * Y + th[6] * X * X + th[7] * X * Y,
                th[3] + th[4] * X + th[5] * Y + th[6] * X * Y + th[7] * Y * Y)

    def flow(self, a, b):
        assert abs(a - b) == 1
        if b > a:
            fx, fy = self._model(self._xs, self._ys)
        else:                                               # the point p with p + F(p) = q, and the flow back -F(p)
            px, py = self._xs.copy(), self._ys.copy()
            for _ in range(60):
                fx, fy = self._model(px, py)
                px, py = self._xs - fx, self._ys - fy
            fx, fy = self._model(px, py)
            fx, fy = -fx, -fy
        f = np.stack([fx, fy], -1)
        f[self.masks[a]] = self.vel * (b - a)
        if (a, b) in self._noise:
            f = f + self._noise[(a, b)]
        return f

    def pair(self, a, b, dtype=np.float32):
        """-> (flow a -> b, flow b -> a) in dtype."""
        return self.flow(a, b).astype(dtype), self.flow(b, a).astype(dtype)


@functools.lru_cache(maxsize=None)
def flow_case(name):
    """pan / pan_noisy: 64 x 80, 8 frames, the prototype's table.  odd: 37 x 53.  tiny: 9 x 7 (fewer pixels than one workgroup).
    large: 300 x 500 = 150000 pixels, more than the 65536 one sweep of the reduction grid covers.  plain: no object."""
    if name == 'pan':
        return FlowCase(64, 80, 8, (14, 28), (11, 15))
    if name == 'pan_noisy':
        return FlowCase(64, 80, 8, (14, 28), (11, 15), noise=0.5, seed=3)
    if name == 'odd':
        return FlowCase(37, 53, 3, (14, 17), (9, 11), noise=0.3, seed=5)
    if name == 'tiny':
        return FlowCase(9, 7, 2, (3, 4), (1.6, 2.1), rel=(1.5, 0.5), theta=(0.6, 0.2, -0.1, -0.3, 0.1, 0.15, 0.05, -0.04))
    if name == 'large':
        return FlowCase(300, 500, 2, (200, 140), (60, 45), rel=(6.0, -2.5), noise=0.4, seed=9)
    if name == 'plain':
        return FlowCase(64, 80, 2, (0, 0), (1, 1), obj=False)
    raise KeyError(name)


def holes(variant='holes'):
    """The first pair of `pan` with bad pixels.  -> (flow, flow back, the mask of the bad pixels), float32.  'holes': a block of
    NaN flows and a block of flows that leave the frame; 'all': every flow is NaN or leaves the frame."""
    f, fb = flow_case('pan').pair(0, 1)
    f, bad = f.copy(), np.zeros(f.shape[:2], bool)
    if variant == 'all':
        f[:] = 1000.
        f[::2] = np.nan
        bad[:] = True
    else:
        f[5:12, 40:52] = np.nan
        f[30:33, 60:61, 1] = np.inf
        f[44:58, 8:21] = (-300., 40.)
        bad[5:12, 40:52] = bad[30:33, 60:61] = bad[44:58, 8:21] = True
    return f, fb, bad


class PanSequence(mr.Sequence):
    """maskprop_restated.Sequence seen by a moving camera: the background of frame t is a texture sampled at the world point
    A_t (p - c) + c + b_t, with A_t a rotation by t rot and a zoom 1 + t zoom and b_t = t pan, so the background flow s -> t is
    A_t^-1 (A_s (p - c) + b_s - b_t) + c - p: closed form and affine in p.  The ellipse moves as in Sequence, in image coordinates."""

    def __init__(self, H, W, T, c0, vel, axes0, grow, seed, pan=(-1.5, 0.5), rot=0.004, zoom=0.003, flow_noise=0.):
        rng = np.random.default_rng(seed)
        self.H, self.W, self.T = H, W, T
        self.c = [np.array(c0, float) + t * np.array(vel, float) for t in range(T)]
        self.axes = [np.array(axes0, float) * (1 + t * np.array(grow, float)) for t in range(T)]
        self.ctr = np.array([0.5 * (W - 1), 0.5 * (H - 1)])
        self.A = [(1 + t * zoom) * np.array([[np.cos(t * rot), -np.sin(t * rot)], [np.sin(t * rot), np.cos(t * rot)]]) for t in range(T)]
        self.b = [t * np.array(pan, float) for t in range(T)]
        obj_base, bg_base = np.array([200., 80., 60.]), np.array([60., 120., 170.])
        pad = 24
        tex = np.stack([mr.smooth_noise(rng, (64, 64), 5, 25) for _ in range(3)], -1) + obj_base
        world = np.stack([mr.smooth_noise(rng, (H + 2 * pad, W + 2 * pad), 4, 25) for _ in range(3)], -1) + bg_base
        ys, xs = np.mgrid[0:H, 0:W].astype(float)
        self.frames, self.masks = [], []
        for t in range(T):
            nx, ny = (xs - self.c[t][0]) / self.axes[t][0], (ys - self.c[t][1]) / self.axes[t][1]
            inside = nx * nx + ny * ny <= 1
            coords_o = [(np.clip(ny, -1.05, 1.05) / 2.1 + 0.5) * 63, (np.clip(nx, -1.05, 1.05) / 2.1 + 0.5) * 63]
            obj = np.stack([ndimage.map_coordinates(tex[..., ch], coords_o, order=1) for ch in range(3)], -1)
            wx, wy = self._world(t, xs, ys)
            bg = np.stack([ndimage.map_coordinates(world[..., ch], [wy + pad, wx + pad], order=1, mode='nearest') for ch in range(3)], -1)
            img = np.where(inside[..., None], obj, bg) + rng.integers(-2, 3, (H, W, 3))
            self.frames.append(np.clip(np.rint(img), 0, 255).astype(np.uint8))
            self.masks.append(inside)
        self.frames, self.masks = np.stack(self.frames), np.stack(self.masks)
        self._xs, self._ys = xs, ys
        self._noise = {}
        if flow_noise:
            for s in range(T):
                for t in (s - 1, s + 1):
                    if 0 <= t < T:
                        self._noise[(s, t)] = np.stack([mr.smooth_noise(rng, (H, W), 8, flow_noise) for _ in range(2)], -1)
        self._index = {f.tobytes(): i for i, f in enumerate(self.frames)}
        self.calls = []

    def _world(self, t, x, y):
        dx, dy = x - self.ctr[0], y - self.ctr[1]
        A = self.A[t]
        return (A[0, 0] * dx + A[0, 1] * dy + self.ctr[0] + self.b[t][0], A[1, 0] * dx + A[1, 1] * dy + self.ctr[1] + self.b[t][1])

    def background_flow(self, s, t):
        wx, wy = self._world(s, self._xs, self._ys)
        Ai = np.linalg.inv(self.A[t])
        dx, dy = wx - self.ctr[0] - self.b[t][0], wy - self.ctr[1] - self.b[t][1]
        return np.stack([Ai[0, 0] * dx + Ai[0, 1] * dy + self.ctr[0] - self._xs, Ai[1, 0] * dx + Ai[1, 1] * dy + self.ctr[1] - self._ys], -1)

    def flow(self, s, t):
        r = self.axes[t] / self.axes[s]
        fx = (self._xs - self.c[s][0]) * r[0] + self.c[t][0] - self._xs
        fy = (self._ys - self.c[s][1]) * r[1] + self.c[t][1] - self._ys
        f = np.where(self.masks[s][..., None], np.stack([fx, fy], -1), self.background_flow(s, t))
        if (s, t) in self._noise:
            f = f + self._noise[(s, t)]
        return f.astype(np.float32)

    def flow_fn(self, imgA, imgB):
        a, b = self._index[np.ascontiguousarray(imgA).tobytes()], self._index[np.ascontiguousarray(imgB).tobytes()]
        self.calls.append((a, b))
        f = self.flow(a, b)
        return np.concatenate([f, np.ones(f.shape[:2] + (1,), np.float32)], -1), np.zeros(f.shape[:2], np.float32)


@functools.lru_cache(maxsize=None)
def sequence(name):
    """pan / pan_noisy (flow noise 0.5 px): 64 x 80, 8 frames, the ellipse of maskprop_restated's fixture under a moving camera."""
    if name == 'pan':
        return PanSequence(64, 80, 8, (24, 28), (4.5, 1.0), (11, 15), (0.05, -0.025), seed=7)
    if name == 'pan_noisy':
        return PanSequence(64, 80, 8, (24, 28), (4.5, 1.0), (11, 15), (0.05, -0.025), seed=7, flow_noise=0.5)
    raise KeyError(name)
