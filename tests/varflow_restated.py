"""Restatement of the variational optical flow (include/lasr_ops.h) in plain numpy, and the seeded fixtures
tests/test_varflow_cpu.py and tests/test_varflow_gpu.py share.  Nothing here imports the package or torch: the kernels of
lasr_amd/csrc/varflow.hip and the passes of lasr_amd/nnutils/varflow.py are compared against this file, not the other way round.

This file is the definition.  Every function takes the working precision `dt` (float64 by default) and computes in it alone: run
in float32 it follows the kernels' operation order, and its distance from the float64 run is what the GPU bounds are derived from.
Images are uint8 [H,W,3] (or [H,W,3] in dt / 255 once converted); flow fields inside the solver are planar [2,H,W] = (u, v) in
pixels, the public flow is [H,W,2]; the convention is I1(p) ~ I2(p + f(p)).
"""
import functools

import numpy as np

DEFAULTS = dict(alpha=0.03, eps=1e-3, omega=1.8, NW=5, NO=3, NI=10)
OCC_TAU, OCC_S, OCC_CLAMP = 1.0, 0.5, 6.0
KERNEL = (1., 4., 6., 4., 1.)                       # / 16: Burt-Adelson, a = 0.375
TINY = np.float32(1.17549435e-38)                   # the smallest positive normal float32: what an exact 0 of occ is written as


def params(**over):
    p = dict(DEFAULTS)
    unknown = set(over) - set(p)
    assert not unknown, unknown
    p.update(over)
    return p


def level_shapes(H, W):
    """[(H, W), (ceil(H/2), ceil(W/2)), ...]: REDUCE repeats while the smaller side of the last level is >= 32."""
    out = [(H, W)]
    while min(out[-1]) >= 32:
        h, w = out[-1]
        out.append(((h + 1) // 2, (w + 1) // 2))
    return out


def to_unit(img, dt=np.float64):
    """uint8 -> dt / 255."""
    return (np.asarray(img).astype(dt) / dt(255)).astype(dt)


def reduce(a, dt=np.float64):
    """One REDUCE of [H,W] or [H,W,C]: out(y,x) = sum_i k_i (sum_j k_j a(clamp(2y+i), clamp(2x+j))), i and j from -2 to 2 in
    that order, each sum started from its first term."""
    a = np.asarray(a).astype(dt)
    H, W = a.shape[:2]
    h, w = (H + 1) // 2, (W + 1) // 2
    k = [dt(v) / dt(16) for v in KERNEL]
    ys, xs = 2 * np.arange(h), 2 * np.arange(w)
    out = None
    for i in range(5):
        row = a[np.clip(ys + i - 2, 0, H - 1)]
        acc = None
        for j in range(5):
            t = k[j] * row[:, np.clip(xs + j - 2, 0, W - 1)]
            acc = t if acc is None else acc + t
        t = k[i] * acc
        out = t if out is None else out + t
    return out.astype(dt)


def pyramid(img, dt=np.float64):
    """uint8 [H,W,3] -> the list of levels in dt, finest first."""
    levels = [to_unit(img, dt)]
    for _ in level_shapes(*levels[0].shape[:2])[1:]:
        levels.append(reduce(levels[-1], dt))
    return levels


def _lerp4(v00, v01, v10, v11, tx, ty, dt):
    one = dt(1)
    return (v00 * (one - tx) + v01 * tx) * (one - ty) + (v10 * (one - tx) + v11 * tx) * ty


def expand(uv, h, w, dt=np.float64):
    """[2,hc,wc] -> [2,h,w]: 2 * the bilinear sample at (y/2, x/2), the upper taps clamped."""
    uv = np.asarray(uv).astype(dt)
    hc, wc = uv.shape[1:]
    sy, sx = np.arange(h).astype(dt) * dt(0.5), np.arange(w).astype(dt) * dt(0.5)
    y0, x0 = np.floor(sy).astype(np.int64), np.floor(sx).astype(np.int64)
    ty, tx = (sy - np.floor(sy)).astype(dt)[:, None], (sx - np.floor(sx)).astype(dt)[None, :]
    y1, x1 = np.minimum(y0 + 1, hc - 1), np.minimum(x0 + 1, wc - 1)
    out = []
    for f in uv:
        out.append(dt(2) * _lerp4(f[y0][:, x0], f[y0][:, x1], f[y1][:, x0], f[y1][:, x1], tx, ty, dt))
    return np.stack(out).astype(dt)


def neighbours(a):
    """(left, right, up, down) of [H,W,...] with a replicated border."""
    return (np.concatenate([a[:, :1], a[:, :-1]], 1), np.concatenate([a[:, 1:], a[:, -1:]], 1),
            np.concatenate([a[:1], a[:-1]], 0), np.concatenate([a[1:], a[-1:]], 0))


def gradient(a, dt=np.float64):
    """Central differences 0.5 (a[x+1] - a[x-1]) with a replicated border.  -> (gx, gy)."""
    l, r, u, d = neighbours(a)
    return dt(0.5) * (r - l), dt(0.5) * (d - u)


def warp_positions(uv, dt=np.float64):
    """-> (X, Y, valid) of the planar flow [2,H,W]."""
    H, W = uv.shape[1:]
    ys, xs = np.mgrid[0:H, 0:W]
    X, Y = xs.astype(dt) + uv[0], ys.astype(dt) + uv[1]
    valid = (X >= 0) & (X <= W - 1) & (Y >= 0) & (Y <= H - 1)
    return X, Y, valid


def tensor(I1, I2, uv, dt=np.float64):
    """Step 1.  I1, I2 [H,W,3] in dt, uv [2,H,W].  -> J [6,H,W] = (J11, J12, J22, J13, J23, J33), valid folded in."""
    I1, I2, uv = np.asarray(I1).astype(dt), np.asarray(I2).astype(dt), np.asarray(uv).astype(dt)
    H, W = uv.shape[1:]
    X, Y, valid = warp_positions(uv, dt)
    Xc, Yc = np.clip(X, dt(0), dt(W - 1)), np.clip(Y, dt(0), dt(H - 1))
    fx, fy = np.floor(Xc), np.floor(Yc)
    x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    tx, ty = (Xc - fx).astype(dt), (Yc - fy).astype(dt)
    g2x, g2y = gradient(I2, dt)
    g1x, g1y = gradient(I1, dt)

    def sample(f):
        return _lerp4(f[y0, x0], f[y0, x1], f[y1, x0], f[y1, x1], tx, ty, dt)
    J = [None] * 6
    for c in range(3):
        Ix = dt(0.5) * (sample(g2x[..., c]) + g1x[..., c])
        Iy = dt(0.5) * (sample(g2y[..., c]) + g1y[..., c])
        It = sample(I2[..., c]) - I1[..., c]
        terms = (Ix * Ix, Ix * Iy, Iy * Iy, Ix * It, Iy * It, It * It)
        J = [t if j is None else j + t for j, t in zip(J, terms)]
    return np.stack([np.where(valid, j, dt(0)) for j in J]).astype(dt)


def weights(J, uv, d, eps=1e-3, dt=np.float64):
    """Step 2.  -> psi [2,H,W] = (psi_d, psi_s)."""
    J, uv, d = np.asarray(J).astype(dt), np.asarray(uv).astype(dt), np.asarray(d).astype(dt)
    du, dv = d
    e2 = dt(eps) * dt(eps)
    two = dt(2)
    r2 = (du * du) * J[0] + ((two * du) * dv) * J[1] + (dv * dv) * J[2] + (two * du) * J[3] + (two * dv) * J[4] + J[5]
    psid = dt(0.5) / np.sqrt(np.maximum(r2, dt(0)) + e2)
    ux, uy = gradient(uv[0] + du, dt)
    vx, vy = gradient(uv[1] + dv, dt)
    psis = dt(0.5) / np.sqrt(((ux * ux + uy * uy) + (vx * vx + vy * vy)) + e2)
    return np.stack([psid, psis]).astype(dt)


def sor(J, psi, uv, d, alpha=0.03, omega=1.8, iters=10, dt=np.float64):
    """Step 3: `iters` red-black iterations on d = (du, dv); pixels with (x + y) even first.  -> the new d."""
    J, psi, uv = np.asarray(J).astype(dt), np.asarray(psi).astype(dt), np.asarray(uv).astype(dt)
    du, dv = np.asarray(d).astype(dt)
    u, v = uv
    psid, psis = psi
    H, W = u.shape
    ys, xs = np.mgrid[0:H, 0:W]
    ah, om = dt(alpha) * dt(0.5), dt(omega)
    om1 = dt(1) - om
    zero = dt(0)
    pl, pr, pu, pd = neighbours(psis)
    wl, wr = np.where(xs > 0, ah * (psis + pl), zero), np.where(xs < W - 1, ah * (psis + pr), zero)
    wu, wd = np.where(ys > 0, ah * (psis + pu), zero), np.where(ys < H - 1, ah * (psis + pd), zero)
    ws = ((wl + wr) + wu) + wd

    def smooth(f):
        l, r, up, dn = neighbours(f)
        return ((wl * l + wr * r) + wu * up) + wd * dn
    for _ in range(int(iters)):
        for colour in (0, 1):
            m = ((xs + ys) & 1) == colour
            new = om1 * du + om * (((smooth(u + du) - ws * u) - psid * (J[3] + J[1] * dv)) / (psid * J[0] + ws))
            du = np.where(m, new, du)
            new = om1 * dv + om * (((smooth(v + dv) - ws * v) - psid * (J[4] + J[1] * du)) / (psid * J[2] + ws))
            dv = np.where(m, new, dv)
    return np.stack([du, dv]).astype(dt)


def flow_planar(imgA, imgB, dt=np.float64, trace=None, **over):
    """The whole estimate A -> B on planar fields.  -> uv [2,H,W] in dt.  trace, a list, receives one dict per (level, warp):
    level, warp, I1, I2, uv (before the warp), J, psi and d_in of the last weight pass, d (after it)."""
    p = params(**over)
    A, B = pyramid(imgA, dt), pyramid(imgB, dt)
    uv = np.zeros((2,) + A[-1].shape[:2], dt)
    for lev in range(len(A) - 1, -1, -1):
        I1, I2 = A[lev], B[lev]
        if lev != len(A) - 1:
            uv = expand(uv, I1.shape[0], I1.shape[1], dt)
        for k in range(int(p['NW'])):
            J = tensor(I1, I2, uv, dt)
            d = np.zeros_like(uv)
            for _ in range(int(p['NO'])):
                d_in = d
                psi = weights(J, uv, d, p['eps'], dt)
                d = sor(J, psi, uv, d, p['alpha'], p['omega'], p['NI'], dt)
            if trace is not None:
                trace.append(dict(level=lev, warp=k, I1=I1, I2=I2, uv=uv, J=J, psi=psi, d_in=d_in, d=d))
            uv = (uv + d).astype(dt)
    return uv


def flow(imgA, imgB, dt=np.float64, trace=None, **over):
    """-> [H,W,2] in dt."""
    return np.ascontiguousarray(np.moveaxis(flow_planar(imgA, imgB, dt, trace, **over), 0, -1))


def occlusion(f_ab, f_ba, dt=np.float64, tau=OCC_TAU, s=OCC_S):
    """[H,W,2] x 2 -> (occ [H,W] float32, e [H,W] in dt with NaN where p + f_ab(p) leaves the frame)."""
    f_ab, f_ba = np.asarray(f_ab)[..., :2].astype(dt), np.asarray(f_ba)[..., :2].astype(dt)
    H, W = f_ab.shape[:2]
    ys, xs = np.mgrid[0:H, 0:W]
    fx, fy = f_ab[..., 0], f_ab[..., 1]
    X, Y = xs.astype(dt) + fx, ys.astype(dt) + fy
    inside = (X >= 0) & (X <= W - 1) & (Y >= 0) & (Y <= H - 1)
    Xc, Yc = np.where(inside, X, dt(0)), np.where(inside, Y, dt(0))
    flx, fly = np.floor(Xc), np.floor(Yc)
    x0, y0 = flx.astype(np.int64), fly.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    tx, ty = (Xc - flx).astype(dt), (Yc - fly).astype(dt)
    bx = _lerp4(f_ba[y0, x0, 0], f_ba[y0, x1, 0], f_ba[y1, x0, 0], f_ba[y1, x1, 0], tx, ty, dt)
    by = _lerp4(f_ba[y0, x0, 1], f_ba[y0, x1, 1], f_ba[y1, x0, 1], f_ba[y1, x1, 1], tx, ty, dt)
    ex, ey = fx + bx, fy + by
    e = np.sqrt(ex * ex + ey * ey)
    o = np.clip((e - dt(tau)) / dt(s), -dt(OCC_CLAMP), dt(OCC_CLAMP))
    o = np.where(inside, o, dt(OCC_CLAMP)).astype(np.float32)
    o = np.where(o == 0, TINY, o).astype(np.float32)
    return o, np.where(inside, e, np.nan)


def epe(f, truth, region=None):
    """Mean end-point error over `region` (default: everywhere)."""
    e = np.sqrt(((np.asarray(f, np.float64)[..., :2] - truth[..., :2]) ** 2).sum(-1))
    return float(e.mean() if region is None else e[region].mean())


def near_edge(trace, shape, bound):
    """bool [H,W]: the pixels of the finest level that lie under a pixel, of any level and warp of `trace`, whose warped position
    after that warp (p + uv + d) is within `bound` of the frame edge 0, W-1 or H-1 without being exactly on it: there `valid` of the
    next linearisation may differ between two precisions.  A coarse pixel covers the 2^level x 2^level block it was reduced to."""
    H, W = shape
    out = np.zeros((H, W), bool)
    for t in trace:
        uv = np.asarray(t['uv'], np.float64) + np.asarray(t['d'], np.float64)
        h, w = uv.shape[1:]
        X, Y, _ = warp_positions(uv, np.float64)
        m = np.zeros((h, w), bool)
        for P, hi in ((X, w - 1), (Y, h - 1)):
            for edge in (0., float(hi)):
                m |= (np.abs(P - edge) <= bound) & (P != edge)
        if m.any():
            k = 1 << t['level']
            big = np.kron(m, np.ones((k, k), bool))[:H, :W]
            out[:big.shape[0], :big.shape[1]] |= big
    return out


# ---- fixtures ---------------------------------------------------------------------------------------------------------------------

class Texture:
    """A band-limited colour texture in closed form: per channel 128 + sum_k a_k cos(2 pi (fx_k x + fy_k y) + phi_k) with
    |f| between 0.008 and 0.11 cycles per pixel and a_k proportional to 1 / |f|, so it can be sampled anywhere without a resampling
    filter."""

    def __init__(self, rng, n=28, contrast=90.):
        mag = np.exp(rng.uniform(np.log(0.008), np.log(0.11), (3, n)))
        ang = rng.uniform(0, 2 * np.pi, (3, n))
        self.fx, self.fy = mag * np.cos(ang), mag * np.sin(ang)
        self.phi = rng.uniform(0, 2 * np.pi, (3, n))
        amp = 1. / mag
        self.amp = amp * (contrast / np.abs(amp).sum(1, keepdims=True)) * 2.2

    def __call__(self, x, y):
        out = []
        for c in range(3):
            arg = 2 * np.pi * (self.fx[c][:, None, None] * x[None] + self.fy[c][:, None, None] * y[None]) + self.phi[c][:, None, None]
            out.append(128. + (self.amp[c][:, None, None] * np.cos(arg)).sum(0))
        return np.stack(out, -1)


def quantise(img):
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


class Pair:
    """imgA, imgB uint8 [H,W,3]; truth_ab / truth_ba float64 [H,W,2] (None where no closed form is given); inframe_ab: the pixels
    p of A with p + truth_ab(p) inside the frame; for the two-layer case also maskA / maskB, the object's silhouettes."""

    def __init__(self, name, imgA, imgB, truth_ab=None, truth_ba=None, maskA=None, maskB=None):
        self.name, self.imgA, self.imgB, self.truth_ab, self.truth_ba = name, imgA, imgB, truth_ab, truth_ba
        self.maskA, self.maskB = maskA, maskB
        self.H, self.W = imgA.shape[:2]

    def inframe(self, truth):
        ys, xs = np.mgrid[0:self.H, 0:self.W]
        X, Y = xs + truth[..., 0], ys + truth[..., 1]
        return (X >= 0) & (X <= self.W - 1) & (Y >= 0) & (Y <= self.H - 1)


def _affine_pair(name, H, W, seed, M, t):
    """B(q) = T(A^-1 q) for the map p -> q = c + M (p - c) + t about the image centre c: truth_ab(p) = q - p."""
    rng = np.random.default_rng(seed)
    tex = Texture(rng)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    c = np.array([(W - 1) / 2., (H - 1) / 2.])
    M, t = np.asarray(M, np.float64), np.asarray(t, np.float64)
    Mi = np.linalg.inv(M)
    px, py = xs - c[0], ys - c[1]
    ab = np.stack([M[0, 0] * px + M[0, 1] * py + t[0] - px, M[1, 0] * px + M[1, 1] * py + t[1] - py], -1)
    qx, qy = px - t[0], py - t[1]
    sx, sy = Mi[0, 0] * qx + Mi[0, 1] * qy + c[0], Mi[1, 0] * qx + Mi[1, 1] * qy + c[1]      # the point of A seen at q in B
    ba = np.stack([sx - xs, sy - ys], -1)
    return Pair(name, quantise(tex(xs, ys)), quantise(tex(sx, sy)), ab, ba)


def _ellipse_pair(name, H, W, seed, centre, axes, t, t_bg):
    """An object layer (an ellipse moving by t) over a background layer moving by t_bg.  The background moves a little rather than
    not at all: over a static one the estimate at the frame's border is within 1e-4 px of zero, so p + f(p) there sits within the
    comparison bound of the frame edge and `valid` depends on the precision along the whole border."""
    rng = np.random.default_rng(seed)
    bg, obj = Texture(rng), Texture(rng)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    t, t_bg = np.asarray(t, np.float64), np.asarray(t_bg, np.float64)

    def inside(cx, cy):
        return ((xs - cx) / axes[0]) ** 2 + ((ys - cy) / axes[1]) ** 2 <= 1.
    mA, mB = inside(*centre), inside(centre[0] + t[0], centre[1] + t[1])
    A = np.where(mA[..., None], obj(xs - centre[0] + 200., ys - centre[1] + 100.), bg(xs, ys))
    B = np.where(mB[..., None], obj(xs - centre[0] - t[0] + 200., ys - centre[1] - t[1] + 100.), bg(xs - t_bg[0], ys - t_bg[1]))
    ab = np.where(mA[..., None], t[None, None], t_bg[None, None])
    ba = np.where(mB[..., None], -t[None, None], -t_bg[None, None])
    return Pair(name, quantise(A), quantise(B), ab.astype(np.float64), ba.astype(np.float64), mA, mB)


@functools.lru_cache(maxsize=None)
def fixture(name):
    """trans / big / affine / ellipse: 64 x 80 motion cases with a closed-form truth.  odd: 37 x 53, no multiple of anything.
    tiny: 9 x 7, one level, smaller than a solver tile.  seam: 33 x 65, one pixel past a 64 x 8 solver tile each way."""
    eye = np.eye(2)
    if name == 'trans':
        return _affine_pair(name, 64, 80, 21, eye, (3.3, -1.7))
    if name == 'big':
        return _affine_pair(name, 64, 80, 22, eye, (8.8, 3.9))                 # 0.11 W
    if name == 'affine':
        a, s = np.deg2rad(4.), 1.04
        return _affine_pair(name, 64, 80, 23, s * np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]), (0.6, -0.4))
    if name == 'ellipse':
        return _ellipse_pair(name, 64, 80, 24, (34., 33.), (15., 11.), (5.5, -2.25), (0.75, -0.5))
    if name == 'odd':
        return _affine_pair(name, 37, 53, 25, eye, (2.4, 1.3))
    if name == 'tiny':
        return _affine_pair(name, 9, 7, 26, eye, (0.6, -0.4))
    if name == 'seam':
        return _affine_pair(name, 33, 65, 27, eye, (-2.2, 1.6))
    raise KeyError(name)


FIXTURES = ('trans', 'big', 'affine', 'ellipse', 'odd', 'tiny', 'seam')
MOTION = ('trans', 'big', 'affine', 'ellipse')


def erode(mask, r):
    """The pixels whose (2r+1)^2 square lies inside the mask (outside the image counts as outside)."""
    m = np.pad(mask, r, constant_values=False)
    out = np.ones_like(mask)
    H, W = mask.shape
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out &= m[dy:dy + H, dx:dx + W]
    return out


def dilate(mask, r):
    """The pixels with a pixel of the mask in their (2r+1)^2 square."""
    m = np.pad(mask, r, constant_values=False)
    out = np.zeros_like(mask)
    H, W = mask.shape
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out |= m[dy:dy + H, dx:dx + W]
    return out


def score_region(pair):
    """The pixels a motion fixture's EPE is taken over: in-frame under the truth; for the two-layer case the object eroded by 3 px."""
    reg = pair.inframe(pair.truth_ab)
    if pair.maskA is not None:
        reg = reg & erode(pair.maskA, 3)
    return reg


@functools.lru_cache(maxsize=None)
def restated(name, dtype='float64'):
    """(flow [H,W,2], trace) of fixture `name` at the default parameters, computed once and shared; treat as read-only."""
    pair = fixture(name)
    trace = []
    f = flow(pair.imgA, pair.imgB, np.dtype(dtype).type, trace)
    return f, trace


@functools.lru_cache(maxsize=None)
def restated_back(name, dtype='float64'):
    pair = fixture(name)
    return flow(pair.imgB, pair.imgA, np.dtype(dtype).type)
