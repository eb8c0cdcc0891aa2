"""Float64 restatement of the silhouette propagation (include/lasr_ops.h) in numpy, and the analytic
fixtures tests/test_maskprop_cpu.py and tests/test_maskprop_gpu.py share.  Nothing here imports the package: the kernels of
lasr_amd/csrc/maskprop.hip and the passes of lasr_amd/nnutils/maskprop.py are compared against this file, not the other way round.

Every function takes the working precision `dt` (float64 by default); run in float32 it gives the spread the GPU tolerance is
derived from (test_maskprop_gpu.py's header).  Images are uint8 [H,W,3], soft masks [H,W], flows [H,W,2] = (x, y) in pixels.
"""
import functools

import numpy as np
from scipy import ndimage

BINS = 4096
DEFAULTS = dict(hi=0.9, lo=0.1, tau=1., w_p=1., w_a=0.5, eps=1e-3, U=6., R=4, sigma_i=12., sigma_s=3., w_s=0.3, K=5,
                min_component=0.05)


class EmptyPropagation(ValueError):
    pass


def params(**over):
    p = dict(DEFAULTS)
    unknown = set(over) - set(p)
    assert not unknown, unknown
    p.update(over)
    return p


def bins(img):
    i = img.astype(np.int64)
    return ((i[..., 0] >> 4) << 8) | ((i[..., 1] >> 4) << 4) | (i[..., 2] >> 4)


def window_of(P):
    """(x0, y0, x1, y1): the bounding box of P > 0.5 grown by half its width / height plus 8 px, clipped; None when empty."""
    ys, xs = np.nonzero(np.asarray(P) > 0.5)
    if xs.size == 0:
        return None
    H, W = P.shape
    w, h = int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)
    return (max(0, int(xs.min()) - w // 2 - 8), max(0, int(ys.min()) - h // 2 - 8),
            min(W, int(xs.max()) + 1 + w // 2 + 8), min(H, int(ys.max()) + 1 + h // 2 + 8))


def hist(img, P, window, hi=0.9, lo=0.1):
    """int64 [2, 4096]: row 1 counts the window's pixels with P >= hi, row 0 those with P <= lo.  The thresholds are compared in
    P's own precision (float32 soft masks against float32 thresholds, as the kernel does)."""
    out = np.zeros((2, BINS), np.int64)
    x0, y0, x1, y1 = window
    if x1 <= x0 or y1 <= y0:
        return out
    P = np.asarray(P)
    hi, lo = P.dtype.type(hi), P.dtype.type(lo)
    b, p = bins(img)[y0:y1, x0:x1], P[y0:y1, x0:x1]
    out[1] = np.bincount(b[p >= hi], minlength=BINS)
    out[0] = np.bincount(b[p <= lo], minlength=BINS)
    return out


def bilinear(f, qx, qy, dt):
    """f [H,W] sampled at (qx, qy) inside [0,W-1] x [0,H-1]; the upper taps are clamped to the image."""
    H, W = f.shape
    fx, fy = np.floor(qx), np.floor(qy)
    xa, ya = fx.astype(np.int64), fy.astype(np.int64)
    xb, yb = np.minimum(xa + 1, W - 1), np.minimum(ya + 1, H - 1)
    tx, ty = (qx - fx).astype(dt), (qy - fy).astype(dt)
    one = dt(1)
    return (f[ya, xa] * (one - tx) + f[ya, xb] * tx) * (one - ty) + (f[yb, xa] * (one - tx) + f[yb, xb] * tx) * ty


def sigmoid(x, dt):
    return (dt(1) / (dt(1) + np.exp(-x))).astype(dt)


def appearance(h, eps, dt):
    """app [4096] = log((hf/Nf + eps) / (hb/Nb + eps)); a total of 0 counts as 1."""
    Nb, Nf = dt(max(int(h[0].sum()), 1)), dt(max(int(h[1].sum()), 1))
    return np.log((h[1].astype(dt) / Nf + dt(eps)) / (h[0].astype(dt) / Nb + dt(eps))).astype(dt)


def unary(img_t, P_s, flow_ts, flow_st, h, p, dt=np.float64):
    """-> (u, q0, conf, prior), each [H,W] in dt."""
    H, W = P_s.shape
    P_s, flow_ts, flow_st = P_s.astype(dt), flow_ts[..., :2].astype(dt), flow_st[..., :2].astype(dt)
    ys, xs = np.mgrid[0:H, 0:W]
    fx, fy = flow_ts[..., 0], flow_ts[..., 1]
    qx, qy = xs.astype(dt) + fx, ys.astype(dt) + fy
    inside = (qx >= 0) & (qx <= W - 1) & (qy >= 0) & (qy <= H - 1)
    qxc, qyc = np.where(inside, qx, dt(0)), np.where(inside, qy, dt(0))
    prior = np.where(inside, bilinear(P_s, qxc, qyc, dt), dt(0)).astype(dt)
    ex = fx + bilinear(flow_st[..., 0], qxc, qyc, dt)
    ey = fy + bilinear(flow_st[..., 1], qxc, qyc, dt)
    inv = dt(1) / (dt(2) * dt(p['tau']) * dt(p['tau']))
    conf = np.where(inside, np.exp(-(ex * ex + ey * ey) * inv), dt(0)).astype(dt)
    app = appearance(h, p['eps'], dt)[bins(img_t)]
    pc = np.clip(prior, dt(1e-3), dt(1) - dt(1e-3))
    u = dt(p['w_p']) * conf * np.log(pc / (dt(1) - pc)) + dt(p['w_a']) * app
    u = np.clip(u, -dt(p['U']), dt(p['U'])).astype(dt)
    return u, sigmoid(u, dt), conf, prior


def meanfield(img, u, q, p, dt=np.float64):
    """One iteration: q'(p) = sigmoid(u(p) + w_s sum_n k(p,n) (2 q(n) - 1)) over the neighbours inside the image."""
    H, W = q.shape
    R = int(p['R'])
    I = img.astype(np.int64)
    s = (dt(2) * q.astype(dt) - dt(1))
    acc = np.zeros((H, W), dt)
    a, b = dt(1) / (dt(2) * dt(p['sigma_i']) ** 2), dt(1) / (dt(2) * dt(p['sigma_s']) ** 2)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            if dx == 0 and dy == 0:
                continue
            ya, yb, xa, xb = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)      # the pixels whose neighbour is inside
            if ya >= yb or xa >= xb:
                continue
            d = I[ya:yb, xa:xb] - I[ya + dy:yb + dy, xa + dx:xb + dx]
            k = np.exp(-((d * d).sum(-1).astype(dt) * a) - dt(dx * dx + dy * dy) * b)
            acc[ya:yb, xa:xb] += k * s[ya + dy:yb + dy, xa + dx:xb + dx]
    return sigmoid(u.astype(dt) + dt(p['w_s']) * acc, dt)


def component_filter(q, min_component):
    """q * (the 8-connected components of q > 0.5 whose area is at least min_component times the largest)."""
    lab, n = ndimage.label(q > 0.5, structure=np.ones((3, 3), int))
    if n == 0:
        return q * 0
    area = np.bincount(lab.ravel(), minlength=n + 1)
    area[0] = 0
    keep = area >= min_component * area.max()
    keep[0] = False
    return q * keep[lab]


def logit(q, dt=np.float64):
    q = np.clip(q.astype(dt), dt(1e-6), dt(1) - dt(1e-6))
    return np.log(q / (dt(1) - q))


def step(img_s, img_t, P_s, flow_ts, flow_st, key_hist, p, dt=np.float64, trace=None):
    """One propagation step s -> t.  -> q [H,W] before the component filter.  trace, a dict, receives the intermediate fields."""
    win = window_of(P_s)
    h = key_hist + hist(img_s, P_s.astype(dt), win, p['hi'], p['lo'])
    u, q, conf, prior = unary(img_t, P_s, flow_ts, flow_st, h, p, dt)
    qs = [q]
    for _ in range(int(p['K'])):
        q = meanfield(img_t, u, q, p, dt)
        qs.append(q)
    if trace is not None:
        trace.update(window=win, hist=h, u=u, conf=conf, prior=prior, q=qs)
    return q


def key_histogram(frames, key_masks, p, dt=np.float64):
    h = np.zeros((2, BINS), np.int64)
    for k, m in key_masks.items():
        P = np.asarray(m).astype(dt)
        h += hist(frames[k], P, window_of(P), p['hi'], p['lo'])
    return h


def chain(frames, flow_of, start, P0, stop, key_hist, p, dt=np.float64):
    """Propagate from frame `start` (soft mask P0) to frame `stop` inclusive, one step at a time.  flow_of(a, b) is the flow a -> b.
    -> {t: q before the filter}; the state carried on is the filtered q."""
    out, P, s = {}, P0, start
    d = 1 if stop > start else -1
    while s != stop:
        t = s + d
        q = step(frames[s], frames[t], P, flow_of(t, s), flow_of(s, t), key_hist, p, dt)
        P = component_filter(q, p['min_component'])
        if not (P > 0.5).any():
            raise EmptyPropagation('the propagated mask of frame %d is empty' % t)
        out[t] = q
        s = t
    return out


def propagate(frames, key_masks, flow_of, dt=np.float64, **over):
    """-> (masks [T,H,W] bool, soft [T,H,W]).  One key: a pass forward and a pass backward from it; several: a frame between the
    keys a < b is reached from both and the logits are averaged with weights (b-t)/(b-a) and (t-a)/(b-a) before the filter."""
    p = params(**over)
    T = len(frames)
    keys = sorted(key_masks)
    assert keys and 0 <= keys[0] and keys[-1] < T
    kh = key_histogram(frames, key_masks, p, dt)
    soft = np.zeros((T,) + frames[0].shape[:2], dt)
    for k in keys:
        soft[k] = np.asarray(key_masks[k]).astype(dt)
    for t, q in chain(frames, flow_of, keys[0], soft[keys[0]], 0, kh, p, dt).items():
        soft[t] = component_filter(q, p['min_component'])
    for t, q in chain(frames, flow_of, keys[-1], soft[keys[-1]], T - 1, kh, p, dt).items():
        soft[t] = component_filter(q, p['min_component'])
    for a, b in zip(keys[:-1], keys[1:]):
        if b - a < 2:
            continue
        fw = chain(frames, flow_of, a, soft[a], b - 1, kh, p, dt)
        bw = chain(frames, flow_of, b, soft[b], a + 1, kh, p, dt)
        for t in range(a + 1, b):
            wa, wb = dt(b - t) / dt(b - a), dt(t - a) / dt(b - a)
            q = sigmoid(wa * logit(fw[t], dt) + wb * logit(bw[t], dt), dt)
            soft[t] = component_filter(q, p['min_component'])
            if not (soft[t] > 0.5).any():
                raise EmptyPropagation('the propagated mask of frame %d is empty' % t)
    return soft > 0.5, soft


def roundtrip(frames, key, mask, flow_of, dt=np.float64, **over):
    """Forward from the key frame to the last frame, then back to the key frame: the IoU of what returns with the annotation."""
    p = params(**over)
    kh = key_histogram(frames, {key: mask}, p, dt)
    T = len(frames)
    P = np.asarray(mask).astype(dt)
    if key != T - 1:
        P = component_filter(chain(frames, flow_of, key, P, T - 1, kh, p, dt)[T - 1], p['min_component'])
        P = component_filter(chain(frames, flow_of, T - 1, P, key, kh, p, dt)[key], p['min_component'])
    return iou(P > 0.5, mask)


def iou(a, b):
    a, b = np.asarray(a) > 0, np.asarray(b) > 0
    return float((a & b).sum()) / max(float((a | b).sum()), 1.)


# ---- fixtures ---------------------------------------------------------------------------------------------------------------------

def smooth_noise(rng, shape, sigma, amp):
    f = ndimage.gaussian_filter(rng.standard_normal(shape), sigma, mode='wrap')
    return f * (amp / np.abs(f).max())


class Sequence:
    """A textured ellipse that translates and stretches over a textured static background.  The object point at (a_s cos, b_s sin)
    about c_s in frame s sits at (a_t cos, b_t sin) about c_t in frame t, so the flow s -> t is closed form: inside the ellipse of s
    (x - c_s) * (axes_t / axes_s) + c_t - x, outside 0.  flow_noise adds a smooth field of that amplitude (px) to every flow,
    another one per ordered pair; distractor paints a patch of the object's colours into the background."""

    def __init__(self, H, W, T, c0, vel, axes0, grow, seed, flow_noise=0., distractor=None):
        rng = np.random.default_rng(seed)
        self.H, self.W, self.T = H, W, T
        self.c = [np.array(c0, float) + t * np.array(vel, float) for t in range(T)]
        self.axes = [np.array(axes0, float) * (1 + t * np.array(grow, float)) for t in range(T)]
        obj_base, bg_base = np.array([200., 80., 60.]), np.array([60., 120., 170.])
        tex = np.stack([smooth_noise(rng, (64, 64), 5, 25) for _ in range(3)], -1) + obj_base      # canonical [-1.05, 1.05]^2
        bg = np.stack([smooth_noise(rng, (H, W), 4, 25) for _ in range(3)], -1) + bg_base
        ys, xs = np.mgrid[0:H, 0:W].astype(float)
        if distractor is not None:
            x0, y0, x1, y1 = distractor
            patch = np.stack([smooth_noise(rng, (H, W), 4, 25) for _ in range(3)], -1) + obj_base
            bg[y0:y1, x0:x1] = patch[y0:y1, x0:x1]
        self.frames, self.masks = [], []
        for t in range(T):
            nx, ny = (xs - self.c[t][0]) / self.axes[t][0], (ys - self.c[t][1]) / self.axes[t][1]
            inside = nx * nx + ny * ny <= 1
            coords = [(np.clip(ny, -1.05, 1.05) / 2.1 + 0.5) * 63, (np.clip(nx, -1.05, 1.05) / 2.1 + 0.5) * 63]
            obj = np.stack([ndimage.map_coordinates(tex[..., ch], coords, order=1) for ch in range(3)], -1)
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
                        self._noise[(s, t)] = np.stack([smooth_noise(rng, (H, W), 8, flow_noise) for _ in range(2)], -1)
        self._index = {f.tobytes(): i for i, f in enumerate(self.frames)}

    def flow(self, s, t):
        """float32 [H,W,2]: the flow s -> t on the grid of s."""
        r = self.axes[t] / self.axes[s]
        fx = (self._xs - self.c[s][0]) * r[0] + self.c[t][0] - self._xs
        fy = (self._ys - self.c[s][1]) * r[1] + self.c[t][1] - self._ys
        f = np.stack([fx, fy], -1) * self.masks[s][..., None]
        if (s, t) in self._noise:
            f = f + self._noise[(s, t)]
        return f.astype(np.float32)

    def flow_fn(self, imgA, imgB):
        """The signature of auto_gen.run's flow_fn: frames are recognised by their content.  -> (flow [H,W,3], occ [H,W])."""
        f = self.flow(self._index[np.ascontiguousarray(imgA).tobytes()], self._index[np.ascontiguousarray(imgB).tobytes()])
        return np.concatenate([f, np.ones(f.shape[:2] + (1,), np.float32)], -1), np.zeros(f.shape[:2], np.float32)


@functools.lru_cache(maxsize=None)
def fixture(name):
    """ellipse / ellipse_noisy / ellipse_distractor: 64 x 80, 8 frames.  odd: 37 x 53, tile edges and the halo are cut.
    tiny: 9 x 7, smaller than one tile and than the window radius.  border: the object leaves the frame partly, so that with the
    key on the last frame q = p + flow falls outside the image."""
    if name == 'ellipse':
        return Sequence(64, 80, 8, (24, 28), (4.5, 1.0), (11, 15), (0.05, -0.025), seed=7)
    if name == 'ellipse_noisy':
        return Sequence(64, 80, 8, (24, 28), (4.5, 1.0), (11, 15), (0.05, -0.025), seed=7, flow_noise=6.)
    if name == 'ellipse_distractor':
        return Sequence(64, 80, 8, (24, 28), (4.5, 1.0), (11, 15), (0.05, -0.025), seed=7, distractor=(50, 44, 62, 56))
    if name == 'odd':
        return Sequence(37, 53, 3, (20, 17), (4.0, 1.5), (9, 11), (0.05, -0.03), seed=11, flow_noise=1.)
    if name == 'tiny':
        return Sequence(9, 7, 2, (3, 4), (1.0, 0.5), (2.2, 2.8), (0.0, 0.0), seed=13)
    if name == 'border':
        return Sequence(48, 64, 5, (22, 24), (-4.0, 0.5), (12, 14), (0.0, 0.0), seed=17)
    raise KeyError(name)


FIXTURES = ('ellipse', 'odd', 'tiny', 'border')
# the key frame(s) the tests propagate each fixture from
KEYS = {'ellipse': 0, 'ellipse_noisy': 0, 'ellipse_distractor': 0, 'odd': 0, 'tiny': 0, 'border': 4}


def first_step(name):
    """The inputs of the one step the kernel comparisons run on a fixture: from its key frame s to the neighbour t.
    -> dict(img_s, img_t, P_s float32, flow_ts, flow_st, key_hist)."""
    seq = fixture(name)
    s = KEYS[name]
    t = s + 1 if s + 1 < seq.T else s - 1
    P = seq.masks[s].astype(np.float32)
    return dict(img_s=seq.frames[s], img_t=seq.frames[t], P_s=P, flow_ts=seq.flow(t, s), flow_st=seq.flow(s, t),
                key_hist=key_histogram(seq.frames, {s: seq.masks[s]}, params()))
