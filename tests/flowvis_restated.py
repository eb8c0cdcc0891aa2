"""Numpy restatement of lasr_amd/csrc/flowvis.hip: the Middlebury colour coding, the epoch contact sheet
and the scalar ring.  Every function takes the dtype it computes in: float64 is the definition (and equals the reference's
flowlib.flow_to_image bit for bit on the fixture tests/golden/flowvis.npz), float32 follows the kernel's operation order and is
what the exact panels of the sheet are compared with.  Test infrastructure: the product has no CPU path."""
import numpy as np

NCOLS = 55
UNKNOWN = 1e7


def color_wheel():
    """[55,3] Middlebury wheel: six ramps of floor(255 i / n)."""
    wheel, col = np.zeros((NCOLS, 3)), 0
    for n, fixed, ramp, up in ((15, 0, 1, True), (6, 1, 0, False), (4, 1, 2, True), (11, 2, 1, False), (13, 2, 0, True),
                               (6, 0, 2, False)):
        r = np.floor(255 * np.arange(n) / n)
        wheel[col:col + n, fixed] = 255
        wheel[col:col + n, ramp] = r if up else 255 - r
        col += n
    return wheel


def _samples(u, v, mask, dt):
    u, v = np.array(u, dt), np.array(v, dt)
    if mask is not None:
        off = np.asarray(mask) == 0
        u[off] = 0
        v[off] = 0
    with np.errstate(invalid='ignore'):
        dark = (np.abs(u) > UNKNOWN) | (np.abs(v) > UNKNOWN) | np.isnan(u) | np.isnan(v)
    u[dark] = 0
    v[dark] = 0
    return u, v, dark


def max_radius(u, v, mask=None, dt=np.float64):
    u, v, _ = _samples(u, v, mask, dt)
    return np.sqrt(u * u + v * v).max() if u.size else dt(0)


def colour_code(u, v, mask=None, dt=np.float64):
    """One image: u, v [H,W] -> (uint8 [H,W,3], normalised radius [H,W])."""
    u, v, dark = _samples(u, v, mask, dt)
    maxrad = np.sqrt(u * u + v * v).max()
    den = dt(maxrad + dt(np.finfo(float).eps))
    u, v = u / den, v / den
    rad = np.sqrt(u * u + v * v)
    a = np.arctan2(-v, -u) / dt(np.pi)
    fk = (a + dt(1)) / dt(2) * dt(NCOLS - 1) + dt(1)
    k0 = np.clip(np.floor(fk).astype(int), 1, NCOLS)
    k1 = np.where(k0 == NCOLS, 1, k0 + 1)
    f = fk - k0.astype(dt)
    wheel = color_wheel().astype(dt)
    img = np.zeros(u.shape + (3,), np.uint8)
    for c in range(3):
        col0, col1 = wheel[k0 - 1, c] / dt(255), wheel[k1 - 1, c] / dt(255)
        col = (dt(1) - f) * col0 + f * col1
        col = np.where(rad <= 1, dt(1) - rad * (dt(1) - col), col * dt(0.75))
        img[..., c] = np.clip(np.floor(dt(255) * col), 0, 255).astype(np.uint8)
    img[dark] = 0
    return img, rad


def flow_to_image(flow, mask=None, dt=np.float64):
    """flow [B,H,W,C] -> (uint8 [B,H,W,3], normalised radii [B,H,W]); every image by its own maximum."""
    flow = np.asarray(flow)
    out = np.zeros(flow.shape[:3] + (3,), np.uint8)
    rad = np.zeros(flow.shape[:3])
    for b in range(flow.shape[0]):
        if flow[b].size:
            out[b], rad[b] = colour_code(flow[b, ..., 0], flow[b, ..., 1], None if mask is None else mask[b], dt)
    return out, rad


def level(x):
    with np.errstate(invalid='ignore'):
        return np.where(np.isnan(x), 0, np.clip(np.floor(x), 0, 255)).astype(np.uint8)


def minmax_grey(x, dt):
    x = np.asarray(x, dt)
    ok = ~np.isnan(x)
    out = np.zeros(x.shape, np.uint8)
    if ok.any() and x[ok].max() > x[ok].min():
        lo, hi = x[ok].min(), x[ok].max()
        out = level(dt(255) * (x - lo) / (hi - lo))
    return np.repeat(out[..., None], 3, -1)


def ring_mask(IS, cx, cy, dt):
    """Pixels (row r, column c) with 1.5^2 <= (c - cx)^2 + (r - cy)^2 <= 4.5^2."""
    half = dt(0.5) * dt(IS)
    px, py = half + half * dt(cx), half + half * dt(cy)
    r, c = np.mgrid[:IS, :IS]
    dx, dy = c.astype(dt) - px, r.astype(dt) - py
    d2 = dx * dx + dy * dy
    with np.errstate(invalid='ignore'):
        return (d2 >= dt(2.25)) & (d2 <= dt(20.25))


def sheet(p, IS, dt=np.float64):
    """p: flow_obs, flow_rd [2,IS,IS] (u, v planes), vis_mask, flow_err, mask_pred, mask_gt [IS,IS], part [3,IS,IS] or None, img1,
    img2, texture [3,IS,IS], ctl [n,>=2] or None, palette [n,3] -> (uint8 [3 IS, 3 IS, 3], radii of the two flow panels)."""
    m = np.asarray(p['vis_mask'], dt)
    obs, r_obs = colour_code(p['flow_obs'][0], p['flow_obs'][1], m, dt)
    rd, r_rd = colour_code(p['flow_rd'][0], p['flow_rd'][1], m, dt)

    def rgb(x):
        return level(dt(255) * np.asarray(x, dt)).transpose(1, 2, 0)
    tex = rgb(p['texture']).copy()
    if p.get('ctl') is not None:
        for k in range(len(p['ctl'])):
            tex[ring_mask(IS, p['ctl'][k][0], p['ctl'][k][1], dt)] = level(np.asarray(p['palette'][k], dt))
    tiles = [obs, rd, minmax_grey(np.asarray(p['flow_err'], dt) * m, dt), minmax_grey(p['mask_pred'], dt), minmax_grey(p['mask_gt'], dt),
             rgb(p['part']) if p.get('part') is not None else np.zeros((IS, IS, 3), np.uint8), rgb(p['img1']), rgb(p['img2']), tex]
    out = np.concatenate([np.concatenate(tiles[3 * i:3 * i + 3], 1) for i in range(3)], 0)
    return out, (r_obs, r_rd)


def ring(pushes, capacity):
    """pushes: list of lists of arrays -> (ring [capacity,K] of float64 means, head)."""
    K = len(pushes[0])
    out = np.zeros((capacity, K))
    for n, vals in enumerate(pushes):
        out[n % capacity] = [np.asarray(v, np.float64).mean() if v is not None and np.size(v) else np.nan for v in vals]
    return out, len(pushes)
