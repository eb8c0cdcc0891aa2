"""Restatement of the large-displacement matching stage of the variational flow (--vf_match; include/lasr_ops.h, DESIGN.md section
4.16) in plain numpy, and the fixtures tests/test_flowmatch_cpu.py and tests/test_flowmatch_gpu.py share.  Nothing here imports
the package or torch: the kernels of lasr_amd/csrc/flowmatch.hip and the passes of preprocess/flow_match.py are compared against
this file, not the other way round.

This file is the definition.  Everything up to `fuse` is integer arithmetic, so a kernel either gives these very numbers or is
wrong; no tolerance applies.  Displacements are (dx, dy) in pixels of the level the stage runs on, arrays [H,W,2] int32; a
quantised frame is [H,W] uint32, one word r | g << 8 | b << 16 per pixel.

  cost      C(p, d) = sum over q in [-r, r]^2 and the three channels of |A(clamp(p + q)) - B(clamp(p + q + d))|
  search    d*(p) = the minimum of the key (C, dx^2 + dy^2, dy, dx), in lexicographic order, over the d in [-R, R]^2 with p + d in the
            frame; c1 = C(p, d*)
  select    cu = clip(rint(uv), -R, R); ccur = C(p, cu), or (2r+1)^2 765 where p + cu leaves the frame; seeded where
            |d_ab(p) + d_ba(p + d_ab(p))|_inf <= 1 and 256 c1 < K ccur and |d_ab(p) - cu|_inf > 1, K = rint(256 kappa)
  propagate one Jacobi iteration: an unseeded pixel takes, from its left, right, upper, lower neighbour (in that order) that was
            seeded at the start of the iteration, the displacement d with p + d in the frame, 256 C(p, d) < K ccur and C(p, d)
            strictly below the best it holds so far (ccur to begin with), and is seeded from then on
  apply     uv <- d on seeded pixels; every other value passes through bit for bit
"""
import functools

import numpy as np

import robustflow_restated as rr
import varflow_restated as vr

DEFAULTS = dict(patch=2, level=-1, kappa=0.9, prop=16)      # r, L, kappa, N: derived on the dart fixtures below, not on footage
MAX_R, MAX_PATCH, MAX_PROP, LEVEL_SIDE = 32, 3, 64, 512


def check(R, patch=2, level=-1, kappa=0.9, prop=16):
    """-> (R, r, L, K, N) as integers; the limits the host refuses before any launch."""
    R, r, L, N = int(R), int(patch), int(level), int(prop)
    assert 1 <= R <= MAX_R and 1 <= r <= MAX_PATCH and 0 <= N <= MAX_PROP and L >= -1, (R, r, L, N)
    assert np.isfinite(kappa) and 0 < float(kappa) <= 1, kappa
    return R, r, L, int(np.rint(256. * float(kappa))), N


def pick_level(shapes, level=-1):
    """The level the stage runs on: `level` itself, or for -1 the finest of `shapes` (finest first) whose longer side is <=
    LEVEL_SIDE = 512, the coarsest when none is."""
    if level >= 0:
        assert level < len(shapes), (level, len(shapes))
        return int(level)
    for i, (h, w) in enumerate(shapes):
        if max(h, w) <= LEVEL_SIDE:
            return i
    return len(shapes) - 1


def max_cost(r):
    return (2 * r + 1) ** 2 * 765


def pack(rgb):
    """uint8 [H,W,3] -> uint32 [H,W]."""
    c = np.asarray(rgb).astype(np.uint32)
    return (c[..., 0] | (c[..., 1] << 8) | (c[..., 2] << 16)).astype(np.uint32)


def unpack(q):
    """uint32 [H,W] -> int32 [H,W,3]."""
    q = np.asarray(q, np.uint32)
    return np.stack([q & 255, (q >> 8) & 255, (q >> 16) & 255], -1).astype(np.int32)


def quantise(level):
    """Level 0: the uint8 frame itself; a coarser level in its working precision: clip(rint(255 I), 0, 255).  -> uint32 [H,W]."""
    level = np.asarray(level)
    if level.dtype == np.uint8:
        return pack(level)
    dt = level.dtype.type
    return pack(np.clip(np.rint(dt(255) * level), dt(0), dt(255)).astype(np.uint8))


def _box(D, r, H, W):
    """[H+2r, W+2r] -> [H, W]: the sum over each (2r+1)^2 window."""
    n = 2 * r + 1
    rows = sum(D[i:i + H] for i in range(n))
    return sum(rows[:, j:j + W] for j in range(n))


def search(qA, qB, R, r):
    """-> (d [H,W,2] int32 = (dx, dy), c1 [H,W] int32).  The displacements are visited in the order of (dx^2 + dy^2, dy, dx) and a
    later one wins only with a strictly smaller cost: the minimum of the key in lexicographic order."""
    A, B = unpack(qA), unpack(qB)
    H, W = A.shape[:2]
    Ae = np.pad(A, ((r, r), (r, r), (0, 0)), mode='edge')                        # A(clamp(s)) for s in [-r, H - 1 + r]
    Be = np.pad(B, ((r + R, r + R), (r + R, r + R), (0, 0)), mode='edge')        # B(clamp(s + d))
    ys, xs = np.mgrid[0:H, 0:W]
    best = np.full((H, W), np.iinfo(np.int32).max, np.int32)
    d = np.zeros((H, W, 2), np.int32)
    order = sorted(((dx * dx + dy * dy, dy, dx) for dy in range(-R, R + 1) for dx in range(-R, R + 1)))
    for _, dy, dx in order:
        Bs = Be[R + dy:R + dy + H + 2 * r, R + dx:R + dx + W + 2 * r]
        C = _box(np.abs(Ae - Bs).sum(-1), r, H, W).astype(np.int32)
        ok = (xs + dx >= 0) & (xs + dx < W) & (ys + dy >= 0) & (ys + dy < H) & (C < best)
        best = np.where(ok, C, best)
        d[ok] = (dx, dy)
    return d, best


def cost_at(qA, qB, d, r):
    """C(p, d(p)) for a displacement per pixel, d [H,W,2] int32 (wherever it points: the taps are clamped).  -> int32 [H,W]."""
    A, B = unpack(qA), unpack(qB)
    H, W = A.shape[:2]
    ys, xs = np.mgrid[0:H, 0:W]
    C = np.zeros((H, W), np.int32)
    for qy in range(-r, r + 1):
        for qx in range(-r, r + 1):
            a = A[np.clip(ys + qy, 0, H - 1), np.clip(xs + qx, 0, W - 1)]
            b = B[np.clip(ys + qy + d[..., 1], 0, H - 1), np.clip(xs + qx + d[..., 0], 0, W - 1)]
            C += np.abs(a - b).sum(-1).astype(np.int32)
    return C


def inframe(d):
    H, W = d.shape[:2]
    ys, xs = np.mgrid[0:H, 0:W]
    X, Y = xs + d[..., 0], ys + d[..., 1]
    return (X >= 0) & (X < W) & (Y >= 0) & (Y < H)


def select(qA, qB, d_ab, c1, d_ba, uv, R, r, K):
    """uv [2,H,W] (any float precision).  -> (seeded [H,W] uint8, cand [H,W,2] int32: d_ab where seeded, cu elsewhere,
    ccur [H,W] int32)."""
    H, W = c1.shape
    cu = np.clip(np.rint(np.asarray(uv)), -R, R).astype(np.int32)                # np.rint rounds half to even
    cu = np.stack([cu[0], cu[1]], -1)
    ccur = np.where(inframe(cu), cost_at(qA, qB, cu, r), max_cost(r)).astype(np.int32)
    ys, xs = np.mgrid[0:H, 0:W]
    back = d_ba[ys + d_ab[..., 1], xs + d_ab[..., 0]]                            # p + d_ab(p) is inside by construction
    consistent = np.abs(d_ab + back).max(-1) <= 1
    better = 256 * c1.astype(np.int64) < K * ccur.astype(np.int64)
    far = np.abs(d_ab - cu).max(-1) > 1
    seeded = consistent & better & far
    return seeded.astype(np.uint8), np.where(seeded[..., None], d_ab, cu).astype(np.int32), ccur


def propagate(qA, qB, seeded, cand, ccur, r, K):
    """One Jacobi iteration.  -> (seeded, cand) after it."""
    H, W = ccur.shape
    s_in, c_in = seeded.astype(bool), cand
    best = ccur.astype(np.int64).copy()
    out_s, out_c = s_in.copy(), cand.copy()
    for oy, ox in ((0, -1), (0, 1), (-1, 0), (1, 0)):                             # left, right, upper, lower
        ys, xs = np.mgrid[0:H, 0:W]
        ny, nx = ys + oy, xs + ox
        there = (ny >= 0) & (ny < H) & (nx >= 0) & (nx < W)
        ny, nx = np.clip(ny, 0, H - 1), np.clip(nx, 0, W - 1)
        d = c_in[ny, nx]
        C = cost_at(qA, qB, d, r).astype(np.int64)
        take = ~s_in & there & s_in[ny, nx] & inframe(d) & (256 * C < K * ccur.astype(np.int64)) & (C < best)
        best = np.where(take, C, best)
        out_c = np.where(take[..., None], d, out_c)
        out_s |= take
    return out_s.astype(np.uint8), out_c.astype(np.int32)


def apply(uv, seeded, cand):
    uv = np.asarray(uv)
    m = seeded.astype(bool)
    return np.stack([np.where(m, cand[..., 0].astype(uv.dtype), uv[0]), np.where(m, cand[..., 1].astype(uv.dtype), uv[1])])


def fuse(qA, qB, d_ab, c1, d_ba, uv, R, patch=2, kappa=0.9, prop=16, state=None):
    """Steps 5 to 7 on the flow uv [2,H,W] handed to the level.  -> uv.  state, a dict, receives seeded, cand and ccur."""
    R, r, _, K, N = check(R, patch, -1, kappa, prop)
    seeded, cand, ccur = select(qA, qB, d_ab, c1, d_ba, uv, R, r, K)
    for _ in range(N):
        seeded, cand = propagate(qA, qB, seeded, cand, ccur, r, K)
    if state is not None:
        state.update(seeded=seeded, cand=cand, ccur=ccur)
    return apply(uv, seeded, cand)


# ---- the whole flow ------------------------------------------------------------------------------------------------------------------

def flow_planar(imgA, imgB, init=None, dt=np.float64, gamma=0., beta=1., **over):
    """varflow_restated.flow_planar (gamma = 0) or robustflow_restated.flow_planar (gamma > 0) with the hook init(level, uv) -> uv,
    applied after `expand` and on the zero field of the coarsest level.  With init=None the very flows of those two files."""
    p = vr.params(**over)
    A, B = vr.pyramid(imgA, dt), vr.pyramid(imgB, dt)
    if gamma > 0:
        RA, RB = [rr.derivs(a, dt) for a in A], [rr.derivs(b, dt) for b in B]
    uv = np.zeros((2,) + A[-1].shape[:2], dt)
    for lev in range(len(A) - 1, -1, -1):
        h, w = A[lev].shape[:2]
        if lev != len(A) - 1:
            uv = vr.expand(uv, h, w, dt)
        if init is not None:
            uv = np.asarray(init(lev, uv)).astype(dt)
        for _ in range(int(p['NW'])):
            if gamma > 0:
                Jb, Jg = rr.tensor(RA[lev], RB[lev], uv, dt)
            else:
                J = vr.tensor(A[lev], B[lev], uv, dt)
            d = np.zeros_like(uv)
            for _ in range(int(p['NO'])):
                if gamma > 0:
                    J, psi = rr.weights(Jb, Jg, uv, d, p['eps'], beta, gamma, dt)
                else:
                    psi = vr.weights(J, uv, d, p['eps'], dt)
                d = vr.sor(J, psi, uv, d, p['alpha'], p['omega'], p['NI'], dt)
            uv = (uv + d).astype(dt)
    return uv


def matches(imgA, imgB, R, patch=2, level=-1, dt=np.float64):
    """-> (L, qA, qB, (d_ab, c_ab), (d_ba, c_ba)): the level, its two quantised frames and the two searches of a frame pair."""
    R, r, L, _, _ = check(R, patch, level)
    L = pick_level(vr.level_shapes(*np.asarray(imgA).shape[:2]), L)
    if L == 0:
        qA, qB = quantise(np.asarray(imgA)), quantise(np.asarray(imgB))
    else:
        qA, qB = quantise(vr.pyramid(imgA, dt)[L]), quantise(vr.pyramid(imgB, dt)[L])
    return L, qA, qB, search(qA, qB, R, r), search(qB, qA, R, r)


def flow_pair(imgA, imgB, match, dt=np.float64, gamma=0., beta=1., patch=2, level=-1, kappa=0.9, prop=16, **over):
    """-> (f_ab, f_ba), [H,W,2] in dt: both directions, sharing the two searches."""
    L, qA, qB, (d_ab, c_ab), (d_ba, c_ba) = matches(imgA, imgB, match, patch, level, dt)

    def hook(q1, q2, d12, c12, d21):
        return lambda lev, uv: fuse(q1, q2, d12, c12, d21, uv, match, patch, kappa, prop) if lev == L else uv
    f_ab = flow_planar(imgA, imgB, hook(qA, qB, d_ab, c_ab, d_ba), dt, gamma, beta, **over)
    f_ba = flow_planar(imgB, imgA, hook(qB, qA, d_ba, c_ba, d_ab), dt, gamma, beta, **over)
    return tuple(np.ascontiguousarray(np.moveaxis(f, 0, -1)) for f in (f_ab, f_ba))


# ---- fixtures ---------------------------------------------------------------------------------------------------------------------

DART = dict(H=96, W=128, centre=(40., 60.), axes=(7., 5.), t=(21.4, -8.3), t_bg=(0.75, -0.5))
DARTS = ('dart33', 'dart35')
MATCH_R = 24


@functools.lru_cache(maxsize=None)
def fixture(name):
    """dart33 / dart35: a small ellipse (semi-axes 7 x 5) that moves (21.4, -8.3) px over a background moving (0.75, -0.5) px, at
    96 x 128, seeds 33 and 35; every other name is varflow_restated's."""
    if name.startswith('dart'):
        return vr._ellipse_pair(name, DART['H'], DART['W'], int(name[4:]), DART['centre'], DART['axes'], DART['t'], DART['t_bg'])
    return vr.fixture(name)


def object_region(pair):
    """The object eroded by 2 px."""
    return vr.erode(pair.maskA, 2)


def background_region(pair):
    """Away from both silhouettes (dilated by 2 px) and a 4 px border."""
    reg = ~(vr.dilate(pair.maskA, 2) | vr.dilate(pair.maskB, 2))
    reg[:4], reg[-4:], reg[:, :4], reg[:, -4:] = False, False, False, False
    return reg


@functools.lru_cache(maxsize=None)
def plain(name, gamma=0.):
    """flow A -> B [H,W,2] float64 without the stage; read-only."""
    p = fixture(name)
    return np.ascontiguousarray(np.moveaxis(flow_planar(p.imgA, p.imgB, None, np.float64, gamma), 0, -1))


@functools.lru_cache(maxsize=None)
def matched(name, gamma=0.):
    """(f_ab, f_ba) float64 with the stage at R = MATCH_R and the default parameters; read-only."""
    p = fixture(name)
    return flow_pair(p.imgA, p.imgB, MATCH_R, np.float64, gamma)
