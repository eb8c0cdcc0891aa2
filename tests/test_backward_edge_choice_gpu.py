"""The backward raster's edge choice, pixel by pixel: for well-conditioned faces the LASR-mode backward (sr_backward_kernel<true, NCH>)
reads the edge an outside pixel projects to from a 2-bit table, tests the obtuse corner once on prepared operands and runs one
projection on the lane's own edge block (sr_device.h: euclid_one_ext).  A wrong edge for ONE pixel changes that pixel's displacement
(dx, dy) and with it the face gradient it contributes, but drowns in the sum over a dense upstream gradient -- so here the upstream
gradient is one-hot per frame: frame b carries its only non-zero values at probe pixel b, and every frame is compared with the
oracle on its own, at the project's gradient bar (GRAD_REL of tests/test_raster_parity_gpu.py: 1e-3 of the frame's largest gradient).

Scenes (32 x 32, sigma_val 7e-3: the distance threshold log(1 / dist_eps - 1) sigma = 0.0645 is a band of 0.25 NDC = 4 pixels):
  acute ccw / acute cw   one isosceles face whose axis runs 2e-4 NDC beside a pixel column, both windings: the inside pixels of that
                         column are 0.1-0.4 % nearer to one slanted edge than to the other -- inside the 1.5 % near-tie margin, so
                         they take the three-projection path, and far outside fp32 rounding (1e-6), so the nearer edge is the same in
                         every arithmetic (ON the bisector the reference's own rounding picks the edge, and a build that rounds
                         differently may rightly pick the other: the direction of the pixel's contribution flips)
  obtuse 0 / 1 / 2       the obtuse corner at vertex 0, 1, 2: a pair of faces, the same triangle in both windings
  sliver                 a face without record flag 16 (height 0.005 NDC: the generic path) next to a well-conditioned one
tests/test_backward_edge_choice_cases.py classifies every probe in numpy and asserts that the set covers every case of the choice.

The upstream values: a pixel's contribution is C = (alpha term) + (colour term), the colour term being sum_k g_k (c_face,k - c_pixel,k)
times positive factors.  The attributes lie in [0.1, 0.6] under a background of 1, so c_face - c_pixel <= 0 at every probe; with
g_k > 0 the colour term is negative, and g_alpha = -1 makes the alpha term negative as well.  The two terms then add up instead of
cancelling, the frame's gradient is as well conditioned as its terms (fp32 rounding of the oracle, v_rcp / v_exp in the kernel:
1e-6 .. 1e-5 relative), and what 1e-3 of the frame's largest gradient measures is the geometry: the edge, the clamp, the sign.
"""
import functools
import math

import numpy as np
import pytest

import raster_harness as rh
from lasr_amd import synth
from raster_harness import GRAD_REL, rot as _rot, tri as _tri

IS = 32
SIGMA = 7e-3
NEAR, FAR = 1.0, 5.0
MAX_FRAMES = 64
NEAR_TIE, NEAR_TIE_ABS = 0.985, 2.4e-6      # sr_device.h
# A pixel is a probe for a face it lies inside of, or outside of at a squared distance below STRONG x threshold: D = sigmoid(-d^2 / sigma)
# is then at least e^-4.6 = 1e-2.  In the outer half of the band D falls to 1e-4 and the frame's whole gradient with it, while the
# forward image the backward reads back (1 - alpha, colour - pixel colour) keeps its fp32 absolute error of 6e-8: the fp32 oracle
# itself is then only good to 2e-4 .. 1.6e-3 of the frame's largest gradient against its own float64 run, which is the bar.  With
# STRONG = 0.5 most frames are resolved to 1e-5; probes() drops the few that the oracle's two precisions still do not agree on.
STRONG = 0.5


def _rev(t):
    return [t[0], t[2], t[1]]


_AX = 1. / 32 + 2e-4                            # 2e-4 beside a pixel-centre column
_ACUTE = _tri([(-0.5 + _AX, -0.4), (0.5 + _AX, -0.4), (_AX, 0.55)])
_OBT = _tri(rh.OBTUSE)                                             # obtuse at its FIRST vertex
_SLIVER = _tri([(-0.6, 0.6), (0.6, 0.604), (0.0, 0.607)], (3.2, 3.3, 3.4))


def _shift(t, dx, dy):
    return [[x + dx, y + dy, z + 0.2] for x, y, z in t]


SCENES = {
    'acute ccw': [_ACUTE],
    'acute cw': [_rev(_ACUTE)],
    'obtuse 0': [_rot(_OBT, 0), _shift(_rev(_rot(_OBT, 0)), -0.05, -0.3)],
    'obtuse 1': [_rot(_OBT, 1), _shift(_rev(_rot(_OBT, 2)), -0.05, -0.3)],      # (reversing keeps vertex 0 and swaps 1 <-> 2)
    'obtuse 2': [_rot(_OBT, 2), _shift(_rev(_rot(_OBT, 1)), -0.05, -0.3)],
    'sliver': [_SLIVER, _shift(_ACUTE, 0.1, -0.2)],
}
DENSE = [_ACUTE, _shift(_rev(_OBT), 0.1, 0.2), _rot(_OBT, 1), _shift(_rot(_ACUTE, 2), -0.2, 0.1)]


def scene_faces(name):
    return np.asarray(SCENES[name], np.float32)          # [F, 3, 3]


def threshold():
    m = synth.LASR_MODES
    return math.log(1. / m['dist_eps'] - 1.) * SIGMA


def pixel_centres():
    c = (2 * np.arange(IS) + 1 - IS) / IS
    return np.meshgrid(c, c[::-1])                       # X, Y of [row from the top, column]


def classify(tri):
    """Per pixel of the IS x IS image, the case of the backward's edge choice for face `tri` ([3, 3], float64 arithmetic on the
    fp32 vertices): dict of [IS, IS] arrays -- reach (inside, or nearer than the threshold: stage 2 computes a gradient), well
    (record flag 16), inside, tie, k_in (nearest edge line of an inside pixel), idx = n0 + 2 n1 + 4 n2, over, obtuse (corner or -1)."""
    t = np.asarray(tri, np.float64)
    x, y = t[:, 0], t[:, 1]
    X, Y = pixel_centres()
    det = x[2] * (y[0] - y[1]) + x[0] * (y[1] - y[2]) + x[1] * (y[2] - y[0])
    adj = np.array([[y[1] - y[2], x[2] - x[1], x[1] * y[2] - x[2] * y[1]],
                    [y[2] - y[0], x[0] - x[2], x[2] * y[0] - x[0] * y[2]],
                    [y[0] - y[1], x[1] - x[0], x[0] * y[1] - x[1] * y[0]]]) / det
    w = [adj[k, 0] * X + adj[k, 1] * Y + adj[k, 2] for k in range(3)]
    obtuse = -1
    for k in range(3):
        b, c = (k + 1) % 3, (k + 2) % 3
        if obtuse < 0 and (x[b] - x[k]) * (x[c] - x[k]) + (y[b] - y[k]) * (y[c] - y[k]) < 0:
            obtuse = k
    hk2, well = [], True
    for k in range(3):
        b, c = (k + 1) % 3, (k + 2) % 3
        l2 = (x[c] - x[b]) ** 2 + (y[c] - y[b]) ** 2
        hk2.append(det * det / l2)
        well = well and 1e-4 < hk2[-1] < 1e4 and l2 < 16.
    inside = (np.minimum(np.minimum(w[0], w[1]), w[2]) > 0) & (np.maximum(np.maximum(w[0], w[1]), w[2]) < 1)
    q = np.stack([w[2] ** 2 * hk2[2], w[0] ** 2 * hk2[0], w[1] ** 2 * hk2[1]])        # edge 0, 1, 2
    qs = np.sort(q, 0)
    scale = 4. * NEAR_TIE_ABS ** 2 / min(hk2)
    tie = inside & (~(qs[0] < NEAR_TIE * qs[1]) | ~((qs[1] - qs[0]) ** 2 > scale * qs[1]))
    idx = (w[0] <= 0) * 1 + (w[1] <= 0) * 2 + (w[2] <= 0) * 4
    over = np.zeros_like(inside)
    if obtuse >= 0:
        c, o = obtuse, (obtuse + 2) % 3
        over = (X - x[c]) * (x[o] - x[c]) + (Y - y[c]) * (y[o] - y[c]) > 0
    # squared distance to the triangle's boundary
    d2 = np.full(X.shape, np.inf)
    for k in range(3):
        b = (k + 1) % 3
        ex, ey = x[b] - x[k], y[b] - y[k]
        s = np.clip(((X - x[k]) * ex + (Y - y[k]) * ey) / (ex * ex + ey * ey), 0, 1)
        d2 = np.minimum(d2, (x[k] + s * ex - X) ** 2 + (y[k] + s * ey - Y) ** 2)
    return dict(reach=inside | (d2 < threshold()), strong=inside | (d2 < STRONG * threshold()), well=well, inside=inside, tie=tie, k_in=np.argmin(q, 0), idx=idx, over=over,
                obtuse=obtuse)


PAIR_OF = {6: 'n1 n2', 5: 'n2 n0', 3: 'n0 n1'}            # idx of a two-negative sign pattern -> its name
CORNER_OF = {6: 0, 5: 1, 3: 2}                           # ... and the corner whose obtuse override applies to it


def case_of(c, r, col):
    """Name of the case pixel (r, col) is for a face classified as `c`; None when the pixel is no probe for this face (see STRONG)."""
    if not c['strong'][r, col]:
        return None
    if not c['well']:
        return 'generic path (no flag 16)'
    if c['inside'][r, col]:
        return 'inside, near tie' if c['tie'][r, col] else 'inside, edge %d' % c['k_in'][r, col]
    i = int(c['idx'][r, col])
    if i in (1, 2, 4):
        return 'outside, only n%d' % {1: 0, 2: 1, 4: 2}[i]
    if i in PAIR_OF:
        if c['obtuse'] == CORNER_OF[i]:
            return 'outside, %s, %s the obtuse corner' % (PAIR_OF[i], 'beyond' if c['over'][r, col] else 'not beyond')
        return 'outside, %s' % PAIR_OF[i]
    return 'outside, idx %d' % i


def oracle_spread(name, P, nch):
    """Per probe frame of P: the fp32 oracle against its own float64 run, as a fraction of the frame's largest gradient."""
    from oracle import sr_oracle
    faces = scene_faces(name)
    fv = np.ascontiguousarray(np.broadcast_to(faces[None], (len(P),) + faces.shape))
    ft = np.ascontiguousarray(np.broadcast_to(textures(len(faces), nch, 5)[None], (len(P), len(faces), 3, nch)))
    g = one_hot_grad_of(P, nch)
    lo = oracle_grads(sr_oracle, fv, ft, g, nch)
    hi = oracle_grads(sr_oracle, fv.astype(np.float64), ft.astype(np.float64), g.astype(np.float64), nch, dtype=np.float64)
    return [max(float(np.abs(a[n] - b[n]).max() / max(np.abs(b[n]).max(), 1e-300)) for a, b in zip(lo, hi)) for n in range(len(P))]


ORACLE_SPREAD = 1e-4        # a tenth of the bar


@functools.lru_cache(maxsize=None)
def probes(name):
    """Up to MAX_FRAMES probe pixels (row, col) of the scene: for every face, pixels of each case it shows, spread over the case's
    pixels, the rare cases first.  A pixel is only taken when the reference resolves its frame: the fp32 oracle within ORACLE_SPREAD
    of its float64 run at three and at nine channels (the reference's own error, nothing of the kernel under test)."""
    per_case = {}
    for f, tri in enumerate(scene_faces(name)):
        c = classify(tri)
        for r in range(IS):
            for col in range(IS):
                k = case_of(c, r, col)
                if k is not None:
                    per_case.setdefault((f, k), []).append((r, col))
    quota = max(1, MAX_FRAMES // max(len(per_case), 1))
    cand = []
    for key in sorted(per_case, key=lambda k: len(per_case[k])):
        px = per_case[key]
        step = max(1, len(px) // (3 * quota))
        cand.append([p for p in px[::step][:3 * quota]])
    flat = sorted(set(p for c in cand for p in c))
    ok = {p for p, s3, s9 in zip(flat, oracle_spread(name, flat, 3), oracle_spread(name, flat, 9)) if max(s3, s9) <= ORACLE_SPREAD}
    chosen, seen = [], set()
    for c in cand:
        n = 0
        for p in c:
            if p in ok and p not in seen and n < quota and len(chosen) < MAX_FRAMES:
                seen.add(p)
                chosen.append(p)
                n += 1
    return tuple(chosen)


def one_hot_grad_of(P, nch):
    g = np.zeros((len(P), nch + 1, IS, IS), np.float32)
    for b, (r, col) in enumerate(P):
        g[b, :nch, r, col] = 0.5 + 0.25 * np.arange(nch)
        g[b, nch, r, col] = -1.0
    return g


def one_hot_grad(name, nch):
    return one_hot_grad_of(probes(name), nch)


def textures(F, nch, seed):
    return np.random.default_rng(seed).uniform(0.1, 0.6, (F, 3, nch)).astype(np.float32)


KW = dict(synth.LASR_MODES, near=NEAR, far=FAR, sigma_val=SIGMA)


def oracle_grads(oracle, fv, ft, g, nch, dtype=np.float32):
    """Reference gradients of an nch-channel pass (probes() and oracle_spread() call it anew for every set of frames: not cached)."""
    return rh.oracle_reference(oracle, fv, ft, IS, None, KW, g=g, dtype=dtype)[1:]


def hip_grads(dev, fv, ft, g, nch):
    return rh.render(dev, (fv, ft, NEAR, FAR), IS, [1.] * nch if nch == 9 else None, grad=g, sigma_val=SIGMA)[1:]


def check_per_frame(a, b, what):
    for n in range(a.shape[0]):
        scale = float(np.abs(b[n]).max())
        d = float(np.abs(a[n] - b[n]).max())
        assert np.isfinite(a[n]).all() and d <= GRAD_REL * scale, '%s, frame %d: max diff %.3e vs largest gradient %.3e' % (what, n, d, scale)


@pytest.mark.gpu
@pytest.mark.parametrize('nch', [3, 6, 9])
@pytest.mark.parametrize('name', list(SCENES))
def test_one_hot_gradient_per_probe_pixel(oracle, cuda, name, nch):
    faces = scene_faces(name)
    P = probes(name)
    assert 0 < len(P) <= MAX_FRAMES
    fv = np.ascontiguousarray(np.broadcast_to(faces[None], (len(P),) + faces.shape))
    ft = np.ascontiguousarray(np.broadcast_to(textures(len(faces), nch, 5)[None], (len(P), len(faces), 3, nch)))
    g = one_hot_grad(name, nch)
    gf_ref, gt_ref = oracle_grads(oracle, fv, ft, g, nch)
    gf, gt = hip_grads(cuda, fv, ft, g, nch)
    assert min(float(np.abs(gf_ref[n]).max()) for n in range(len(P))) > 0           # every probe reaches a face
    check_per_frame(gf, gf_ref, 'grad_faces')
    check_per_frame(gt, gt_ref, 'grad_textures')


@pytest.mark.gpu
@pytest.mark.parametrize('nch', [3, 6, 9])
def test_dense_gradient_four_faces(oracle, cuda, nch):
    faces = np.asarray(DENSE, np.float32)
    fv = np.ascontiguousarray(np.broadcast_to(faces[None], (2,) + faces.shape)).copy()
    fv[1, :, :, 0] += 0.03                                                             # the second frame: the faces moved a little
    ft = np.stack([textures(4, nch, 6), textures(4, nch, 7)])
    g = np.random.default_rng(8).standard_normal((2, nch + 1, IS, IS)).astype(np.float32)
    gf_ref, gt_ref = oracle_grads(oracle, fv, ft, g, nch)
    gf, gt = hip_grads(cuda, fv, ft, g, nch)
    check_per_frame(gf, gf_ref, 'grad_faces')
    check_per_frame(gt, gt_ref, 'grad_textures')
