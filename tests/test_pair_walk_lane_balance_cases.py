"""The scenes of tests/test_pair_walk_lane_balance_gpu.py, looked at on the CPU with the oracle alone: a scene that renders only
background, or whose pixels meet at most one fragment each, would prove nothing about the order in which fragments fold.  Every
case but the two that are about exactly that ('one face', 'empty mesh') must have a pixel with more than one fragment (a face the
pixel lies inside of, or within the distance threshold of) and an image that is neither background nor constant."""
import math

import numpy as np
import pytest

from lasr_amd import synth
from test_pair_walk_lane_balance_gpu import CASES, background, oracle_image


def fragments_per_pixel(fv, IS):
    """[N, IS, IS] counts of the faces each pixel centre lies inside of or closer to than the threshold (float64, no culling)."""
    m = synth.LASR_MODES
    thr = math.log(1. / m['dist_eps'] - 1.) * m['sigma_val']
    c = (2 * np.arange(IS) + 1 - IS) / IS
    X, Y = np.meshgrid(c, c[::-1])
    cnt = np.zeros((fv.shape[0], IS, IS), np.int64)
    for n in range(fv.shape[0]):
        for t in fv[n].astype(np.float64):
            a, b, d = t[0, :2], t[1, :2], t[2, :2]
            best = np.full((IS, IS), np.inf)
            sign = []
            for p, q in ((a, b), (b, d), (d, a)):
                e = q - p
                s = np.clip(((X - p[0]) * e[0] + (Y - p[1]) * e[1]) / max(e @ e, 1e-300), 0, 1)
                best = np.minimum(best, (p[0] + s * e[0] - X) ** 2 + (p[1] + s * e[1] - Y) ** 2)
                sign.append(e[0] * (Y - p[1]) - e[1] * (X - p[0]))
            inside = ((sign[0] > 0) & (sign[1] > 0) & (sign[2] > 0)) | ((sign[0] < 0) & (sign[1] < 0) & (sign[2] < 0))
            cnt[n] += inside | (best < thr)
    return cnt


@pytest.mark.parametrize('name', list(CASES))
def test_the_scene_has_fragments_to_fold(oracle, name):
    build, IS = CASES[name]
    fv, ft, near, far = build()
    img = oracle_image(oracle, name)
    C = ft.shape[-1]
    assert img.shape == (fv.shape[0], C + 1, IS, IS) and np.isfinite(img).all()
    cnt = fragments_per_pixel(fv, IS)
    if name == 'empty mesh':
        assert cnt.max() == 0 and not img[:, C].any()
        return
    bg = np.asarray(background(C), np.float32)[None, :, None, None]
    assert img[:, C].max() > 1e-2 and img[:, C].min() < 0.5                     # alpha: something drawn, something left free
    assert (np.abs(img[:, :C] - bg).max(1) > 1e-3).sum() >= 4
    assert cnt.max() == 1 if name == 'one face' else cnt.max() > 1, cnt.max()
    if name.startswith('stack'):
        # 70 fragments per covered pixel; the whole stack covers columns 0..7 and nothing right of them, the sliver column 7 only
        cols = np.nonzero(cnt[0].max(0))[0]
        assert cnt.max() == 70 and list(cols) == ([7] if 'sliver' in name else list(range(8)))
