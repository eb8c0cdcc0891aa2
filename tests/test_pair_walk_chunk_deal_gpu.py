"""The pair-walk forward kernel (lasr_amd/csrc/sr_forward_pairs.h) DEALS a tile's face list round-robin over its chunks: a round of
`count` entries makes nch = ceil(count / 64) chunks, chunk c holds the list positions c, c + nch, c + 2 nch, ... (chunk_count,
chunk_size, chunk_pos in the header; tests/test_pair_walk_chunk_deal_cases.py restates them).  Chunks are then partial whenever
count is no multiple of 64 -- 65 entries are 33 + 32 -- so lanes ride along on slot 63 of a staging buffer that no chunk of the
workgroup has written, and a pixel meets its fragments residue class by residue class.  Which chunk an entry lands in must not
show beyond rounding.

Scenes, the smallest shapes at which the deal can go wrong: one 16x16 tile under K stacked triangles at distinct depths, K = 65
(33 + 32: every chunk partial, the workgroup's first included), 128 (64 + 64: the slot is staged), 129 (three chunks of 43) and 130
(44 + 43 + 43: a remainder); a crowded mesh at 16, 20 and 33 pixels (ragged tiles); tame and non-tame records in one chunk (the slow
mask's bits follow their lane's entry); six and nine channels; three frames at 64; eight frames at 64 (the smallest launch that
issues its tiles in an order of its own); 2500 faces in the centre of a 64x64 image (more than one list round; held to 1e-5 as in
tests/test_forward_kernel_choice_gpu.py).

Every scene is forced through the pair walk, with one team and with two teams of four waves per tile (team t walks the chunks
t, t + 2, ...: with an odd chunk count one team makes a trip with no entries), and held against the CPU oracle (colours <= 1e-6,
the project's PAIR_TOL), against the one-wave reference-order kernel (the running-maximum plane aggrs[:, 1] exactly), against a
second run (bit-equal), in the fixed tile order against the launch's own (bit-equal), and one team against two (<= PAIR_TOL)."""
import importlib

import numpy as np
import pytest
import torch

from lasr_amd import _lib, synth
from lasr_amd.soft_renderer import functional as srf

BIG = 10 ** 12
PAIR_WALK = (0, 0, 0, -1, 0)              # every launch through the pair-walk kernel
PAIR_WALK_FIXED = (0, 0, 0, 0, 0)         # ... in the fixed tile order
PAIR_WALK_OWN = (0, 0, 0, BIG, 0)         # ... in the launch's own order wherever one can be built
ONE_WAVE = (0, 0, 0, -1, BIG)             # one wave per 8x8 tile, faces in index order
PAIR_TOL = 1e-6


def stack(K):
    """K identical triangles at distinct depths over one 16x16 image: the vertical edge at x = -0.03 puts the pixel centres of
    columns 0..7 inside every face; all K pixel rects hold the whole tile's left half, so the tile's list has exactly K entries."""
    fv = np.zeros((1, K, 3, 3), np.float32)
    fv[0, :, :, :2] = np.asarray([[-0.03, -2.5], [-0.03, 2.5], [-3., 0.]], np.float32)
    fv[0, :, :, 2] = (2. + 0.02 * np.arange(K, dtype=np.float32))[:, None]
    ft = np.random.default_rng(K).uniform(0, 1, fv.shape).astype(np.float32)
    return fv, ft, 1.0, 5.0


def _not_tame():
    # as tests/test_pair_walk_lane_balance_gpu.py: a sliver, a zero-area face, a face in front of the near plane, huge coordinates
    fv, ft, near, far = synth.raster_batch(4, 3, count=2)
    fv = fv.copy()
    fv[0, 0] = [[0, 0, 3], [0.5, 0.5, 3], [1e-7, 0, 3]]
    fv[0, 1] = [[0.1, 0.1, 3], [0.1, 0.1, 3], [0.1, 0.1, 3]]
    fv[1, 2, :, 2] = 1e-9
    fv[1, 3] = [[-3e4, -2e4, 3], [4e4, -1e4, 3], [0, 5e4, 3]]
    return fv, ft, near, far


def _channels(C):
    fv, ft, near, far = synth.raster_batch(4, 3, count=2)
    rng = np.random.default_rng(C)
    tex = np.concatenate([ft] + [rng.uniform(-2, 2, ft.shape).astype(np.float32) for _ in range(C // 3 - 1)], -1)
    return fv, tex, near, far


def _long_list():
    # tests/test_forward_kernel_choice_gpu.py: 2500 faces in the centre, the tiles there need more than one list round
    rng = np.random.default_rng(7)
    F = 2500
    c = rng.uniform(-0.15, 0.15, (2, F, 1, 2))
    tri = c + rng.uniform(-0.08, 0.08, (2, F, 3, 2))
    z = rng.uniform(2, 4, (2, F, 3, 1))
    fv = np.concatenate([tri, z], -1).astype(np.float32)
    fv[0, 0] = [[-1.5, -1.2, 3], [1.4, -1.1, 3.5], [0.1, 1.6, 2.5]]
    ft = rng.uniform(0, 1, fv.shape).astype(np.float32)
    return fv, ft, 1.0, 5.0


# name -> (scene builder, image size, colour tolerance against the oracle); every scene is (face_vertices, textures, near, far)
CASES = {
    'stack of 65': (lambda: stack(65), 16, PAIR_TOL),
    'stack of 128': (lambda: stack(128), 16, PAIR_TOL),
    'stack of 129': (lambda: stack(129), 16, PAIR_TOL),
    'stack of 130': (lambda: stack(130), 16, PAIR_TOL),
    'crowded 16': (lambda: synth.raster_batch(4, 3, count=1), 16, PAIR_TOL),
    'ragged 20': (lambda: synth.raster_batch(4, 3, count=1), 20, PAIR_TOL),
    'ragged 33': (lambda: synth.raster_batch(4, 3, count=1), 33, PAIR_TOL),
    'tame and not tame': (_not_tame, 64, PAIR_TOL),
    'six channels': (lambda: _channels(6), 48, PAIR_TOL),
    'nine channels': (lambda: _channels(9), 48, PAIR_TOL),
    'three frames': (lambda: synth.raster_batch(4, 3, count=3), 64, PAIR_TOL),
    'eight frames': (lambda: synth.raster_batch(4, 5, count=8), 64, PAIR_TOL),
    'long list': (_long_list, 64, 1e-5),
}
_refs = {}


def background(C):
    return [1., 1., 1.] if C == 3 else [0.25 * k for k in range(C)]


def oracle_image(oracle, name):
    """The oracle's image of a case, [N, C + 1, IS, IS] (alpha last); computed once, triple by triple for six and nine channels."""
    if name not in _refs:
        build, IS, _ = CASES[name]
        fv, ft, near, far = build()
        C = ft.shape[-1]
        bg = background(C)
        parts = [oracle.forward(fv, np.ascontiguousarray(ft[..., k:k + 3]), IS,
                                **dict(synth.LASR_MODES, near=near, far=far, background_color=bg[k:k + 3]))['soft_colors']
                 for k in range(0, C, 3)]
        img = np.concatenate([p[:, :3] for p in parts] + [parts[0][:, 3:4]], 1)
        img.setflags(write=False)
        _refs[name] = img
    return _refs[name]


class _Ctx:                                 # what SoftRasterizeFunction.forward needs of an autograd context: it keeps aggrs_info
    def save_for_backward(self, *t):
        self.saved = t

    def mark_non_differentiable(self, *t):
        pass


def render(dev, scene, IS):
    """(soft_colors, aggrs_info) of a scene through the operator's forward, with the launch options and flags in force."""
    sr_mod = importlib.import_module('lasr_amd.soft_renderer.functional.soft_rasterize')
    fv, ft, near, far = scene
    m = synth.LASR_MODES
    ctx = _Ctx()
    img = sr_mod.SoftRasterizeFunction.forward(
        ctx, torch.from_numpy(fv).to(dev), torch.from_numpy(ft).to(dev), IS, background(ft.shape[-1]), near, far, m['fill_back'],
        m['eps'], m['sigma_val'], m['dist_func'], m['dist_eps'], m['gamma_val'], m['aggr_func_rgb'], m['aggr_func_alpha'],
        m['texture_type'])
    torch.cuda.synchronize()
    return img.cpu().numpy(), ctx.saved[3].cpu().numpy()


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(CASES))
def test_dealt_chunks_agree_with_the_oracle_and_keep_the_running_maximum(oracle, cuda, name):
    build, IS, tol = CASES[name]
    scene = build()
    ref = oracle_image(oracle, name)
    out = {}
    try:
        srf.set_launch_thresholds(*ONE_WAVE)
        _, aggr_ref = render(cuda, scene, IS)
        for flag, teams in ((_lib.SR_PAIR_ONE_TEAM, 'one team'), (_lib.SR_PAIR_TWO_TEAMS, 'two teams')):
            srf.set_forward_flags(flag)
            srf.set_launch_thresholds(*PAIR_WALK)
            img, aggr = render(cuda, scene, IS)
            img2, aggr2 = render(cuda, scene, IS)
            srf.set_launch_thresholds(*PAIR_WALK_FIXED)
            img_f, aggr_f = render(cuda, scene, IS)
            srf.set_launch_thresholds(*PAIR_WALK_OWN)
            img_o, aggr_o = render(cuda, scene, IS)
            err = float(np.abs(img - ref).max())
            print('%s, %s: pair walk against the oracle, max abs %.3e' % (name, teams, err))
            assert img.shape == ref.shape and np.isfinite(img).all()
            assert err <= tol, '%s, %s: max %.3e' % (name, teams, err)
            assert np.array_equal(aggr[:, 1], aggr_ref[:, 1]), '%s, %s: running maximum differs from the one-wave kernel' % (name, teams)
            assert same_bits(img, img2) and same_bits(aggr, aggr2), '%s, %s: a second run differs' % (name, teams)
            assert same_bits(img_f, img_o) and same_bits(aggr_f, aggr_o), '%s, %s: the tile order shows' % (name, teams)
            assert same_bits(img, img_f) and same_bits(aggr, aggr_f)
            out[teams] = img
    finally:
        srf.set_forward_flags(_lib.SR_DEFAULT_FLAGS)
        srf.set_launch_thresholds()
    d = float(np.abs(out['one team'] - out['two teams']).max())
    print('%s: one team against two, max abs %.3e' % (name, d))
    assert d <= PAIR_TOL, '%s: one team against two, max %.3e' % (name, d)
