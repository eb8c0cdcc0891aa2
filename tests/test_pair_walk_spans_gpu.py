"""The forward pair walk with row-span classification and the cross-lane bit transpose (lasr_amd/csrc/sr_forward_pairs.h: span_edge,
span_row, wave_transpose64) on the GPU, through the C ABI with pair_min_tiles = 0 (the pair walk whatever the size) into NaN-filled
outputs.

Shapes, the smallest at which the spans can go wrong: 32 pixels (2 x 2 tiles of 16) and a ragged 24; 3 and 8 frames of the level-4
blob (320 faces) as it is and scaled x 3.5 (every tile busy, most faces cut by the image); stacks of 65 / 128 / 129 / 130 faces over
one tile column (partial chunks, a staged slot 63, three chunks, a remainder); the hand-made faces of
tests/test_pair_walk_spans_cases.py -- a sliver, an edge-on face the conservative reject does not apply to, an edge with A == 0 on a
pixel-centre row, an edge through pixel centres, a face half outside the image, a rect the ragged edge cuts, a rect over a whole
tile -- in one chunk together with tame faces of the blob and with records that are not tame.  Every scene with three, six and nine
channels, one and two teams, with and without the background argument.

Asserted: soft_colors within the pair walk's 1e-6 of oracle/sr_oracle; the running-maximum plane torch.equal to the one-wave
kernel's; no NaN left; lasr_sr_backward_ex on that forward within 1e-3 (of the largest reference magnitude) of the oracle's
gradients.  One case runs the transpose's selftest entry point on random words, the identity, all-ones and single-bit rows."""
import numpy as np
import pytest
import torch

import pair_spans_restated as ps
import raster_harness as rh
from lasr_amd import _lib, synth
from raster_harness import GRAD_REL, ONE_WAVE, PAIR_TOL, PAIR_WALK, hand_made

pytestmark = pytest.mark.gpu

ONE, TWO = _lib.SR_PAIR_ONE_TEAM, _lib.SR_PAIR_TWO_TEAMS


def _stack(K):
    fv, _, near, far = rh.stack(K)
    return fv, near, far


def _hand_made():
    """One frame: the hand-made faces, two records that are not tame (a zero-area face, huge coordinates) and 40 tame faces of the
    blob -- 49 entries, one chunk wherever they meet."""
    blob, near, far = rh.blob(3, 1.)
    hm = np.asarray(list(hand_made().values()), np.float32)
    hm[:, :, 2] = 0.5 * (near + far) + 0.01 * np.arange(len(hm), dtype=np.float32)[:, None]
    odd = np.asarray([[[0.1, 0.1, 0], [0.1, 0.1, 0], [0.1, 0.1, 0]], [[-3e4, -2e4, 0], [4e4, -1e4, 0], [0, 5e4, 0]]], np.float32)
    odd[:, :, 2] = 0.5 * (near + far)
    return np.ascontiguousarray(np.concatenate([hm, odd, blob[0, 100:140]])[None]), near, far


SCENES = {
    'plain, 3 frames': lambda: rh.blob(3, 1.),
    'plain, 8 frames': lambda: rh.blob(8, 1.),
    'scaled x 3.5, 3 frames': lambda: rh.blob(3, 3.5),
    'scaled x 3.5, 8 frames': lambda: rh.blob(8, 3.5),
    'stack of 65': lambda: _stack(65),
    'stack of 128': lambda: _stack(128),
    'stack of 129': lambda: _stack(129),
    'stack of 130': lambda: _stack(130),
    'hand-made faces among tame ones': _hand_made,
}


def scene(name):
    def build():
        fv, near, far = SCENES[name]()
        fv.setflags(write=False)
        return fv, near, far
    return rh.cached(('spans scene', name), build)


def textures(F, N, C):
    return np.random.default_rng(5).uniform(0, 1, (N, F, 3, C)).astype(np.float32)


def background(C, with_bg):
    return [0.125 * (k + 1) for k in range(C)] if with_bg else [0.25 + 0.0625 * k for k in range(C)]


def upstream(N, C, IS):
    return np.random.default_rng(9).uniform(-1, 1, (N, C + 1, IS, IS)).astype(np.float32)


def reference(oracle, name, IS, C, with_bg):
    """The oracle's image [N, C + 1, IS, IS] and gradients of a scene; computed once."""
    def compute():
        fv, near, far = scene(name)
        N, F = fv.shape[:2]
        return rh.oracle_reference(oracle, fv, textures(F, N, C), IS, background(C, with_bg), dict(synth.LASR_MODES, near=near, far=far),
                                   g=upstream(N, C, IS))
    return rh.cached(('spans reference', name, IS, C, with_bg), compute)


def forward(dev, fv, tex, near, far, IS, C, options, flags, with_bg):
    bg = background(C, with_bg)                                # no background argument: the caller's image is the background
    return rh.forward(dev, fv, tex, near, far, IS, options=options, flags=flags, background=bg if with_bg else None,
                      prefill=None if with_bg else bg)


@pytest.mark.parametrize('IS', [32, 24])
@pytest.mark.parametrize('name', list(SCENES))
def test_span_classified_pair_walk_against_the_oracle(oracle, cuda, name, IS):
    fv, near, far = scene(name)
    N, F = fv.shape[:2]
    for C in (3, 6, 9):
        tex = textures(F, N, C)
        g = torch.from_numpy(upstream(N, C, IS)).to(cuda)
        for with_bg in (True, False):
            img_ref, gf_ref, gt_ref = reference(oracle, name, IS, C, with_bg)
            one = forward(cuda, fv, tex, near, far, IS, C, ONE_WAVE, 0, with_bg)
            aggr_one = one.aggrs
            assert one.plan.form == _lib.SR_FORM_ONE_WAVE
            for flags, form in ((ONE, _lib.SR_FORM_PAIRS_ONE_TEAM), (TWO, _lib.SR_FORM_PAIRS_TWO_TEAMS)):
                what = '%s, %d px, %d channels, %s, %s background' % (name, IS, C, 'one team' if flags == ONE else 'two teams',
                                                                      'with' if with_bg else 'no')
                rec = forward(cuda, fv, tex, near, far, IS, C, PAIR_WALK, flags, with_bg)
                colors, aggrs = rec.colors, rec.aggrs
                assert rec.plan.form == form, what
                assert not torch.isnan(colors).any() and not torch.isnan(aggrs).any(), what
                err = float(np.abs(colors.cpu().numpy() - img_ref).max())
                gf, gt = rh.backward(cuda, rec, g, near, far, IS)
                egf = float(np.abs(gf.cpu().numpy().reshape(gf_ref.shape) - gf_ref).max() / np.abs(gf_ref).max())
                egt = float(np.abs(gt.cpu().numpy() - gt_ref).max() / np.abs(gt_ref).max())
                print('%s: image %.3e, grad_faces %.3e, grad_textures %.3e (relative to the largest)' % (what, err, egf, egt))
                assert err <= PAIR_TOL, '%s: %.3e from the oracle' % (what, err)
                assert torch.equal(aggrs[:, 1], aggr_one[:, 1]), '%s: running maximum differs from the one-wave kernel' % what
                assert egf <= GRAD_REL and egt <= GRAD_REL, '%s: gradients %.3e, %.3e' % (what, egf, egt)


def test_the_scenes_are_what_their_names_say(oracle):
    fv, near, far = scene('hand-made faces among tame ones')
    rec = ps.records(fv[0], 32, ps.threshold())
    assert fv.shape[1] == 49 and not rec['well'][1] and rec['well'][0] and (rec['rect'][:7, 0] <= rec['rect'][:7, 1]).all()
    for K in (65, 128, 129, 130):
        fv, _, _ = scene('stack of %d' % K)
        r = ps.records(fv[0], 32, ps.threshold())['rect']
        assert fv.shape[1] == K and (r[:, 0] == 0).all() and (r[:, 1] >= 15).all() and (r[:, 2] == 0).all() and (r[:, 3] == 31).all()
    img, _, _ = reference(oracle, 'scaled x 3.5, 3 frames', 32, 3, True)
    assert (img[:, 3].reshape(3, 2, 16, 2, 16).max((2, 4)) > 0.5).all()          # every tile of every frame meets the mesh


def test_the_wave_transposes_64_words(cuda):
    h = _lib.lib()
    rng = np.random.default_rng(64)
    cases = [rng.integers(0, 2 ** 64, 64, dtype=np.uint64) for _ in range(4)]
    cases += [np.asarray([1 << e for e in range(64)], np.uint64), np.full(64, 2 ** 64 - 1, np.uint64), np.zeros(64, np.uint64)]
    for r in (0, 15, 16, 31, 32, 63):
        row = np.zeros(64, np.uint64)
        row[r] = np.uint64(2 ** 64 - 1)
        one = np.zeros(64, np.uint64)
        one[r] = np.uint64(1 << (63 - r))
        cases += [row, one]
    st = torch.cuda.current_stream(cuda).cuda_stream
    for words in cases:
        src = torch.from_numpy(words.view(np.int64)).to(cuda)
        dst = torch.full((64,), -1, dtype=torch.int64, device=cuda)
        _lib.check(h.lasr_selftest_transpose64(src.data_ptr(), dst.data_ptr(), st), 'lasr_selftest_transpose64')
        torch.cuda.synchronize()
        got = [int(x) for x in dst.cpu().numpy().view(np.uint64)]
        assert got == ps.transpose64_numpy([int(w) for w in words])
    assert h.lasr_selftest_transpose64(None, dst.data_ptr(), st) == -1
