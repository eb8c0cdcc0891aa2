"""The forward pair walk classifies by ROW SPANS (lasr_amd/csrc/sr_forward_pairs.h: span_edge / span_row): lane = entry computes,
for each row of the tile, the one run of columns the entry does not certainly miss, and a 64 x 64 bit transpose across the wave
(wave_transpose64) turns the entries' words into the per-pixel masks the walk pops.  Checked here on the CPU alone, with the
float32 numpy restatement of tests/pair_spans_restated.py:

  the superset property -- NO (pixel, entry) pair of the entry's pixel rect whose pixel centre lies inside the face or closer to it
  than sqrt(thr), by a float64 point-triangle distance, is missing from the spans: on every face of the bench frames 0, 37 and 101
  at 256 pixels (mesh M2) and on hand-made faces at 32 and at a ragged 24 pixels;
  the pairs the spans keep beyond the per-pixel test they replace (w_k < far[k] at every pixel of the rect) are counted and printed;
  on the bench frames they must stay below twice the measured share -- 0.074 % measured (439 of 593 471 on frame 0), so 0.148 % -- so that a slack set far too
  wide cannot hide;
  entries the conservative reject does not apply to (flags bit 4 clear) keep exactly their pixel rect;
  the six stages of the transpose against numpy's."""
import numpy as np
import pytest

import bench
import pair_spans_restated as ps
from lasr_amd import synth
from raster_harness import hand_made

BENCH_FRAMES = (0, 37, 101)
EXTRA_SHARE_MEASURED = 0.00074           # spans beyond the per-pixel test on the bench frames, as a share of that test's pairs
_bench = {}


def bench_frame(fr):
    if not _bench:
        v, f, _ = synth.blobby_mesh(bench.NU)
        pv = synth.frame_vertices(v, bench.N_FRAMES_CYCLE, first=0, count=max(BENCH_FRAMES) + 1)
        for k in BENCH_FRAMES:
            _bench[k] = np.ascontiguousarray(pv[k][f], np.float32)
    return _bench[fr]


def masks(fv, IS):
    thr = ps.threshold()
    rec = ps.records(fv, IS, thr)
    face, tx, ty = ps.tile_pairs(rec, IS)
    span = ps.span_masks(rec, face, tx, ty, IS)
    return rec, face, span, ps.pixel_test_masks(rec, face, tx, ty, IS), ps.rect_masks(rec, face, tx, ty), \
        ps.exact_masks(rec, face, tx, ty, IS, thr)


@pytest.mark.parametrize('fr', BENCH_FRAMES)
def test_bench_frames_lose_no_pair_and_gain_few(fr):
    rec, face, span, pixel, rect, exact = masks(bench_frame(fr), 256)
    real = exact & rect
    missing = int((real & ~span).sum())
    extra = int((span & ~pixel).sum())
    dropped = int((pixel & ~span).sum())
    print('frame %d: %d (face, tile) pairs on %d busy tiles, rect %d, per-pixel test %d, spans %d, exact %d; spans beyond the per-pixel '
          'test %d (%.3f %%), per-pixel beyond the spans %d, exact pairs missing %d'
          % (fr, len(face), len(set(zip(*ps.tile_pairs(rec, 256)[1:]))), rect.sum(), pixel.sum(), span.sum(), real.sum(), extra,
             100. * extra / pixel.sum(), dropped, missing))
    assert missing == 0
    assert int((real & ~pixel).sum()) == 0                      # (the line test itself keeps every exact pair)
    assert not (span & ~rect).any()
    assert extra <= 2 * EXTRA_SHARE_MEASURED * pixel.sum()


@pytest.mark.parametrize('IS', [32, 24])
def test_hand_made_faces_lose_no_pair(IS):
    names = list(hand_made())
    fv = np.asarray([hand_made()[n] for n in names], np.float32)
    rec, face, span, pixel, rect, exact = masks(fv, IS)
    assert set(face.tolist()) == set(range(len(names)))        # every face meets the image
    assert [bool(w) for w in rec['well']] == [n != 'edge-on, flag 16 clear' for n in names]
    a = fv[names.index('A == 0 on a pixel-centre row')]
    assert a[0, 1] == a[1, 1] and rec['inv'][names.index('A == 0 on a pixel-centre row'), 6] == 0
    whole = names.index('rect covers a whole tile')
    assert any(rect[i].all() for i in np.nonzero(face == whole)[0])
    for i, n in enumerate(names):
        sel = face == i
        real = exact[sel] & rect[sel]
        print('%d px, %s: rect %d, per-pixel test %d, spans %d, exact %d, missing %d'
              % (IS, n, rect[sel].sum(), pixel[sel].sum(), span[sel].sum(), real.sum(), (real & ~span[sel]).sum()))
        assert real.sum() > 0
        assert int((real & ~span[sel]).sum()) == 0, n
        assert not (span[sel] & ~rect[sel]).any()
        if not rec['well'][i]:
            assert np.array_equal(span[sel], rect[sel])           # today's candidates, as they are
        else:
            assert span[sel].sum() < rect[sel].sum() or rect[sel].sum() == real.sum()
    if IS == 24:                                                   # the rects end at the image: no bit beyond column / row 23
        _, tx, ty = ps.tile_pairs(rec, IS)
        cols = tx[:, None, None] * 16 + np.arange(16)[None, None, :]
        rows = ty[:, None, None] * 16 + np.arange(16)[None, :, None]
        assert not (span & ((cols >= IS) | (rows >= IS))).any()


def test_entries_that_are_not_tame_keep_their_rect():
    fv = np.asarray([hand_made()['sliver'], hand_made()['rect covers a whole tile']], np.float32)
    thr = ps.threshold()
    rec = ps.records(fv, 32, thr)
    face, tx, ty = ps.tile_pairs(rec, 32)
    span = ps.span_masks(rec, face, tx, ty, 32, tame=np.array([True, False]))
    rect = ps.rect_masks(rec, face, tx, ty)
    assert np.array_equal(span[face == 1], rect[face == 1]) and span[face == 0].sum() < rect[face == 0].sum()


def test_the_six_stage_transpose_is_a_transpose():
    rng = np.random.default_rng(64)
    cases = {
        'random': [int(x) for x in rng.integers(0, 2 ** 64, 64, dtype=np.uint64)],
        'identity': [1 << e for e in range(64)],
        'all ones': [2 ** 64 - 1] * 64,
        'zero': [0] * 64,
        'anti-diagonal': [1 << (63 - e) for e in range(64)],
    }
    for r in (0, 17, 63):
        cases['row %d' % r] = [(2 ** 64 - 1) if e == r else 0 for e in range(64)]
        cases['single bit (%d, %d)' % (r, 63 - r // 2)] = [(1 << (63 - r // 2)) if e == r else 0 for e in range(64)]
    for name, words in cases.items():
        got = ps.transpose64(words)
        assert got == ps.transpose64_numpy(words), name
        assert ps.transpose64(got) == words, name
    assert ps.transpose64(cases['identity']) == cases['identity'] and ps.transpose64(cases['row 17']) == [1 << 17] * 64
