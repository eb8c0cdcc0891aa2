"""The pair walk's store-only path for empty tiles (lasr_amd/csrc/sr_forward_pairs.h: store_empty_tile).  sr_order_kernel flags the
entries of the launch's order table whose tile no face's pixel rect overlaps; a workgroup that draws such an entry forms the
tile's outputs from the launch's scalars and one wave stores them -- 16-byte stores where the tile lies inside an image whose side
is a multiple of 4, the tensors are 16-byte aligned and the call has a background argument; pixel by pixel otherwise.  (The
one-team kernel of six channels reads the flag and keeps the tile path, which costs it no register: the same checks hold.)

Every case goes through the C ABI (pair_min_tiles = 0: the pair walk whatever the size) into NaN-filled outputs, once with the
launch's own tile order and once with order_max_tiles = 0: that launch has no table and can never take the new path.  Asserted:
the plan (so the ordered call did have a table), the number of flagged entries found in the table afterwards (so the case is what
its name says), torch.equal on soft_colors and aggrs_info, no NaN left, and the pair walk's bar against oracle/sr_oracle (1e-6,
tests/test_forward_kernel_choice_gpu.py)."""
import numpy as np
import pytest
import torch

import raster_harness as rh
from lasr_amd import _lib, synth
from raster_harness import BIG, PAIR_TOL

pytestmark = pytest.mark.gpu

ONE, TWO = _lib.SR_PAIR_ONE_TEAM, _lib.SR_PAIR_TWO_TEAMS
#  kind -> (scale, shift) of the level-4 blob (320 faces)
MESHES = {'small': (0.3, (0.35, -0.3)),                        # a blob a third of the frame wide, off-centre
          'right of the frame': (None, (5., 0.)),
          'below the frame': (None, (0., -7.)),
          'everywhere': (3.5, (0., 0.)),                       # every tile meets a face
          'plain': (None, (0., 0.))}


def mesh(kind, N):
    """(face_vertices [N, F, 3, 3], near, far) of the level-4 blob (320 faces), N frames of its turn."""
    return rh.cached(('empty tiles', kind, N), lambda: rh.blob(N, *MESHES[kind]))


def forward(dev, fv, tex, near, far, IS, C, order_max, flags, bg, offset=0, plain_entry=False):
    N, F = fv.shape[:2]
    out = dict(colors=rh.carve_at_offset(dev, (N, C + 1, IS, IS), offset), aggrs=rh.carve_at_offset(dev, (N, 2, IS, IS), offset))
    prefill = [0.25 + 0.0625 * k for k in range(C)] if bg is None else None
    if plain_entry:
        assert bg is None
        rec = rh.forward(dev, fv, tex, near, far, IS, prefill=prefill, out=out, plain_entry=True)
    else:
        rec = rh.forward(dev, fv, tex, near, far, IS, options=(0, 0, 0, order_max, 0), flags=flags, background=bg, prefill=prefill, out=out)
    return rec.colors, rec.aggrs, rec.plan, rh.order_table(rec.ws, N, F, IS, 16)


def textures(F, N, C, seed=5):
    rng = np.random.default_rng(seed)
    return rng.uniform(0, 1, (N, F, 3, C)).astype(np.float32)


def check(oracle, dev, kind, N, IS, C=3, flags=ONE, with_bg=True, offset=0, plain_entry=False, flagged=None):
    fv, near, far = mesh(kind, N)
    F = fv.shape[1]
    tex = textures(F, N, C)
    bg = [0.125 * (k + 1) for k in range(C)] if with_bg else None
    t16 = (IS + 15) // 16
    tiles = N * t16 * t16
    form = _lib.SR_FORM_PAIRS_ONE_TEAM if flags == ONE else _lib.SR_FORM_PAIRS_TWO_TEAMS
    want_c, want_a, p0, _ = forward(dev, fv, tex, near, far, IS, C, 0, flags, bg, offset)
    assert (p0.form, p0.ordered, p0.grid) == (form, 0, tiles)
    got_c, got_a, p1, table = forward(dev, fv, tex, near, far, IS, C, BIG, flags, bg, offset, plain_entry)
    if p1 is not None:
        assert (p1.form, p1.ordered, p1.tile_shift, p1.grid) == (form, 1, 4, tiles)
    # the table: a permutation of the launch's tiles under the flag, the flagged entries last in every XCD's list
    plain = table & 0x7fffffff
    assert sorted(plain.tolist()) == [(n << 16) | (y << 8) | x for n in range(N) for y in range(t16) for x in range(t16)]
    n_flag = int((table < 0).sum())
    for x in range(8):
        mine = table[x * (tiles // 8):(x + 1) * (tiles // 8)] < 0
        assert (np.diff(mine.astype(np.int8)) >= 0).all()
    lo, hi = flagged if flagged is not None else (0, tiles)
    assert lo <= n_flag <= hi, '%d of %d entries flagged, expected %d..%d' % (n_flag, tiles, lo, hi)
    assert not torch.isnan(got_c).any() and not torch.isnan(got_a).any()
    assert torch.equal(got_c, want_c), 'soft_colors: %d values differ' % int((got_c != want_c).sum())
    assert torch.equal(got_a, want_a), 'aggrs_info: %d values differ' % int((got_a != want_a).sum())
    # the oracle renders three channels: one call per attribute triple (the channels are independent)
    kw = dict(synth.LASR_MODES, near=near, far=far)
    img = got_c.cpu().numpy()
    for g in range(C // 3):
        kw['background_color'] = bg[3 * g:3 * g + 3] if with_bg else [0.25 + 0.0625 * (3 * g + k) for k in range(3)]
        ref = oracle.forward(fv, tex[..., 3 * g:3 * g + 3], IS, **kw)['soft_colors']
        err = max(np.abs(img[:, 3 * g:3 * g + 3] - ref[:, :3]).max(), np.abs(img[:, C] - ref[:, 3]).max())
        assert err <= PAIR_TOL, 'channels %d..%d: %.3e from the oracle' % (3 * g, 3 * g + 2, err)
    return n_flag


@pytest.mark.parametrize('flags', [ONE, TWO], ids=['one team', 'two teams'])
@pytest.mark.parametrize('C', [3, 6, 9])
def test_a_small_blob_leaves_most_tiles_to_the_store_only_path(oracle, cuda, flags, C):
    check(oracle, cuda, 'small', 8, 64, C=C, flags=flags, flagged=(8 * 16 // 2 + 1, 8 * 16 - 8))


@pytest.mark.parametrize('flags', [ONE, TWO], ids=['one team', 'two teams'])
@pytest.mark.parametrize('kind', ['right of the frame', 'below the frame'])
def test_a_mesh_of_culled_faces_only_flags_every_entry(oracle, cuda, kind, flags):
    check(oracle, cuda, kind, 8, 64, flags=flags, flagged=(128, 128))


@pytest.mark.parametrize('flags', [ONE, TWO], ids=['one team', 'two teams'])
def test_a_mesh_that_covers_every_tile_flags_none(oracle, cuda, flags):
    check(oracle, cuda, 'everywhere', 8, 64, flags=flags, flagged=(0, 0))


@pytest.mark.parametrize('flags', [ONE, TWO], ids=['one team', 'two teams'])
@pytest.mark.parametrize('IS', [72, 70])
def test_ragged_edge_tiles_and_sides_that_are_no_multiple_of_four(oracle, cuda, IS, flags):
    # 5 x 5 tiles per frame, the last column and row 8 (6) pixels wide: 200 tiles, a multiple of 8.  72: inner tiles by 16-byte
    # stores, edge tiles pixel by pixel; 70: rows are only 8-byte aligned, every tile pixel by pixel
    check(oracle, cuda, 'small', 8, IS, flags=flags, flagged=(101, 192))


@pytest.mark.parametrize('C', [3, 9])
def test_without_a_background_argument_the_prefilled_image_is_the_background(oracle, cuda, C):
    check(oracle, cuda, 'small', 8, 64, C=C, with_bg=False, flagged=(65, 120))


def test_the_plain_entry_point_on_a_prefilled_image(oracle, cuda):
    # lasr_sr_forward has neither options nor a background: 8 frames of 200x200 are 5000 8x8 tiles (the pair walk from 3072 up),
    # 1352 16x16 tiles (ordered; two teams up to 3072), the last column and row 8 pixels wide
    check(oracle, cuda, 'small', 8, 200, flags=TWO, with_bg=False, plain_entry=True, flagged=(677, 1344))


@pytest.mark.parametrize('flags', [ONE, TWO], ids=['one team', 'two teams'])
@pytest.mark.parametrize('C', [3, 9])
def test_outputs_that_are_four_byte_aligned_and_no_more(oracle, cuda, C, flags):
    check(oracle, cuda, 'small', 8, 64, C=C, flags=flags, offset=1, flagged=(65, 120))


def test_five_frames_are_the_smallest_ordered_launch(oracle, cuda):
    check(oracle, cuda, 'small', 5, 64, flagged=(41, 75))              # 80 tiles, an image split between two XCDs
