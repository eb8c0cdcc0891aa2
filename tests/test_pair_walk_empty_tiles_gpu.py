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
import ctypes
import math

import numpy as np
import pytest
import torch

from lasr_amd import _lib, synth

pytestmark = pytest.mark.gpu

PAIR_TOL = 1e-6
ONE, TWO = _lib.SR_PAIR_ONE_TEAM, _lib.SR_PAIR_TWO_TEAMS
BIG = 10 ** 12


def _tail():
    m = synth.LASR_MODES
    return (float(m['eps']), float(m['sigma_val']), 2, float(math.log(1. / m['dist_eps'] - 1.)), float(m['gamma_val']), 1, 2, 1, 1)


_meshes = {}


def mesh(kind, N):
    """(face_vertices [N, F, 3, 3], near, far) of the level-4 blob (320 faces), N frames of its turn."""
    if (kind, N) not in _meshes:
        fv, _, near, far = synth.raster_batch(4, max(N, 3), count=N)
        fv = fv.copy()
        if kind == 'small':                                    # a blob a third of the frame wide, off-centre
            fv[..., :2] = fv[..., :2] * 0.3 + np.array([0.35, -0.3], np.float32)
        elif kind == 'right of the frame':
            fv[..., 0] += 5.
        elif kind == 'below the frame':
            fv[..., 1] -= 7.
        elif kind == 'everywhere':                             # every tile meets a face
            fv[..., :2] *= 3.5
        else:
            assert kind == 'plain'
        _meshes[kind, N] = (np.ascontiguousarray(fv), float(near), float(far))
    return _meshes[kind, N]


def carve(dev, shape, offset_floats):
    """A NaN-filled float tensor of `shape` that starts `offset_floats` floats into its (256-byte aligned) buffer."""
    n = int(np.prod(shape))
    buf = torch.full((n + offset_floats,), float('nan'), dtype=torch.float32, device=dev)
    t = buf[offset_floats:].view(*shape)
    assert t.data_ptr() % 16 == (4 * offset_floats) % 16
    return t


def forward(dev, fv, tex, near, far, IS, C, order_max, flags, bg, offset=0, plain_entry=False):
    h = _lib.lib()
    N, F = fv.shape[:2]
    tfv = torch.from_numpy(fv).reshape(N, F, 9).to(dev).contiguous()
    tft = torch.from_numpy(tex).to(dev).contiguous()
    colors, aggrs = carve(dev, (N, C + 1, IS, IS), offset), carve(dev, (N, 2, IS, IS), offset)
    if bg is None:                                             # no background argument: the caller's image is the background
        for k in range(C):
            colors[:, k] = 0.25 + 0.0625 * k
    nbytes = h.lasr_sr_workspace_bytes(N, F, 3, IS)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    t = _tail()
    if plain_entry:
        assert C == 3 and bg is None
        _lib.check(h.lasr_sr_forward(tfv.data_ptr(), tft.data_ptr(), None, aggrs.data_ptr(), colors.data_ptr(), ws.data_ptr(), nbytes,
                                     N, F, 3, IS, near, far, *t, st), 'lasr_sr_forward')
        p = None
    else:
        options = _lib.SrOptions(0, 0, 0, order_max, 0)
        p = _lib.SrPlan()
        assert h.lasr_sr_plan_forward(N, F, 3, C, IS, 2, 1, 2, 1, 1, flags, ctypes.byref(options), ctypes.byref(p)) == 0
        cbg = (ctypes.c_float * C)(*bg) if bg is not None else None
        _lib.check(h.lasr_sr_forward_opt(tfv.data_ptr(), tft.data_ptr(), None, aggrs.data_ptr(), colors.data_ptr(), ws.data_ptr(), nbytes,
                                         N, F, 3, C, IS, near, far, None, *t, cbg, flags, ctypes.byref(options), st), 'lasr_sr_forward_opt')
    torch.cuda.synchronize()
    # the order table the call left in its workspace (sr_raster.hip: sr_layout), in 16x16 tiles
    up = lambda v: (v + 255) // 256 * 256                      # noqa: E731
    o_order = (-ws.data_ptr()) % 256 + up(N * F * 48 * 4) + up(N * F * 8) + up(N * ((F + 63) // 64) * 8) + 256
    t16 = (IS + 15) // 16
    table = ws[o_order:o_order + N * t16 * t16 * 4].view(torch.int32).cpu().numpy()
    return colors, aggrs, p, table


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
