"""tests/raster_harness.py on the CPU: what the raster tests lean on must itself be right -- the workspace layout against the
library's own size, the mode scalars against the operator's, the comparisons at and around their bars, and the oracle reference of
a nine-channel input against three plain oracle calls."""
import importlib

import numpy as np
import pytest

import raster_harness as rh
from lasr_amd import _lib, synth


@pytest.mark.parametrize('ptr', [0, 4096 + 36, 255])
@pytest.mark.parametrize('N,F,IS', [(1, 1, 8), (3, 49, 24), (8, 320, 64), (2, 2500, 64), (5, 64, 0), (5, 65, 33)])
def test_the_layout_adds_up_to_the_library_s_workspace_size(N, F, IS, ptr):
    L = rh.layout(ptr, N, F, IS)
    assert L.total == _lib.lib().lasr_sr_workspace_bytes(N, F, 3, IS)
    base = rh.layout(0, N, F, IS)
    shift = (-ptr) % 256
    assert (ptr + L.recs) % 256 == 0 and L.recs == shift
    assert [L.recs, L.rects, L.grects, L.choice, L.order] == [o + shift for o in (base.recs, base.rects, base.grects, base.choice, base.order)]
    assert L.rects - L.recs >= N * F * rh.REC_FLOATS * 4 and L.grects - L.rects >= N * F * 8
    assert L.choice - L.grects >= N * ((F + rh.GROUP - 1) // rh.GROUP) * 8 and L.order - L.choice == 256
    assert L.order + N * ((IS + 7) // 8) ** 2 * 4 <= L.total            # the table of 8x8 tiles ends inside the workspace


def test_the_tail_is_the_operator_s_mode_scalars():
    sr_mod = importlib.import_module('lasr_amd.soft_renderer.functional.soft_rasterize')

    def scalars(**over):
        m = dict(synth.LASR_MODES, **over)
        return sr_mod._mode_scalars(m['eps'], m['sigma_val'], m['dist_func'], m['dist_eps'], m['gamma_val'], m['aggr_func_rgb'],
                                    m['aggr_func_alpha'], m['texture_type'], m['fill_back'])
    assert rh.tail() == scalars() and len(rh.tail()) == 9
    assert rh.tail(1e-4) == rh.tail(sigma=1e-4) == scalars(sigma_val=1e-4)
    assert rh.tail(7e-3) == scalars(sigma_val=7e-3) != rh.tail()
    assert rh.tail(alpha='sum') == scalars(aggr_func_alpha='sum') != rh.tail()
    hard = dict(dist_func='hard', aggr_func_rgb='hard', aggr_func_alpha='hard')
    assert rh.tail(**hard) == scalars(**hard)


def test_same_bits_sees_one_ulp_a_signed_zero_and_a_shape():
    a = np.linspace(0.1, 0.9, 12, dtype=np.float32).reshape(3, 4)
    assert rh.same_bits(a, a.copy())
    b = a.copy()
    b[1, 2] = np.nextafter(b[1, 2], np.float32(2))
    assert not rh.same_bits(a, b)
    assert not rh.same_bits(np.zeros(4, np.float32), -np.zeros(4, np.float32))
    assert not rh.same_bits(a, a.reshape(4, 3)) and not rh.same_bits(a, a[:2])


def test_check_grad_holds_the_bar_relative_to_the_largest_reference_gradient():
    ref = np.array([[2.0, -8.0], [0.5, 0.0]])
    off = np.array([[0.0, 0.0], [1.0, 0.0]])                   # the difference sits on a SMALL entry: the bar is the largest one's
    rh.check_grad('inside', ref + 0.9e-3 * 8.0 * off, ref)
    with pytest.raises(AssertionError):
        rh.check_grad('outside', ref + 1.1e-3 * 8.0 * off, ref)
    bad = ref.copy()
    bad[0, 0] = np.nan
    with pytest.raises(AssertionError):
        rh.check_grad('not finite', bad, ref)
    with pytest.raises(AssertionError):
        rh.check_grad('no gradient', np.zeros_like(ref), np.zeros_like(ref))
    rh.check_grad('a wider bar', ref + 1.1e-3 * 8.0 * off, ref, rel=2e-3)


def test_the_oracle_reference_of_nine_channels_is_three_oracle_calls(oracle):
    IS = 8
    fv, _, near, far = synth.raster_batch(1, 3, count=1)               # the smallest blob: 20 faces
    N, F = fv.shape[:2]
    rng = np.random.default_rng(1)
    tex = rng.uniform(0, 1, (N, F, 3, 9)).astype(np.float32)
    g = rng.standard_normal((N, 10, IS, IS)).astype(np.float32)
    bg = [0.125 * (k + 1) for k in range(9)]
    kw = dict(synth.LASR_MODES, near=near, far=far)
    img, gf, gt = rh.oracle_reference(oracle, fv, tex, IS, bg, kw, g=g)
    assert img.shape == (N, 10, IS, IS) and gf.shape == (N, F, 3, 3) and gt.shape == (N, F, 3, 9)
    assert not (img.flags.writeable or gf.flags.writeable or gt.flags.writeable)
    gf_sum, gf_colour_only = 0, 0
    for k in range(3):
        okw = dict(kw, background_color=bg[3 * k:3 * k + 3])
        ref = oracle.forward(fv, np.ascontiguousarray(tex[..., 3 * k:3 * k + 3]), IS, **okw)
        assert np.array_equal(img[:, 3 * k:3 * k + 3], ref['soft_colors'][:, :3]) and np.array_equal(img[:, 9], ref['soft_colors'][:, 3])
        colour = np.concatenate([g[:, 3 * k:3 * k + 3], np.zeros_like(g[:, 9:10])], 1)
        with_alpha = np.concatenate([g[:, 3 * k:3 * k + 3], g[:, 9:10]], 1)
        gf_k, gt_k = oracle.backward(ref, with_alpha if k == 0 else colour, IS, **okw)
        assert np.array_equal(gt[..., 3 * k:3 * k + 3], gt_k)
        gf_sum = gf_sum + gf_k
        gf_colour_only = gf_colour_only + (oracle.backward(ref, colour, IS, **okw)[0] if k == 0 else gf_k)
    assert np.array_equal(gf, gf_sum)
    # alpha's upstream gradient exactly once: what is left of the sum without the colour terms is one alpha-only backward
    alpha_only = oracle.backward(ref, np.concatenate([np.zeros_like(g[:, :3]), g[:, 9:10]], 1), IS, **okw)[0]
    scale = float(np.abs(alpha_only).max())
    assert scale > 0 and np.abs((gf - gf_colour_only) - alpha_only).max() <= 1e-4 * max(scale, float(np.abs(gf).max()))
    # and without g: the image alone (three channels: one more oracle call)
    img3, none_f, none_t = rh.oracle_reference(oracle, fv, tex[..., :3], IS, bg[:3], kw)
    assert np.array_equal(img3[:, :3], img[:, :3]) and np.array_equal(img3[:, 3], img[:, 9]) and none_f is None and none_t is None
