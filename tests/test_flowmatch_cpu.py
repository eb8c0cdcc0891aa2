"""The large-displacement matching stage of the variational flow without a device: the restatement (tests/flowmatch_restated.py) on
closed forms and on the dart fixtures, the flags of the three preprocessing scripts and of scripts/reconstruct.py, the C ABI's
host-side checks, and the launch sites of preprocess/flow_match.py against the guarded case (tests/flowmatch_guarded.py).

dart33 / dart35: varflow_restated._ellipse_pair at 96 x 128, an ellipse of semi-axes (7, 5) centred at (40, 60) that moves (21.4,
-8.3) px over a background moving (0.75, -0.5) px.  The object's EPE is taken on the ellipse eroded by 2 px (33 px; zero flow scores
22.95), the background's away from both silhouettes dilated by 2 px and from a 4 px border.  Measured with the float64 restatement at
R = 24, r = 2, kappa = 0.9, N = 16 (plain flow -> with the stage):
            object              background
  dart31    28.95 -> 0.523      0.0040 -> 0.0037      (measured, not asserted)
  dart32    32.79 -> 0.385      0.0035 -> 0.0031      (likewise)
  dart33    22.57 -> 0.037      0.0042 -> 0.0043
  dart35    38.78 -> 0.173      0.0046 -> 0.0044
The bars are the issue's: plain > 10 px, with the stage <= 1 px and <= 0.05 x plain, background <= 0.1 px.  The motion fixtures of
varflow_restated with the stage (EPE over varflow_restated.score_region, plain -> with the stage): trans 0.0030 -> 0.0029, big
0.0025 -> 0.0025, affine 0.0452 -> 0.0451, ellipse 0.0214 -> 0.0167, odd 0.0034 -> 0.0032, seam 0.0060 -> 0.0068: all under the
project's 0.1 px.  tiny (9 x 7, one level) is a plumbing case whose plain flow already scores 0.498 px against a zero-flow 0.72: it
has no 0.1 px bar to stay under, so the test asks that the stage leaves it bit for bit what it was (nothing is seeded there).
"""
import os
import re
import sys

import numpy as np
import pytest

import flowmatch_guarded
import flowmatch_restated as fm
import varflow_restated as vr
from test_guarded_alloc_cpu import launched_in

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'preprocess'))

ENTRY_POINTS = flowmatch_guarded.NATIVES


def _texture(H, W, seed):
    """uint8 [H,W,3] noise: no two patches alike."""
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3)).astype(np.uint8)


# ---- closed forms -------------------------------------------------------------------------------------------------------------------

def test_identical_frames_match_at_zero_and_fuse_returns_its_input():
    q = fm.quantise(_texture(21, 30, 1))
    d, c1 = fm.search(q, q, 6, 2)
    assert not d.any() and not c1.any() and d.dtype == np.int32 and c1.dtype == np.int32
    uv = np.random.default_rng(2).uniform(-1.4, 1.4, (2, 21, 30)).astype(np.float32)       # within a pixel of the match after rounding
    state = {}
    out = fm.fuse(q, q, d, c1, d, uv, 6, state=state)
    assert not state['seeded'].any()
    assert out.dtype == np.float32 and np.array_equal(out.view(np.uint32), uv.view(np.uint32))       # bit for bit


def test_an_integer_shift_is_found_wherever_patch_and_target_are_inside():
    H, W, r, R = 30, 41, 2, 8
    big = _texture(H + 20, W + 20, 3)
    A, B = big[10:10 + H, 10:10 + W], big[10 + 3:10 + 3 + H, 10 - 5:10 - 5 + W]     # A(p) = B(p + (5, -3))
    d, c1 = fm.search(fm.quantise(A), fm.quantise(B), R, r)
    ys, xs = np.mgrid[0:H, 0:W]
    inside = (xs >= r) & (xs < W - r) & (ys >= r) & (ys < H - r) & (xs + 5 >= r) & (xs + 5 < W - r) & (ys - 3 >= r) & (ys - 3 < H - r)
    assert inside.sum() > 600
    assert (d[inside] == (5, -3)).all() and not c1[inside].any()
    # and the two searches are consistent there
    d_ba, _ = fm.search(fm.quantise(B), fm.quantise(A), R, r)
    assert (d_ba[ys[inside] - 3, xs[inside] + 5] == (-5, 3)).all()


def test_a_constant_image_matches_at_zero():
    q = fm.quantise(np.full((12, 17, 3), 77, np.uint8))
    d, c1 = fm.search(q, q, 5, 1)
    assert not d.any() and not c1.any()                                           # every candidate costs 0: the key decides
    # the key's order among equal costs: the shorter displacement, then the smaller dy, then the smaller dx
    A = np.zeros((15, 15, 3), np.uint8)
    B = np.zeros((15, 15, 3), np.uint8)
    A[7, 7] = 200
    B[7, 4] = B[7, 10] = B[4, 7] = B[10, 7] = 200                                 # four exact matches at distance 3, patches apart
    d, c1 = fm.search(fm.quantise(A), fm.quantise(B), 3, 1)
    assert tuple(d[7, 7]) == (0, -3) and c1[7, 7] == 0                            # dy = -3 before dy = 0 and dy = 3
    B[4, 7] = 0
    d, _ = fm.search(fm.quantise(A), fm.quantise(B), 3, 1)
    assert tuple(d[7, 7]) == (-3, 0)                                              # dy = 0 before dy = 3, and dx = -3 before dx = 3
    B[7, 4] = B[7, 10] = 0
    B[7, 9] = 200                                                                 # a shorter one wins whatever its dy and dx
    d, _ = fm.search(fm.quantise(A), fm.quantise(B), 3, 1)
    assert tuple(d[7, 7]) == (2, 0)


def test_a_candidate_outside_the_frame_is_never_chosen():
    for H, W, R, r, seed in ((9, 7, 24, 2, 4), (9, 7, 32, 3, 5), (14, 11, 6, 1, 6)):
        A, B = _texture(H, W, seed), _texture(H, W, seed + 100)
        d, c1 = fm.search(fm.quantise(A), fm.quantise(B), R, r)
        assert fm.inframe(d).all() and np.abs(d).max() <= R
        assert np.array_equal(c1, fm.cost_at(fm.quantise(A), fm.quantise(B), d, r))
    # a frame whose border is what the clamped taps would match best: the clamped position is not a candidate
    A = np.zeros((9, 7, 3), np.uint8)
    B = np.full((9, 7, 3), 255, np.uint8)
    B[:, -1] = 0                                                                  # B's last column equals A everywhere
    d, _ = fm.search(fm.quantise(A), fm.quantise(B), 24, 1)
    assert fm.inframe(d).all() and (d[:, 0, 0] == 6).all() and (d[..., 0] <= 6).all()


def test_the_acceptance_rule_at_an_exact_equality():
    """kappa = 0.9 gives K = 230.  At ccur = 768 the rule 256 c1 < 230 * 768 = 176640 = 256 * 690 holds up to c1 = 689 and fails at
    690, the exact equality; at kappa = 0.5 (K = 128) and ccur = 750 it fails at 375."""
    H, W, r = 11, 11, 1
    assert fm.check(8, 1, -1, 0.9, 0)[3] == 230 and fm.check(8, 1, -1, 0.5, 0)[3] == 128 and 230 * 768 == 256 * 690
    uv = np.zeros((2, H, W))
    B = np.zeros((H, W, 3), np.uint8)
    qB = fm.quantise(B)
    d_ab = np.zeros((H, W, 2), np.int32)
    d_ab[5, 5] = (3, 0)
    d_ba = np.zeros((H, W, 2), np.int32)
    d_ba[5, 8] = (-3, 0)
    for K, extra, total, edge in ((230, (3, 0, 0), 768, 690), (128, (0, 0, 0), 750, 375)):
        A = np.zeros((H, W, 3), np.uint8)
        A[5, 5] = (255, 255, 255) if K == 230 else (250, 250, 250)
        A[5, 6] = extra
        qA = fm.quantise(A)
        for c, want in ((edge - 1, True), (edge, False), (edge + 1, False)):
            c1 = np.full((H, W), c, np.int32)
            seeded, cand, ccur = fm.select(qA, qB, d_ab, c1, d_ba, uv, 8, r, K)
            assert ccur[5, 5] == total and 256 * edge == K * total
            assert bool(seeded[5, 5]) == want and seeded.sum() == int(want)
            assert tuple(cand[5, 5]) == ((3, 0) if want else (0, 0))
    # each of the other two conditions alone keeps the pixel unseeded
    c1 = np.zeros((H, W), np.int32)
    assert not fm.select(qA, qB, d_ab, c1, np.zeros_like(d_ba), uv, 8, r, 128)[0].any()           # not consistent: |3 + 0| > 1
    near = np.zeros((2, H, W))
    near[0, 5, 5] = 2.                                                            # the flow is already within a pixel of the match
    assert not fm.select(qA, qB, d_ab, c1, d_ba, near, 8, r, 128)[0].any()
    # and in the propagation: the neighbour's displacement is taken below the equality only
    B = np.zeros((H, W, 3), np.uint8)
    B[5, 8] = (125, 125, 125)                                                     # C((5, 5), (3, 0)) = 3 * 125 = 375 against A's 750
    qB = fm.quantise(B)
    ccur = np.full((H, W), 750, np.int32)
    seeded = np.zeros((H, W), np.uint8)
    seeded[5, 4] = 1
    cand = np.zeros((H, W, 2), np.int32)
    cand[5, 4] = (3, 0)
    d = np.zeros((H, W, 2), np.int32)
    d[...] = (3, 0)
    assert fm.cost_at(qA, qB, d, r)[5, 5] == 375
    s, _ = fm.propagate(qA, qB, seeded, cand, ccur, r, 128)
    assert not s[5, 5]                                                            # 256 * 375 = 128 * 750: not below
    s, c = fm.propagate(qA, qB, seeded, cand, ccur, r, 129)
    assert s[5, 5] and tuple(c[5, 5]) == (3, 0)


def test_select_rounds_half_to_even_clips_and_prices_a_flow_that_leaves_the_frame():
    H, W = 8, 9
    q = fm.quantise(_texture(H, W, 7))
    uv = np.zeros((2, H, W), np.float32)
    uv[0, 0, 0], uv[0, 0, 1], uv[0, 0, 2], uv[1, 3, 3], uv[0, 4, 4] = 0.5, 1.5, 2.5, -0.5, 40.
    z = np.zeros((H, W, 2), np.int32)
    _, cand, ccur = fm.select(q, q, z, np.full((H, W), 10 ** 6, np.int32), z, uv, 5, 2, 230)          # (a cost no flow is worse than: unseeded)
    assert [int(cand[0, k, 0]) for k in range(3)] == [0, 2, 2] and cand[3, 3, 1] == 0 and cand[4, 4, 0] == 5
    assert ccur[4, 4] == fm.max_cost(2) == 25 * 765 and ccur[0, 0] == 0


def test_propagation_is_jacobi_and_a_seeded_pixel_never_changes():
    H, W, r = 9, 20, 1
    big = _texture(H, W + 6, 8)
    A, B = big[:, :W], big[:, 6:]                                                # A(p) = B(p + (-6, 0))
    qA, qB = fm.quantise(A), fm.quantise(B)
    seeded = np.zeros((H, W), np.uint8)
    seeded[4, 12] = 1
    cand = np.zeros((H, W, 2), np.int32)
    cand[4, 12] = (-6, 0)
    ccur = fm.cost_at(qA, qB, np.zeros((H, W, 2), np.int32), r)
    s, c = seeded, cand
    for k in range(1, 4):
        s, c = fm.propagate(qA, qB, s, c, ccur, r, 230)
        ys, xs = np.nonzero(s)
        assert (np.abs(ys - 4) + np.abs(xs - 12)).max() == k                      # one ring per iteration
        assert (c[s.astype(bool)] == (-6, 0)).all()
    assert s.sum() == 1 + 4 + 8 + 12


def test_levels_and_limits():
    assert fm.pick_level(vr.level_shapes(96, 128)) == 0 and fm.pick_level(vr.level_shapes(64, 80)) == 0
    assert fm.pick_level(vr.level_shapes(480, 854)) == 1 and fm.pick_level(vr.level_shapes(1080, 1920)) == 2
    assert fm.pick_level(vr.level_shapes(512, 512)) == 0 and fm.pick_level(vr.level_shapes(513, 20)) == 0      # one level: the coarsest
    assert fm.pick_level(vr.level_shapes(480, 854), 0) == 0
    for bad in (dict(R=0), dict(R=33), dict(patch=0), dict(patch=4), dict(prop=65), dict(prop=-1), dict(level=-2), dict(kappa=0.),
                dict(kappa=1.5), dict(kappa=float('nan'))):
        with pytest.raises(AssertionError):
            fm.check(**dict(dict(R=24), **bad))
    assert fm.check(24) == (24, 2, -1, 230, 16) and fm.check(32, 3, 2, 1., 64) == (32, 3, 2, 256, 64)
    level = np.array([[[0., 1., 0.5], [0.002, 0.998, 1.2], [-0.1, 0.4999, 0.1]]], np.float32)
    assert fm.unpack(fm.quantise(level)).tolist() == [[[0, 255, 128], [1, 254, 255], [0, 127, 26]]]     # 127.5 -> 128: half to even
    assert fm.quantise(_texture(4, 5, 9)).dtype == np.uint32


# ---- the restatement on the fixtures --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', fm.DARTS)
def test_the_stage_recovers_a_small_fast_object(name):
    p = fm.fixture(name)
    obj, bg = fm.object_region(p), fm.background_region(p)
    plain, (f_ab, f_ba) = fm.plain(name), fm.matched(name)
    e_plain, e_match = vr.epe(plain, p.truth_ab, obj), vr.epe(f_ab, p.truth_ab, obj)
    b_plain, b_match = vr.epe(plain, p.truth_ab, bg), vr.epe(f_ab, p.truth_ab, bg)
    e_back = vr.epe(f_ba, p.truth_ba, vr.erode(p.maskB, 2))
    print('%s: object %d px, zero flow %.2f; plain %.3f px -> %.4f px with the stage (B -> A: %.4f); background %.4f -> %.4f px'
          % (name, int(obj.sum()), vr.epe(np.zeros_like(plain), p.truth_ab, obj), e_plain, e_match, e_back, b_plain, b_match))
    assert obj.sum() == 33 and bg.sum() > 9000
    assert e_plain > 10
    assert e_match <= 1 and e_match <= 0.05 * e_plain
    assert e_back <= 1                                                             # both directions share the two searches
    assert b_match <= 0.1
    assert e_match <= 0.5                                                         # (the issue: else another seed)


@pytest.mark.parametrize('name', [n for n in vr.FIXTURES if n != 'tiny'])
def test_the_existing_fixtures_stay_under_their_bar_with_the_stage(name):
    p = vr.fixture(name)
    region = vr.score_region(p) if p.truth_ab is not None else None
    got, was = vr.epe(fm.matched(name)[0], p.truth_ab, region), vr.epe(vr.restated(name)[0], p.truth_ab, region)
    print('%s: %.4f px with the stage, %.4f px without' % (name, got, was))
    assert got < 0.1


def test_the_stage_leaves_the_one_level_plumbing_case_alone():
    assert np.array_equal(fm.matched('tiny')[0], vr.restated('tiny')[0])


def test_the_hook_is_the_only_difference_to_the_two_flows():
    import robustflow_restated as rr
    p = vr.fixture('odd')
    assert np.array_equal(fm.flow_planar(p.imgA, p.imgB), vr.flow_planar(p.imgA, p.imgB))
    assert np.array_equal(fm.flow_planar(p.imgA, p.imgB, None, np.float64, 5., 1.), rr.flow_planar(p.imgA, p.imgB))
    seen = []
    fm.flow_planar(p.imgA, p.imgB, lambda lev, uv: seen.append((lev, uv.shape, bool(uv.any()))) or uv)
    assert seen == [(1, (2, 19, 27), False), (0, (2, 37, 53), True)]              # the zero field of the coarsest level first


# ---- the flags ----------------------------------------------------------------------------------------------------------------------

def _scripts():
    import auto_gen
    import auto_mask
    import propagate_mask as pm
    return {auto_gen: ['--datapath', 'd/JPEGImages/x/'], pm: ['--datapath', 'd/JPEGImages/x/', '--key', '0:a.png'],
            auto_mask: ['--datapath', 'd/JPEGImages/x/']}


def _stage(a):
    return (a.vf_match, a.vf_match_patch, a.vf_match_level, a.vf_match_kappa, a.vf_match_prop)


def test_the_three_scripts_parse_the_flags_and_refuse_bad_values(capsys):
    for mod, argv in _scripts().items():
        assert _stage(mod.parse_args(argv)) == (0, 2, -1, 0.9, 16)
        a = mod.parse_args(argv + ['--flow_method', 'variational', '--vf_match', '24'])
        assert _stage(a) == (24, 2, -1, 0.9, 16)
        a = mod.parse_args(argv + ['--vf_match', '32', '--vf_match_patch', '3', '--vf_match_level', '1', '--vf_match_kappa', '1', '--vf_match_prop', '64'])
        assert _stage(a) == (32, 3, 1, 1., 64)
        assert mod.parse_args(argv + ['--vf_match_prop', '0']).vf_match_prop == 0
        for bad in (['--vf_match', '33'], ['--vf_match', '-1'], ['--vf_match', '2.5'], ['--vf_match_patch', '0'], ['--vf_match_patch', '4'],
                    ['--vf_match_level', '-2'], ['--vf_match_kappa', '0'], ['--vf_match_kappa', '1.01'], ['--vf_match_kappa', 'nan'],
                    ['--vf_match_prop', '65'], ['--vf_match_prop', '-1']):
            with pytest.raises(SystemExit):
                mod.parse_args(argv + bad)
            assert 'vf_match' in capsys.readouterr().err


def test_variational_flow_fn_routes_to_the_stage_only_when_it_is_on(monkeypatch):
    import auto_gen
    seen = []

    def make(**over):
        seen.append(over)
        return lambda a, b: (np.zeros(a.shape[:2] + (3,), np.float32), np.zeros(a.shape[:2], np.float32))
    auto_gen.variational_flow_fn(auto_gen.parse_args(['--flow_method', 'variational', '--vf_NI', '6']), make)
    auto_gen.variational_flow_fn(auto_gen.parse_args(['--flow_method', 'variational', '--vf_NI', '6', '--vf_match_patch', '3']), make)
    assert seen == [dict(vr.DEFAULTS, NI=6)] * 2                                  # today's call: no keyword of the stage
    auto_gen.variational_flow_fn(auto_gen.parse_args(['--vf_gamma', '5', '--vf_match', '0']), make)
    assert seen[-1] == dict(vr.DEFAULTS, gamma=5., beta=1.)
    auto_gen.variational_flow_fn(auto_gen.parse_args(['--vf_match', '24', '--vf_match_prop', '8', '--vf_NW', '3']), make)
    assert seen[-1] == dict(vr.DEFAULTS, NW=3, match=24, patch=2, level=-1, kappa=0.9, prop=8, gamma=0., beta=1.)
    auto_gen.variational_flow_fn(auto_gen.parse_args(['--vf_match', '16', '--vf_gamma', '5', '--vf_beta', '2']), make)
    assert seen[-1] == dict(vr.DEFAULTS, match=16, patch=2, level=-1, kappa=0.9, prop=16, gamma=5., beta=2.)
    img = np.zeros((20, 30, 3), np.uint8)
    f, o = auto_gen.variational_flow_fn(auto_gen.parse_args(['--vf_match', '24', '--testres', '0.5']), make)(img, img)
    assert f.shape == (20, 30, 3) and o.shape == (20, 30)
    # without `make`, each flow's own factory is taken
    import flow_match
    import robust_flow
    from lasr_amd.nnutils import varflow
    monkeypatch.setattr(flow_match, 'make_flow_fn', lambda **kw: ('match', kw))
    monkeypatch.setattr(robust_flow, 'make_flow_fn', lambda **kw: ('robust', kw))
    monkeypatch.setattr(varflow, 'make_flow_fn', lambda **kw: ('plain', kw))
    assert auto_gen.variational_flow_fn(auto_gen.parse_args(['--vf_match', '24']))[0] == 'match'
    assert auto_gen.variational_flow_fn(auto_gen.parse_args(['--vf_gamma', '5'])) == ('robust', dict(vr.DEFAULTS, gamma=5., beta=1.))
    assert auto_gen.variational_flow_fn(auto_gen.parse_args([])) == ('plain', dict(vr.DEFAULTS))


def test_a_default_propagate_argv_is_unchanged_and_the_flags_are_handed_on_when_set():
    import auto_mask
    import propagate_mask as pm
    base = ['--datapath', 'd/JPEGImages/x/', '--flow_method', 'variational']
    plain = auto_mask.propagate_argv(auto_mask.parse_args(base), {0: 'k.png'})
    assert not any('vf_match' in t for t in plain)                                # a default run prints the line it always printed
    assert _stage(pm.parse_args(plain)) == (0, 2, -1, 0.9, 16)
    argv = auto_mask.propagate_argv(auto_mask.parse_args(base + ['--vf_match', '24', '--vf_match_kappa', '0.8']), {0: 'k.png'})
    assert _stage(pm.parse_args(argv)) == (24, 2, -1, 0.8, 16)
    assert [t for t in argv if 'vf_match' in t] == ['--vf_match', '--vf_match_kappa']
    assert [t for t in argv if t not in ('--vf_match', '24', '--vf_match_kappa', '0.8')] == plain


def test_reconstruct_hands_the_flags_to_all_three_steps_and_reports_the_caveat(tmp_path):
    from lasr_amd import pipeline as pl
    from test_reconstruct_cpu import by_name, load, make_args
    extra = ['--', '--vf_match', '24', '--vf_match_prop', '8']
    steps = by_name(pl.plan(make_args(tmp_path, *extra)))
    assert _stage(load('preprocess', 'auto_mask.py').parse_args(list(steps['masks'].argv[2:]))) == (24, 2, -1, 0.9, 8)
    for name in ('flow-r', 'flow'):
        assert load('preprocess', 'auto_gen.py').parse_args(list(steps[name].argv[2:])).vf_match == 24
    key = str(tmp_path / 'k.png')
    masks = by_name(pl.plan(make_args(tmp_path, '--key', '2:' + key, *extra)))['masks']
    assert load('preprocess', 'propagate_mask.py').parse_args(list(masks.argv[2:])).vf_match == 24
    # the default plan is the parent's: no step names the flag, no caveat is added
    plain = pl.plan(make_args(tmp_path))
    assert not any('vf_match' in t for s in plain if s.argv for t in s.argv)
    assert 'large_displacement' not in pl.describe(make_args(tmp_path))['pieces']
    assert 'large_displacement' not in pl.describe(make_args(tmp_path, '--', '--vf_match', '0'))['pieces']
    assert 'large_displacement' not in pl.describe(make_args(tmp_path, '--', '--vf_match_prop', '8'))['pieces']
    pieces = pl.describe(make_args(tmp_path, *extra))['pieces']
    assert pieces.index('large_displacement') == pieces.index('variational') + 1
    both = pl.describe(make_args(tmp_path, '--', '--vf_match=24', '--vf_gamma', '5'))['pieces']
    assert both.index('gradient_constancy') < both.index('large_displacement')
    assert 'unverified on real footage' in pl.CAVEATS['large_displacement'] and 'not on' in pl.CAVEATS['large_displacement']
    assert [s.timeout_s for s in plain] == [s.timeout_s for s in pl.plan(make_args(tmp_path, *extra))]


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------

def test_header_and_binding_agree_on_the_four_entry_points():
    from lasr_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'lasr_ops.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    kinds = {'int': _lib._i, 'float': _lib._f}
    for name in ENTRY_POINTS:
        args = re.search(r'int\s+%s\s*\((.*?)\)\s*;' % name, hdr, re.S).group(1)
        want = [_lib._p if '*' in a else kinds[a.split()[0]] for a in args.split(',')]
        res, got = _lib.SIGNATURES[name]
        assert res is _lib._i and got == want, name
    assert '#define LASR_FLOWMATCH_MAX_R 32\n' in hdr and '#define LASR_FLOWMATCH_MAX_PATCH 3\n' in hdr
    assert (_lib.FLOWMATCH_MAX_R, _lib.FLOWMATCH_MAX_PATCH) == (32, 3) == (fm.MAX_R, fm.MAX_PATCH)
    assert sorted(n for n in _lib.SIGNATURES if n.startswith('lasr_flowmatch_')) == sorted(ENTRY_POINTS)
    assert _lib.ABI_VERSION == 13                                                 # new symbols only


def test_symbols_are_exported_and_the_host_checks_run_without_a_device():
    from lasr_amd import _lib
    h = _lib.lib()
    n = None
    p = [1 << 20, 1 << 21, 1 << 22, 1 << 23, 1 << 24, 1 << 25, 1 << 26, 1 << 27, 1 << 28]     # non-null addresses; no launch reads them
    BAD = -1
    sizes = ((1, 8), (8, 1), (0, 0), (-1, 8), (16385, 8), (8, 16385))

    def quantise(img=p[0], level=n, out=p[1], H=8, W=9):
        return h.lasr_flowmatch_quantise(img, level, out, H, W, n)
    assert quantise(img=n) == BAD and quantise(level=p[2]) == BAD and quantise(out=n) == BAD and quantise(out=p[0]) == BAD

    def search(qA=p[0], qB=p[1], d=p[2], c1=p[3], H=8, W=9, R=24, r=2):
        return h.lasr_flowmatch_search(qA, qB, d, c1, H, W, R, r, n)
    for k in ('qA', 'qB', 'd', 'c1'):
        assert search(**{k: n}) == BAD, k
    assert search(c1=p[2]) == BAD and search(d=p[0]) == BAD and search(c1=p[1]) == BAD
    assert search(R=0) == BAD and search(R=33) == BAD and search(r=0) == BAD and search(r=4) == BAD

    names = ('qA', 'qB', 'd_ab', 'c1', 'd_ba', 'uv', 'seeded', 'cand', 'ccur')

    def select(H=8, W=9, R=24, r=2, K=230, **kw):
        a = dict(zip(names, p))
        a.update(kw)
        return h.lasr_flowmatch_select(*[a[k] for k in names], H, W, R, r, K, n)
    for k in names:
        assert select(**{k: n}) == BAD, k
    assert select(cand=p[8]) == BAD and select(cand=p[2]) == BAD and select(ccur=p[3]) == BAD
    assert select(R=0) == BAD and select(R=33) == BAD and select(r=4) == BAD and select(K=0) == BAD and select(K=257) == BAD

    pnames = ('qA', 'qB', 'seeded_in', 'cand_in', 'ccur', 'seeded_out', 'cand_out')

    def propagate(H=8, W=9, r=2, K=230, **kw):
        a = dict(zip(pnames, p))
        a.update(kw)
        return h.lasr_flowmatch_propagate(*[a[k] for k in pnames], H, W, r, K, n)
    for k in pnames:
        assert propagate(**{k: n}) == BAD, k
    assert propagate(seeded_out=p[2]) == BAD and propagate(cand_out=p[3]) == BAD and propagate(cand_out=p[4]) == BAD
    assert propagate(r=0) == BAD and propagate(r=4) == BAD and propagate(K=0) == BAD and propagate(K=257) == BAD
    for H, W in sizes:
        assert quantise(H=H, W=W) == BAD and search(H=H, W=W) == BAD and select(H=H, W=W) == BAD and propagate(H=H, W=W) == BAD
    table = [h.lasr_prof_kernel_name(i) for i in range(h.lasr_prof_kernel_count())]
    assert not any(b'flowmatch' in x for x in table)                              # the kernel-name table is not extended


def test_python_layer_refuses_cpu_tensors_and_bad_parameters():
    import torch
    mod = flowmatch_guarded.flow_match()
    img = torch.zeros(8, 9, 3, dtype=torch.uint8)
    q, d, c = torch.zeros(8, 9, dtype=torch.int32), torch.zeros(8, 9, 2, dtype=torch.int32), torch.zeros(8, 9, dtype=torch.int32)
    s, uv = torch.zeros(8, 9, dtype=torch.uint8), torch.zeros(2, 8, 9)
    for call in (lambda: mod.quantise(img), lambda: mod.search(q, q, 24), lambda: mod.select(q, q, d, c, d, uv, 24),
                 lambda: mod.propagate(q, q, s, d, c), lambda: mod.fuse(q, q, d, c, d, uv, 24), lambda: mod.flow_pair(img, img, 24),
                 lambda: mod.matches(img, img, 24)):
        with pytest.raises(TypeError, match='only cuda'):
            call()
    with pytest.raises(TypeError):
        mod.flow_pair(img.numpy(), img.numpy(), 24)
    with pytest.raises(TypeError, match='unknown parameters'):
        mod.make_flow_fn(match=24, Q=5)
    for bad in (dict(match=0), dict(match=33), dict(match=2.5), dict(patch=0), dict(patch=4), dict(level=-2), dict(kappa=0.),
                dict(kappa=1.5), dict(kappa=float('nan')), dict(prop=65), dict(prop=-1), dict(alpha=0.), dict(NI=0),
                dict(gamma=-1.), dict(gamma=float('inf'))):
        with pytest.raises(ValueError):
            mod.make_flow_fn(**dict(dict(match=24), **bad))
    assert mod.DEFAULTS == fm.DEFAULTS and (mod.MAX_PROP, mod.LEVEL_SIDE) == (fm.MAX_PROP, fm.LEVEL_SIDE)
    assert mod.check(24) == fm.check(24) and mod.check(32, 3, 2, 1., 64) == fm.check(32, 3, 2, 1., 64)
    for H, W in ((96, 128), (480, 854), (1080, 1920), (513, 20)):
        assert mod.pick_level(vr.level_shapes(H, W)) == fm.pick_level(vr.level_shapes(H, W))
    with pytest.raises(ValueError):
        mod.pick_level(vr.level_shapes(96, 128), 3)


# ---- the native scan ----------------------------------------------------------------------------------------------------------------

def test_every_native_flow_match_launches_is_in_the_guarded_case():
    with open(os.path.join(ROOT, 'preprocess', 'flow_match.py')) as fh:
        names, opaque = launched_in(fh.read())
    assert not opaque and sorted(set(names)) == sorted(flowmatch_guarded.CASE.natives) == sorted(ENTRY_POINTS)
