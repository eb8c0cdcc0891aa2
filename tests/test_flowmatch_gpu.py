"""The large-displacement matching stage of the variational flow on the device (preprocess/flow_match.py, lasr_amd/csrc/flowmatch.hip)
against its restatement (tests/flowmatch_restated.py).  The stage is integer arithmetic from the quantised pixels to the seeded
displacements, so every comparison is torch.equal / np.array_equal: no tolerance anywhere.  The flow that leaves `fuse` holds
either the incoming float32 value, bit for bit, or an integer.

Sizes: 9 x 7 (smaller than the 32 x 8 tile of the search and than every radius), 37 x 53 and 33 x 65 (no multiple of the tile; one
pixel past it each way), 96 x 128 (48 workgroups).  (R, r) = (3, 1), (24, 2), (32, 3): the three patch instantiations of the search
and its largest LDS window.  The quality bars on the device are those of tests/test_flowmatch_cpu.py, with the same numbers.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import flowmatch_guarded
import flowmatch_restated as fr
import guarded
import varflow_restated as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
SIZES = {'9x7': 'tiny', '37x53': 'odd', '33x65': 'seam', '96x128': 'dart33'}
RADII = ((3, 1), (24, 2), (32, 3))


def _fm():
    return flowmatch_guarded.flow_match()


def _vf():
    from lasr_amd.nnutils import varflow
    return varflow


def _dev(cuda, *arrays):
    out = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in arrays)
    return out if len(out) > 1 else out[0]


def _words(q):
    """The restatement's uint32 words as the int32 the device holds (the top byte is 0)."""
    return np.asarray(q).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _restated(name, R, r):
    """(qA, qB, (d_ab, c_ab), (d_ba, c_ba), uv) of the fixture: the restatement's two searches and a float32 flow to select against,
    computed once, shared, left unchanged.  The flow is noise of 4 px with ties of the rounding, values past the radius and a part
    that leaves the frame."""
    p = fr.fixture(name)
    qA, qB = fr.quantise(p.imgA), fr.quantise(p.imgB)
    uv = np.random.default_rng(R * 10 + r).normal(0, 4, (2, p.H, p.W)).astype(np.float32)
    uv[0, 0, :4] = (0.5, 1.5, 2.5, -0.5)
    uv[1, 1, :3] = (-1.5, 40., -40.)
    uv[0, :, -2:] = 3.5
    return qA, qB, fr.search(qA, qB, R, r), fr.search(qB, qA, R, r), uv


@pytest.mark.parametrize('R,r', RADII)
@pytest.mark.parametrize('size', list(SIZES))
def test_every_kernel_equals_the_restatement(cuda, size, R, r):
    fm = _fm()
    name = SIZES[size]
    p = fr.fixture(name)
    qA, qB, (d_ab, c_ab), (d_ba, c_ba), uv = _restated(name, R, r)
    A, B = _dev(cuda, p.imgA, p.imgB)
    tA, tB = fm.quantise(A), fm.quantise(B)
    assert tA.dtype == torch.int32 and tuple(tA.shape) == (p.H, p.W)
    assert np.array_equal(tA.cpu().numpy(), _words(qA)) and np.array_equal(tB.cpu().numpy(), _words(qB))
    # search, both directions, twice
    g_ab, g_ba = fm.search(tA, tB, R, r), fm.search(tB, tA, R, r)
    for (gd, gc), wd, wc, what in ((g_ab, d_ab, c_ab, 'A -> B'), (g_ba, d_ba, c_ba, 'B -> A')):
        assert gd.dtype == torch.int32 and tuple(gd.shape) == (p.H, p.W, 2) and gc.dtype == torch.int32
        bad = int((gd.cpu().numpy() != wd).any(-1).sum())
        print('%s %s R %d r %d %s: %d of %d displacements differ, %d costs' % (size, name, R, r, what, bad, p.H * p.W,
                                                                            int((gc.cpu().numpy() != wc).sum())))
        assert np.array_equal(gc.cpu().numpy(), wc) and np.array_equal(gd.cpu().numpy(), wd)
    again = fm.search(tA, tB, R, r)
    assert torch.equal(again[0], g_ab[0]) and torch.equal(again[1], g_ab[1])
    # select
    K = fr.check(R, r)[3]
    w_s, w_c, w_cc = fr.select(qA, qB, d_ab, c_ab, d_ba, uv, R, r, K)
    tuv = _dev(cuda, uv)
    s, c, cc = fm.select(tA, tB, g_ab[0], g_ab[1], g_ba[0], tuv, R, r, 0.9)
    assert s.dtype == torch.uint8 and c.dtype == torch.int32 and cc.dtype == torch.int32
    print('%s R %d r %d: %d of %d pixels seeded' % (size, R, r, int(w_s.sum()), w_s.size))
    assert np.array_equal(cc.cpu().numpy(), w_cc) and np.array_equal(s.cpu().numpy(), w_s) and np.array_equal(c.cpu().numpy(), w_c)
    assert size == '9x7' or 0 < w_s.sum() < w_s.size
    # propagate: N = 1 and N = 16; N iterations are N single calls; the inputs are left alone
    keep = (s.clone(), c.clone())
    s1, c1 = fm.propagate(tA, tB, s, c, cc, r, 0.9, 1)
    w1 = fr.propagate(qA, qB, w_s, w_c, w_cc, r, K)
    assert np.array_equal(s1.cpu().numpy(), w1[0]) and np.array_equal(c1.cpu().numpy(), w1[1])
    s16, c16 = fm.propagate(tA, tB, s, c, cc, r, 0.9, 16)
    ws, wc = w_s, w_c
    ts, tc = s, c
    for _ in range(16):
        ws, wc = fr.propagate(qA, qB, ws, wc, w_cc, r, K)
        ts, tc = fm.propagate(tA, tB, ts, tc, cc, r, 0.9, 1)
    print('%s R %d r %d: %d seeded after 1 iteration, %d after 16' % (size, R, r, int(w1[0].sum()), int(ws.sum())))
    assert np.array_equal(s16.cpu().numpy(), ws) and np.array_equal(c16.cpu().numpy(), wc)
    assert torch.equal(s16, ts) and torch.equal(c16, tc)
    assert torch.equal(s, keep[0]) and torch.equal(c, keep[1])
    s0, c0 = fm.propagate(tA, tB, s, c, cc, r, 0.9, 0)
    assert torch.equal(s0, s) and torch.equal(c0, c)
    # fuse: the three steps and the apply
    want = fr.fuse(qA, qB, d_ab, c_ab, d_ba, uv, R, r, 0.9, 16)
    got = fm.fuse(tA, tB, g_ab[0], g_ab[1], g_ba[0], tuv, R, r, 0.9, 16)
    assert got.dtype == torch.float32 and want.dtype == np.float32
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert torch.equal(got, fm.fuse(tA, tB, g_ab[0], g_ab[1], g_ba[0], tuv, R, r, 0.9, 16))           # two runs, the same bits


def test_the_quantisation_of_a_coarser_level(cuda):
    fm, vf = _fm(), _vf()
    p = fr.fixture('dart33')
    levels = vr.pyramid(p.imgA, np.float32)
    for lev in (1, 2):
        assert np.array_equal(fm.quantise(_dev(cuda, levels[lev])).cpu().numpy(), _words(fr.quantise(levels[lev])))
    edge = np.array([[[0., 1., 0.5], [0.002, 0.998, 1.2], [-0.1, 0.4999, 0.1]], [[0.5 / 255, 1.5 / 255, 2.5 / 255], [1e-9, -0., 7.]] + [[0.25] * 3]],
                    np.float32)
    assert np.array_equal(fm.quantise(_dev(cuda, edge)).cpu().numpy(), _words(fr.quantise(edge)))
    # through the module's own pyramid: L = 1 at 96 x 128
    A, B = _dev(cuda, p.imgA, p.imgB)
    L, qA, qB, (d_ab, c_ab), (d_ba, c_ba) = fm.matches(A, B, 12, 2, 1)
    wL, wA, wB, (wd_ab, wc_ab), (wd_ba, wc_ba) = fr.matches(p.imgA, p.imgB, 12, 2, 1, np.float32)
    assert L == wL == 1 and tuple(qA.shape) == (48, 64)
    assert np.array_equal(qA.cpu().numpy(), _words(wA)) and np.array_equal(qB.cpu().numpy(), _words(wB))
    assert np.array_equal(d_ab.cpu().numpy(), wd_ab) and np.array_equal(c_ba.cpu().numpy(), wc_ba)
    assert fm.matches(A, B, 12)[0] == 0                                           # -1: the finest level with a longer side <= 512


@pytest.fixture(scope='module')
def fused(cuda):
    """(name, gamma) -> (flow A -> B on the device with the stage [H,W,2], the uv the hook received, the uv it returned)."""
    fm, vf = _fm(), _vf()
    rf = __import__('robustflow_guarded').robust_flow()
    out = {}
    for name in fr.DARTS:
        p = fr.fixture(name)
        A, B = _dev(cuda, p.imgA, p.imgB)
        L, qA, qB, (d_ab, c_ab), (d_ba, c_ba) = fm.matches(A, B, fr.MATCH_R)
        for gamma in (0., 5.):
            seen = []

            def hook(lev, uv):
                if lev != L:
                    return uv
                new = fm.fuse(qA, qB, d_ab, c_ab, d_ba, uv, fr.MATCH_R)
                seen.append((uv.clone(), new.clone()))
                return new
            f = rf.flow(A, B, gamma, 1., hook) if gamma > 0 else vf.flow(A, B, hook)
            assert len(seen) == 1
            out[name, gamma] = (f, seen[0][0], seen[0][1])
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('gamma', [0., 5.])
@pytest.mark.parametrize('name', fr.DARTS)
def test_fuse_inside_the_whole_flow_equals_the_restatement(cuda, fused, name, gamma):
    """The device's incoming uv, as the same float32 array, through the restatement's fuse: the outgoing uv must be bit-equal."""
    p = fr.fixture(name)
    _, uv_in, uv_out = fused[name, gamma]
    L, qA, qB, (d_ab, c_ab), (d_ba, _) = fr.matches(p.imgA, p.imgB, fr.MATCH_R)
    state = {}
    want = fr.fuse(qA, qB, d_ab, c_ab, d_ba, uv_in.cpu().numpy(), fr.MATCH_R, state=state)
    got = uv_out.cpu().numpy()
    print('%s gamma %g: %d pixels seeded, %d of them inside the object' % (name, gamma, int(state['seeded'].sum()),
                                                                          int((state['seeded'].astype(bool) & p.maskA).sum())))
    assert L == 0 and want.dtype == np.float32 and state['seeded'].sum() > 0
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize('gamma', [0., 5.])
@pytest.mark.parametrize('name', fr.DARTS)
def test_the_stage_recovers_a_small_fast_object_on_the_device(cuda, fused, name, gamma):
    fm, vf = _fm(), _vf()
    p = fr.fixture(name)
    obj, bg = fr.object_region(p), fr.background_region(p)
    A, B = _dev(cuda, p.imgA, p.imgB)
    plain = (__import__('robustflow_guarded').robust_flow().flow(A, B, gamma, 1.) if gamma > 0 else vf.flow(A, B)).cpu().numpy()
    f = fused[name, gamma][0].cpu().numpy()
    e_plain, e_match, b_match = vr.epe(plain, p.truth_ab, obj), vr.epe(f, p.truth_ab, obj), vr.epe(f, p.truth_ab, bg)
    print('%s gamma %g on the device: object plain %.3f px -> %.4f px with the stage; background %.4f -> %.4f px'
          % (name, gamma, e_plain, e_match, vr.epe(plain, p.truth_ab, bg), b_match))
    assert e_plain > 10
    assert e_match <= 1 and e_match <= 0.05 * e_plain
    assert b_match <= 0.1
    # flow_pair: the same flow, and the reverse direction from the shared searches
    f_ab, occ_ab, f_ba, occ_ba = fm.flow_pair(A, B, fr.MATCH_R, gamma)
    assert torch.equal(f_ab, fused[name, gamma][0])
    e_back = vr.epe(f_ba.cpu().numpy(), p.truth_ba, vr.erode(p.maskB, 2))
    print('%s gamma %g B -> A: %.4f px' % (name, gamma, e_back))
    assert e_back <= 1 and tuple(occ_ab.shape) == (p.H, p.W) and bool((occ_ab != 0).all()) and bool((occ_ba != 0).all())


def test_without_a_hook_both_flows_are_what_they_were(cuda):
    vf = _vf()
    rf = __import__('robustflow_guarded').robust_flow()
    for name in ('odd', 'dart33'):
        p = fr.fixture(name)
        A, B = _dev(cuda, p.imgA, p.imgB)
        base, base5 = vf.flow(A, B), rf.flow(A, B)
        assert torch.equal(vf.flow(A, B, init=None), base) and torch.equal(vf.flow(A, B, None), base)
        assert torch.equal(vf.flow(A, B, init=lambda lev, uv: uv), base)
        assert torch.equal(rf.flow(A, B, init=None), base5) and torch.equal(rf.flow(A, B, 5., 1., lambda lev, uv: uv), base5)
        assert torch.equal(vf.flow_planar(A, B).permute(1, 2, 0), base)
        f_ab, _, f_ba, _ = vf.flow_pair(A, B)
        assert torch.equal(f_ab, base) and torch.equal(f_ba, vf.flow(B, A))
    # against the float64 restatement, as tests/test_varflow_gpu.py holds the flow: the hook changed no arithmetic
    from test_varflow_cpu import bound
    p = vr.fixture('odd')
    f64, trace = vr.restated('odd')
    b = bound(vr.restated('odd', 'float32')[0], f64)
    out = vr.near_edge(trace, (p.H, p.W), b)
    err = np.abs(vf.flow(*_dev(cuda, p.imgA, p.imgB)).cpu().numpy().astype(np.float64) - f64).max(-1)
    assert err[~out].max() <= b


def test_the_script_runs_the_stage_end_to_end(cuda, fused):
    sys.path.insert(0, os.path.join(ROOT, 'preprocess'))
    import auto_gen
    p = fr.fixture('dart33')
    fn = auto_gen.variational_flow_fn(auto_gen.parse_args(['--flow_method', 'variational', '--vf_match', '24']))
    f, occ = fn(p.imgA, p.imgB)
    assert f.shape == (p.H, p.W, 3) and (f[..., 2] == 1).all() and occ.shape == (p.H, p.W) and (occ != 0).all()
    assert torch.equal(torch.from_numpy(np.ascontiguousarray(f[..., :2])), fused['dart33', 0.][0].cpu())
    e = vr.epe(f[..., :2], p.truth_ab, fr.object_region(p))
    print('dart33 through auto_gen.variational_flow_fn: object %.4f px' % e)
    assert e <= 1
    fn(p.imgB, p.imgA)
    assert fn.stats == dict(computed=1, cached=1)
    # the flag absent: the flow the script always made
    plain = auto_gen.variational_flow_fn(auto_gen.parse_args(['--flow_method', 'variational']))
    f0, _ = plain(p.imgA, p.imgB)
    assert torch.equal(torch.from_numpy(np.ascontiguousarray(f0[..., :2])), _vf().flow(*_dev(cuda, p.imgA, p.imgB)).cpu())
    assert vr.epe(f0[..., :2], p.truth_ab, fr.object_region(p)) > 10
    # with the gradient-constancy term beside it
    fn5 = auto_gen.variational_flow_fn(auto_gen.parse_args(['--flow_method', 'variational', '--vf_match', '24', '--vf_gamma', '5']))
    f5, _ = fn5(p.imgA, p.imgB)
    assert torch.equal(torch.from_numpy(np.ascontiguousarray(f5[..., :2])), fused['dart33', 5.][0].cpu())


def test_the_python_layer_refuses_what_the_host_can_check(cuda):
    fm = _fm()
    q = torch.zeros(8, 9, dtype=torch.int32, device=cuda)
    d, c = torch.zeros(8, 9, 2, dtype=torch.int32, device=cuda), torch.zeros(8, 9, dtype=torch.int32, device=cuda)
    s, uv = torch.zeros(8, 9, dtype=torch.uint8, device=cuda), torch.zeros(2, 8, 9, device=cuda)
    img = torch.zeros(8, 9, 3, dtype=torch.uint8, device=cuda)
    for call in (lambda: fm.search(q, q, 33), lambda: fm.search(q, q, 0), lambda: fm.search(q, q, 8, 4), lambda: fm.search(q, q[:, :8], 8),
                 lambda: fm.search(q.float(), q, 8), lambda: fm.select(q, q, d, c, d, uv, 8, 2, 0.), lambda: fm.select(q, q, c, c, d, uv, 8),
                 lambda: fm.propagate(q, q, s, d, c, 2, 0.9, 65), lambda: fm.propagate(q, q, c, d, c), lambda: fm.quantise(img.int()),
                 lambda: fm.quantise(img[:1, :1]), lambda: fm.flow_pair(img, img, 8, level=5), lambda: fm.flow_pair(img, img[:, :8], 8),
                 lambda: fm.fuse(q, q, d, c, d, uv[:, :4], 8)):
        with pytest.raises(ValueError):
            call()
    assert not fm.search(q, q, 8)[0].any()


# ---- guard bands and relocated inputs -------------------------------------------------------------------------------------------------

def test_the_four_natives_with_guard_bands_and_poison(cuda):
    fm = _fm()
    guarded.run_case(flowmatch_guarded.CASE, cuda, modules=[fm] + guarded._product_modules())


def test_the_four_natives_with_relocated_inputs(cuda):
    fm = _fm()
    record = guarded.run_relocated(flowmatch_guarded.CASE, cuda, modules=[fm] + guarded._product_modules())
    assert sorted(record) == sorted(flowmatch_guarded.NATIVES)
