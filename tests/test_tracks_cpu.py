"""Dense point tracks without a device: closed forms of the float64 restatement (tests/tracks_restated.py) on a hand-made raster,
the undecided share of the fixture tests/test_tracks_gpu.py compares on, the C ABI's host-side checks, the Python layer's refusal
of CPU tensors and the script's argument handling."""
import os
import sys

import numpy as np
import pytest

import tracks_cases as tc
import tracks_restated as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = tc.H, tc.W


def _track(verts, faces, K, queries, snap_radius=0, window=1):
    planes = tc.face_index(verts, faces, K)
    anc = tr.anchor(verts, faces, K, planes, queries, H, W, snap_radius)
    return anc, tr.project(verts, faces, K, planes, anc, H, W, window), planes


def test_restatement_translating_quad_closed_form():
    verts, faces, K = tc.quad_case()
    q = tc.quad_queries()
    anc, (tracks, state, _), _ = _track(verts, faces, K, q)
    want = tc.quad_closed_form(q)
    assert (anc['face'] >= 0).all() and np.abs(anc['bary'].sum(1) - 1).max() <= 1e-15
    # float32 vertices of a plane z = const: the restatement follows the analytic projection to float32's rounding of the inputs
    assert np.abs(tracks - want).max() <= 1e-5
    inside = (want[..., 0] >= 0) & (want[..., 0] < W) & (want[..., 1] >= 0) & (want[..., 1] < H)
    assert (state[inside] == 1).all() and (state[~inside] == 3).all()
    assert (~inside).sum() >= 10 and inside[:, 0].all()                   # a part of the quad does leave the frame
    assert np.abs(tracks[:, 0] - q[:, [2, 1]]).max() <= 1e-5              # frame 0 returns the query, (u, v) from (t, v, u)


def test_restatement_snapping_and_the_tie_rule():
    verts, faces, K = tc.quad_case()
    q = np.array([[0., 23.5, 12.5], [0., 24.0, 12.5], [0., 23.5, 30.5]])  # 2 px left of the outline; equidistant from two; covered
    anc, (tracks, state, _), planes = _track(verts, faces, K, q, snap_radius=3)
    assert planes[0, 23, 13] == -1 and planes[0, 23, 14] >= 0 and planes[0, 24, 14] >= 0
    assert (anc['face'] >= 0).all()
    assert (anc['snapped'] == np.array([[23.5, 14.5], [23.5, 14.5], [23.5, 30.5]])).all()
    assert np.abs(tracks[:2, 0] - (14.5, 23.5)).max() <= 1e-5 and (state[:, 0] == 1).all()
    anc, (tracks, state, _), _ = _track(verts, faces, K, q, snap_radius=1)
    assert (anc['face'][:2] == -1).all() and (state[:2] == 0).all() and np.isnan(tracks[:2]).all()
    assert (anc['snapped'][:2] == q[:2, 1:]).all() and state[2, 0] == 1


@pytest.mark.parametrize('w', [0, 1])
def test_restatement_occluder_rectangle(w):
    verts, faces, K = tc.occluder_case()
    q = tc.occluder_queries()
    anc, (tracks, state, _), _ = _track(verts, faces, K, q, window=w)
    assert np.isin(anc['face'], (0, 1)).all()                             # every query starts on the far quad
    assert np.abs(tracks - q[:, None, [2, 1]]).max() <= 1e-5              # which stands still
    hidden = shown = 0
    for t in range(verts.shape[0]):
        d = tc.inside_by(tracks[:, t, 0], tracks[:, t, 1], tc.occluder_rect(t))
        assert (state[d > w + 1, t] == 2).all() and (state[d < -1, t] == 1).all()
        hidden, shown = hidden + (d > w + 1).sum(), shown + (d < -1).sum()
    assert hidden >= 10 and shown >= 100


def test_restatement_rotating_octahedron():
    verts, faces, K = tc.octahedron_case()
    planes = tc.face_index(verts, faces, K)
    q = tc.centres(planes[0] >= 0, 0)[::7]
    anc = tr.anchor(verts, faces, K, planes, q, H, W)
    tracks, state, _ = tr.project(verts, faces, K, planes, anc, H, W)
    assert len(q) >= 20 and (anc['face'] >= 0).all()
    flipped_any = 0
    for i in range(len(q)):
        ndp = tc.octahedron_n_dot_p(anc['face'][i], anc['bary'][i])
        assert (np.abs(ndp) > 0.02).all()                                 # no frame is edge-on: |n| |P| is about 0.6 * 4
        flipped = np.sign(ndp) != np.sign(ndp[0])
        assert anc['facing'][i] == np.sign(ndp[0])
        assert (state[i][flipped] == 2).all() and (state[i][~flipped] == 1).all()
        flipped_any += flipped.any()
    assert flipped_any == len(q)                                          # half a turn: every front point ends at the back


def test_restatement_splat_overlap_and_blend():
    frames, tracks, state, colors = tc.splat_case()
    out, keys = tr.splat(frames, tracks, state, colors, 2)
    Q = len(colors)
    assert keys[0, 30, 20] == Q and keys[0, 28, 20] == Q and keys[0, 30, 23] < Q       # the later of the two queries; radius 2
    assert (keys[1, :3, :3] > 0).sum() >= 6                                             # the disc at the corner is clipped
    c, f = colors[Q - 1].astype(int), frames[0, 30, 20].astype(int)
    assert (out[0, 30, 20] == (192 * c + 63 * f + 127) // 255).all()
    assert (out[keys == 0] == frames[keys == 0]).all()
    out0, keys0 = tr.splat(frames, tracks, state, colors, 0)
    assert ((keys0 > 0).sum((1, 2)) <= (state == 1).sum(0)).all()


def test_undecided_share_of_the_gpu_fixture_is_small():
    verts, faces, K = tc.sphere_case()
    planes = tc.face_index(verts, faces, K)
    q = tc.sphere_queries(planes)
    anc = tr.anchor(verts, faces, K, planes, q, H, W)
    tracks, state, undecided = tr.project(verts, faces, K, planes, anc, H, W)
    counts = [int(((state == s) & ~undecided).sum()) for s in range(5)]
    print('parity case: %d queries, undecided %.3f %%, decided states 0..4: %s' % (len(q), 100 * undecided.mean(), counts))
    assert faces.shape == (320, 3) and verts.shape[0] == 5
    assert (anc['face'] >= 0).all()
    assert undecided.mean() <= 0.02
    assert min(counts[1:4]) >= 20
    # a pixel-centre query returns to itself in its own frame; a sub-pixel one may have been clamped onto the face that owns the
    # centre of its pixel, so it returns to a point of that pixel's face: less than a pixel's diagonal away
    for t in range(5):
        own = q[:, 0] == t
        assert np.abs(tracks[own, t] - q[own][:, [2, 1]]).max() <= (1e-9 if t == 0 else 1.5) and (state[own, t] == 1).all()


def test_symbols_are_exported_and_the_host_checks_run_without_a_device():
    from lasr_amd import _lib
    h = _lib.lib()
    n = None
    anc = lambda t0=0, nf=1, Q=1, V=3, F=1, IS=64, H=48, W=64, snap=0: h.lasr_track_anchor(n, n, n, n, n, n, n, t0, nf, Q, V, F, IS, H,  # noqa: E731
                                                                                            W, snap, n)
    assert anc(nf=0) == 0 and anc(Q=0) == 0                                # nothing to do
    assert anc() == -1                                                     # null buffers
    assert anc(Q=0, snap=-1) == -1 and anc(Q=0, snap=17) == -1 and anc(Q=0, snap=16) == 0
    assert anc(Q=0, H=0) == -1 and anc(Q=0, W=0) == -1 and anc(Q=0, H=65) == -1 and anc(Q=0, W=65) == -1
    assert anc(Q=0, IS=8193, H=1, W=8193) == -1 and anc(Q=0, IS=8192, H=1, W=8192) == 0
    assert anc(Q=0, t0=-1) == -1 and anc(nf=-1) == -1 and anc(Q=-1) == -1 and anc(Q=0, V=0) == -1 and anc(Q=0, F=-1) == -1
    assert anc(Q=0, F=0) == 0 and anc(Q=0, F=(1 << 24) + 1) == -1 and anc(Q=0, t0=1 << 24) == -1
    prj = lambda nf=1, Q=1, V=3, F=1, IS=64, H=48, W=64, w=1: h.lasr_track_project(n, n, n, n, n, n, n, nf, Q, V, F, IS, H, W, w, n)  # noqa: E731
    assert prj(nf=0) == 0 and prj(Q=0) == 0 and prj() == -1
    assert prj(Q=0, w=-1) == -1 and prj(Q=0, w=3) == -1 and prj(Q=0, w=0) == 0 and prj(Q=0, w=2) == 0
    assert prj(Q=0, H=65) == -1 and prj(Q=0, V=0) == -1 and prj(nf=-1) == -1 and prj(Q=-1) == -1
    key = lambda nf=1, Q=1, H=48, W=64, r=2: h.lasr_track_splat_keys(n, n, n, nf, Q, H, W, r, n)                            # noqa: E731
    assert key(nf=0) == 0 and key(Q=0) == 0 and key() == -1
    assert key(Q=0, r=-1) == -1 and key(Q=0, r=9) == -1 and key(Q=0, r=8) == 0 and key(Q=0, H=0) == -1 and key(Q=0, W=8193) == -1
    res = lambda nf=1, Q=1, H=48, W=64: h.lasr_track_splat_resolve(n, n, n, n, nf, Q, H, W, n)                              # noqa: E731
    assert res(nf=0) == 0 and res() == -1 and res(Q=0) == -1 and res(nf=0, H=0) == -1 and res(nf=-1) == -1 and res(nf=0, Q=-1) == -1
    assert (_lib.TRACK_MAX_SNAP, _lib.TRACK_MAX_WINDOW, _lib.TRACK_MAX_RADIUS, _lib.TRACK_MAX_SIZE, _lib.TRACK_SPLAT_ALPHA) == (16, 2, 8, 8192, 192)
    assert tr.SPLAT_ALPHA == _lib.TRACK_SPLAT_ALPHA
    hdr = open(os.path.join(ROOT, 'include', 'lasr_ops.h')).read()
    for name, value in (('MAX_SNAP', '16'), ('MAX_WINDOW', '2'), ('MAX_RADIUS', '8'), ('MAX_SIZE', '8192'), ('SPLAT_ALPHA', '192u')):
        assert '#define LASR_TRACK_%s %s\n' % (name, value) in hdr
    names = [h.lasr_prof_kernel_name(i) for i in range(h.lasr_prof_kernel_count())]
    assert not any(b'track' in x for x in names)                           # these launches stay out of the kernel-name table


def test_python_layer_refuses_cpu_tensors_and_non_tensors():
    import torch
    from lasr_amd.nnutils import tracks
    v, f, K, q = torch.zeros(1, 3, 3), torch.tensor([[0, 1, 2]]), torch.ones(1, 4), torch.zeros(1, 3)
    with pytest.raises(TypeError):
        tracks.track_points(v, f, K, q, 4, 4)
    with pytest.raises(TypeError, match='queries must be a tensor'):
        tracks.track_points(v, f, K, q.numpy(), 4, 4)
    with pytest.raises(TypeError):
        tracks.splat(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), torch.zeros(1, 1, 2), torch.zeros(1, 1, dtype=torch.uint8),
                     torch.zeros(1, 3, dtype=torch.uint8))
    plane = -torch.ones(6, 6)
    plane[2, 4] = plane[3, 3] = plane[4, 4] = 5.
    assert tracks.covered_queries(plane, 3, 1).tolist() == [[3., 2.5, 4.5], [3., 3.5, 3.5], [3., 4.5, 4.5]]
    assert tracks.covered_queries(torch.stack([plane, plane]), 0, 2).tolist() == [[0., 2.5, 4.5], [0., 4.5, 4.5]]
    assert tracks.covered_queries(plane, 0, 1, H=4, W=4).tolist() == [[0., 3.5, 3.5]]
    with pytest.raises(ValueError, match='stride'):
        tracks.covered_queries(plane, 0, 0)


def test_script_arguments_and_topology_check():
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    import export_tracks
    a = export_tracks.parse_args(['--testdir', 'log/camel-5/', '--seqname', 'camel'])
    assert (a.query_frame, a.stride, a.queries, a.snap_radius, a.window, a.outpath, a.preview, a.radius) == (0, 4, '', 0, 1, '', '', 2)
    a = export_tracks.parse_args('--testdir t --seqname s --query_frame 3 --stride 2 --queries q.npy --snap_radius 5 --window 2 '
                                 '--outpath o/tracks.npz --preview p.gif --radius 3'.split())
    assert (a.query_frame, a.stride, a.queries, a.snap_radius, a.window, a.outpath, a.preview, a.radius) == \
        (3, 2, 'q.npy', 5, 2, 'o/tracks.npz', 'p.gif', 3)
    f = np.array([[0, 1, 2], [0, 2, 3]])
    assert (export_tracks.check_topology([f, f.copy()], [0, 1]) == f).all()
    with pytest.raises(ValueError, match='pred7 does not share the topology of pred5'):
        export_tracks.check_topology([f, f, f[:, ::-1]], [5, 6, 7])
    assert export_tracks.summary_line(np.array([[1, 1, 2, 3], [0, 0, 0, 0]], np.uint8)) == \
        'tracked 2 queries, anchored 50.0 %, visible in 50.0 % of the frames on average'
    with pytest.raises(ValueError, match=r'\[Q, 3\]'):
        export_tracks.check_queries(np.zeros((4, 2)), 5)
    with pytest.raises(ValueError, match='frame position'):
        export_tracks.check_queries(np.array([[5., 1., 1.]]), 5)
    assert export_tracks.check_queries(np.array([[4, 1, 1]]), 5).dtype == np.float32
