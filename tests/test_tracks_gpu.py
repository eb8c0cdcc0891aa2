"""Dense point tracks on the device (lasr_amd/nnutils/tracks.py, csrc/tracks.hip) against closed forms and the float64
restatement (tests/tracks_restated.py).  The tracks are this project's own addition: the restatement is the only parity there is.

The bound of 1e-3 px on positions is derived, not measured: at |u| <= 64 px the interpolation, the division, the product and the
sum each round at about 6e-8 relative, and the edge-form barycentrics at about 6e-8 |V|/|edge|; together that is of order 1e-4 px,
and 1e-3 leaves a tenfold margin.  Barycentrics are compared to 1e-5.

Measured on an MI355X (each test prints its figures before it asserts):
  translating quad: 296 queries, max error 7.9e-6 px, 68 entries outside the frame, the nearest 0.018 px from its border.
  round trip: 2187 covered pixel centres, max error 5.7e-6 px.
  occlusion: window 0: 68 entries hidden for certain, 662 visible for certain, 70 in between; window 1: 28 / 662 / 110.
  octahedron: 117 queries, at most 4.8e-6 px from the restatement.
  parity: 1340 queries x 5 frames, undecided share 0.373 % (cap 2 %; tests/test_tracks_cpu.py finds the same 0.373 % with its
    hand-made raster), decided states 1 / 2 / 3: 3125 / 2830 / 720, no state mismatch on decided entries, position error
    8.1e-6 px, barycentric error 1.8e-6 (2.0e-5 with the ray origin at the camera, which is why the anchor shifts it).
  splat: 77 / 918 / 7106 of 9216 pixels drawn at radius 0 / 2 / 8.
  script: 67 queries, all anchored, visible in 60.0 % of the frames; 198 preview pixels drawn, each changed by at least 122 (sum
    over the channels), no other pixel changed.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import tracks_cases as tc
import tracks_restated as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
H, W, IS = tc.H, tc.W, tc.IS
PX = 1e-3


def _tk():
    from lasr_amd.nnutils import tracks
    return tracks


def _dev(cuda, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in arrays]


def _planes(cuda, verts, faces, K):
    """The device raster's own face-index planes [T,IS,IS] (one launch for all frames, as track_points rasterises one chunk)."""
    from lasr_amd.nnutils import bake
    tv, tf, tK = _dev(cuda, verts, faces, K)
    return bake.face_index_raster(tv, tf.int(), tK, IS)[:, 1].cpu().numpy()


def _run(cuda, verts, faces, K, queries, snap_radius=0, window=1):
    tv, tf, tK, tq = _dev(cuda, verts, faces, K, np.asarray(queries, np.float32))
    tracks, state, anc = _tk().track_points(tv, tf, tK, tq, H, W, snap_radius=snap_radius, window=window)
    torch.cuda.synchronize()
    assert tracks.shape == (len(queries), verts.shape[0], 2) and tracks.dtype == torch.float32 and tracks.is_contiguous()
    assert state.shape == (len(queries), verts.shape[0]) and state.dtype == torch.uint8
    return tracks.cpu().numpy(), state.cpu().numpy(), {k: v.cpu().numpy() for k, v in anc.items()}


def test_translating_quad_closed_form(cuda):
    verts, faces, K = tc.quad_case()
    q = tc.quad_queries()
    tracks, state, anc = _run(cuda, verts, faces, K, q)
    want = tc.quad_closed_form(q)
    err = np.abs(tracks - want).max()
    inside = (want[..., 0] >= 0) & (want[..., 0] < W) & (want[..., 1] >= 0) & (want[..., 1] < H)
    margin = min(np.abs(want[..., 0] - W).min(), np.abs(want[..., 0]).min(), np.abs(want[..., 1] - H).min(), np.abs(want[..., 1]).min())
    print('translating quad: %d queries, max error %.3e px, %d entries outside, nearest to the frame border %.3f px'
          % (len(q), err, (~inside).sum(), margin))
    assert (anc['face'] >= 0).all()
    assert err <= PX
    assert margin > PX and (~inside).sum() >= 10
    assert (state[inside] == 1).all() and (state[~inside] == 3).all()


def test_round_trip_on_a_non_square_frame(cuda):
    verts, faces, K = tc.sphere_case()
    assert (H, W) == (48, 64) and K[0, 2] != K[0, 3] and K[0, 0] != K[0, 1]
    planes = _planes(cuda, verts, faces, K)
    worst, total = 0., 0
    for t in (0, 2):
        q = tc.centres(planes[t, :H, :W] >= 0, t)
        tracks, state, anc = _run(cuda, verts, faces, K, q)
        err = np.abs(tracks[:, t] - q[:, [2, 1]]).max()
        worst, total = max(worst, err), total + len(q)
        assert (anc['face'] == planes[t][np.floor(q[:, 1]).astype(int), np.floor(q[:, 2]).astype(int)]).all()
        assert (state[:, t] == 1).all() and err <= PX
        assert (anc['snapped'] == q[:, 1:].astype(np.float32)).all()
    print('round trip: %d covered pixel centres, max error %.3e px' % (total, worst))
    assert total >= 1000


@pytest.mark.parametrize('w', [0, 1])
def test_occlusion(cuda, w):
    verts, faces, K = tc.occluder_case()
    q = tc.occluder_queries()
    tracks, state, anc = _run(cuda, verts, faces, K, q, window=w)
    assert np.isin(anc['face'], (0, 1)).all()
    assert np.abs(tracks - q[:, None, [2, 1]]).max() <= PX                # the far quad stands still
    hidden = shown = 0
    for t in range(verts.shape[0]):
        d = tc.inside_by(q[:, 2], q[:, 1], tc.occluder_rect(t))
        assert (state[d > w + 1, t] == 2).all() and (state[d < -1, t] == 1).all()
        hidden, shown = hidden + int((d > w + 1).sum()), shown + int((d < -1).sum())
    print('occlusion, window %d: %d entries hidden for certain, %d visible for certain, %d in between' % (w, hidden, shown,
                                                                                                         state.size - hidden - shown))
    assert hidden >= 10 and shown >= 100


def test_back_faces_of_a_turning_octahedron(cuda):
    verts, faces, K = tc.octahedron_case()
    planes = _planes(cuda, verts, faces, K)
    q = tc.centres(planes[0, :H, :W] >= 0, 0)[::7]
    tracks, state, anc = _run(cuda, verts, faces, K, q)
    ranc = tr.anchor(verts, faces, K, planes, q, H, W)
    rtracks, rstate, _ = tr.project(verts, faces, K, planes, ranc, H, W)
    assert len(q) >= 20 and (anc['face'] == ranc['face']).all() and (anc['face'] >= 0).all()
    err = np.abs(tracks - rtracks).max()
    print('octahedron: %d queries, max distance from the restatement %.3e px' % (len(q), err))
    assert err <= PX
    for i in range(len(q)):
        ndp = tc.octahedron_n_dot_p(ranc['face'][i], ranc['bary'][i])
        assert (np.abs(ndp) > 0.02).all()                                 # no frame is edge-on
        flipped = np.sign(ndp) != np.sign(ndp[0])
        assert flipped.any() and anc['facing'][i] == np.sign(ndp[0])
        assert (state[i][flipped] == 2).all() and (state[i][~flipped] == 1).all()


@pytest.fixture(scope='module')
def sphere(cuda):
    verts, faces, K = tc.sphere_case()
    planes = _planes(cuda, verts, faces, K)
    q = tc.sphere_queries(planes).astype(np.float32)                      # what the device sees
    anc = tr.anchor(verts, faces, K, planes, q, H, W)
    tracks, state, undecided = tr.project(verts, faces, K, planes, anc, H, W)
    return dict(verts=verts, faces=faces, K=K, planes=planes, q=q, anc=anc, tracks=tracks, state=state, undecided=undecided)


def test_against_the_restatement(cuda, sphere):
    s = sphere
    tracks, state, anc = _run(cuda, s['verts'], s['faces'], s['K'], s['q'])
    ok = ~s['undecided']
    counts = [int(((s['state'] == k) & ok).sum()) for k in range(5)]
    both = ok & np.isin(s['state'], (1, 2, 3))
    perr = np.abs(tracks - s['tracks'])[both].max()
    berr = np.abs(anc['bary'] - s['anc']['bary']).max()
    print('parity: %d queries x %d frames, undecided %.3f %%, decided states 0..4 %s, state mismatches on decided entries %d, '
          'position error %.3e px, barycentric error %.3e'
          % (len(s['q']), state.shape[1], 100 * s['undecided'].mean(), counts, int((state != s['state'])[ok].sum()), perr, berr))
    assert s['undecided'].mean() <= 0.02 and min(counts[1:4]) >= 20
    assert (anc['face'] == s['anc']['face']).all() and (anc['face'] >= 0).all()
    assert berr <= 1e-5
    assert (anc['facing'] == s['anc']['facing'])[~s['anc']['shaky']].all()
    assert (state == s['state'])[ok].all()
    assert perr <= PX
    assert np.isnan(tracks[state == 0]).all() and np.isnan(tracks[state == 4]).all() and not np.isnan(tracks[np.isin(state, (1, 2, 3))]).any()


def test_chunking_and_determinism(cuda, sphere, monkeypatch):
    tk = _tk()
    s = sphere
    tv, tf, tK, tq = _dev(cuda, s['verts'], s['faces'], s['K'], s['q'])
    assert tk.CHUNK_FRAMES >= 5
    a = tk.track_points(tv, tf, tK, tq, H, W)
    b = tk.track_points(tv, tf, tK, tq, H, W)
    monkeypatch.setattr(tk, 'CHUNK_FRAMES', 2)                            # windows of 2, 2 and 1 frames; queries in all of them
    c = tk.track_points(tv, tf, tK, tq, H, W)
    for other in (b, c):
        assert torch.equal(a[0].view(torch.int32), other[0].view(torch.int32)) and torch.equal(a[1], other[1])   # NaN bits too
        for k in a[2]:
            assert torch.equal(a[2][k], other[2][k]), k
    assert (a[1] == 1).float().mean() > 0.3


def test_snapping_and_the_tie_rule(cuda):
    verts, faces, K = tc.quad_case()
    planes = _planes(cuda, verts, faces, K)
    assert planes[0, 23, 13] == -1 and planes[0, 23, 14] >= 0 and planes[0, 24, 14] >= 0 and planes[0, 24, 13] == -1
    q = np.array([[0., 23.5, 12.5], [0., 24.0, 12.5], [0., 23.5, 30.5]])  # 2 px left of the outline; equidistant from two; covered
    tracks, state, anc = _run(cuda, verts, faces, K, q, snap_radius=3)
    assert (anc['face'] == planes[0, 23, [14, 14, 30]]).all()
    assert (anc['snapped'] == np.array([[23.5, 14.5], [23.5, 14.5], [23.5, 30.5]], np.float32)).all()
    assert np.abs(tracks[:, 0] - np.array([[14.5, 23.5], [14.5, 23.5], [30.5, 23.5]])).max() <= PX and (state[:, 0] == 1).all()
    tracks, state, anc = _run(cuda, verts, faces, K, q, snap_radius=1)
    assert (anc['face'][:2] == -1).all() and (state[:2] == 0).all() and np.isnan(tracks[:2]).all()
    assert (anc['snapped'] == q[:, 1:].astype(np.float32)).all() and state[2, 0] == 1 and not np.isnan(tracks[2]).any()


def test_splat_equals_the_restatement(cuda):
    tk = _tk()
    frames, tracks, state, colors = tc.splat_case()
    tfr, ttr, tst, tco = _dev(cuda, frames, tracks, state, colors)
    Q = len(colors)
    for radius in (0, 2, 8):
        want, keys = tr.splat(frames, tracks, state, colors, radius)
        a = tk.splat(tfr, ttr, tst, tco, radius)
        b = tk.splat(tfr, ttr, tst, tco, radius)
        assert torch.equal(a, b)
        assert np.array_equal(a.cpu().numpy(), want)
        assert keys[0, 30, 20] == Q                                       # the highest query index wins the shared pixel
        print('splat radius %d: %d of %d pixels drawn' % (radius, (keys > 0).sum(), keys.size))
    got = tk.splat(tfr, ttr, tst, tco, 2).cpu().numpy()
    assert (got[0, 30, 20] == (192 * colors[Q - 1].astype(int) + 63 * frames[0, 30, 20].astype(int) + 127) // 255).all()


def test_python_layer_validates_its_arguments(cuda):
    tk = _tk()
    verts, faces, K = tc.quad_case()
    tv, tf, tK, tq = _dev(cuda, verts, faces, K, tc.quad_queries().astype(np.float32))
    bad = tf.clone()
    bad[1, 1] = 4
    with pytest.raises(ValueError, match='must index the 4 vertices'):
        tk.track_points(tv, bad, tK, tq, H, W)
    with pytest.raises(ValueError, match=r'queries must be floating point \[Q, 3\]'):
        tk.track_points(tv, tf, tK, tq[:, :2], H, W)
    with pytest.raises(ValueError, match='whole number in 0..3'):
        tk.track_points(tv, tf, tK, tq + torch.tensor([4., 0., 0.], device=cuda), H, W)
    with pytest.raises(ValueError, match='snap_radius'):
        tk.track_points(tv, tf, tK, tq, H, W, snap_radius=17)
    with pytest.raises(ValueError, match='window'):
        tk.track_points(tv, tf, tK, tq, H, W, window=3)
    with pytest.raises(ValueError, match=r'K must be \[T = 4, 4\]'):
        tk.track_points(tv, tf, tK[:3], tq, H, W)
    with pytest.raises(TypeError):
        tk.track_points(tv, tf, tK, tq.cpu(), H, W)
    tracks, state, anc = tk.track_points(tv, tf, tK, tq[:0], H, W)        # no queries: empty outputs, nothing launched
    assert tracks.shape == (0, 4, 2) and state.shape == (0, 4) and anc['face'].shape == (0,)
    raster = tk.frame_raster(tv, tf, tK, 0, H, W)
    got = tk.covered_queries(raster, 0, 3, H, W).cpu().numpy()
    plane = raster[1].cpu().numpy()
    r, c = np.nonzero(plane[:H:3, :W:3] >= 0)
    assert np.array_equal(got, np.stack([np.zeros(len(r)), 3 * r + 0.5, 3 * c + 0.5], 1).astype(np.float32)) and len(got) >= 50


def _write_sequence(root, name, verts, faces, K, frames):
    """What export_tracks.py reads: configs/<name>.config, the frames it lists, and per frame pred<i>.obj and cam<i>.txt (the
    intrinsics in row 3).  Frames are PNGs of a flat colour, so that the GIF's palette holds them exactly."""
    from PIL import Image
    from lasr_amd.soft_renderer.functional import save_obj
    img_dir = os.path.join(root, 'database', 'DAVIS', 'JPEGImages', 'Full-Resolution', name)
    test = os.path.join(root, 'out-' + name)
    os.makedirs(img_dir), os.makedirs(test), os.makedirs(os.path.join(root, 'configs'))
    with open(os.path.join(root, 'configs', '%s.config' % name), 'w') as f:
        f.write('[data]\ndatapath = database/DAVIS/JPEGImages/Full-Resolution/%s/\ndframe = 1\ncan_frame = 0\ninit_frame = 0\n'
                'end_frame = -1\n' % name)
    for i in range(len(verts)):
        Image.fromarray(frames[i]).save(os.path.join(img_dir, '%05d.png' % i))
        save_obj(os.path.join(test, 'pred%d.obj' % i), torch.from_numpy(verts[i]), torch.from_numpy(faces))
        rtk = np.eye(4)
        rtk[3] = K[i]
        np.savetxt(os.path.join(test, 'cam%d.txt' % i), rtk)
    return test


def test_script_end_to_end(cuda, tmp_path):
    from PIL import Image, ImageSequence
    root = str(tmp_path)
    verts, faces, K = tc.sphere_case()
    T = len(verts)
    frames = np.full((T, H, W, 3), 102, np.uint8)
    test = _write_sequence(root, 'ball', verts, faces, K, frames)
    out, gif = os.path.join(root, 'exported', 'tracks.npz'), os.path.join(root, 'preview.gif')
    rc = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'export_tracks.py'), '--testdir', test, '--seqname', 'ball',
                         '--query_frame', '1', '--stride', '4', '--outpath', out, '--preview', gif, '--radius', '0'], cwd=root,
                        timeout=600, capture_output=True, text=True)
    assert rc.returncode == 0, rc.stderr[-2000:]
    print(rc.stdout.strip())
    z = np.load(out)
    assert sorted(z.files) == ['frame_ids', 'queries', 'size', 'state', 'tracks', 'visible']
    Q = z['queries'].shape[0]
    assert Q >= 40 and z['queries'].shape == (Q, 3) and z['queries'].dtype == np.float32 and (z['queries'][:, 0] == 1).all()
    assert ((z['queries'][:, 1:] - 0.5) % 4 == 0).all()
    assert z['tracks'].shape == (Q, T, 2) and z['tracks'].dtype == np.float32
    assert z['visible'].shape == (Q, T) and z['visible'].dtype == np.bool_ and z['state'].dtype == np.uint8
    assert np.array_equal(z['visible'], z['state'] == 1) and z['visible'][:, 1].all()
    assert np.array_equal(z['frame_ids'], np.arange(T)) and tuple(z['size']) == (H, W)
    assert np.abs(z['tracks'][:, 1] - z['queries'][:, [2, 1]]).max() <= PX
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    import export_tracks
    lines = rc.stdout.splitlines()
    assert lines[0] == export_tracks.summary_line(z['state']) and lines[0].startswith('tracked %d queries, anchored 100.0 %%' % Q)
    assert lines[1] == 'wrote %d frames to %s' % (T, gif)

    g = Image.open(gif)
    assert g.n_frames == T and g.size == (W, H)
    shown = np.stack([np.asarray(fr.convert('RGB')) for fr in ImageSequence.Iterator(g)]).astype(int)
    drawn = np.zeros((T, H, W), bool)
    for t in range(T):
        p = np.floor(z['tracks'][z['visible'][:, t], t]).astype(int)
        drawn[t, p[:, 1], p[:, 0]] = True
    change = np.abs(shown - 102).sum(-1)
    print('preview: %d pixels drawn; smallest change on them %d, largest change elsewhere %d' % (drawn.sum(), change[drawn].min(),
                                                                                               change[~drawn].max()))
    assert drawn.sum() >= 100 and (change[drawn] >= 24).all() and (change[~drawn] <= 6).all()
