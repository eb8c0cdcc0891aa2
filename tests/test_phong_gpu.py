"""lasr_phong_shade (lasr_amd/csrc/phong.hip) and lasr_amd/phong.py on the device: the kernel against the float64 restatement
(tests/phong_restated.py) fed the same face-index maps, culling and depth conventions, the three views of extract.py --render, and
extract.py / scripts/eval_mesh.py --render end to end."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import phong_restated as pr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


@pytest.fixture(scope='module')
def cuda():
    if not torch.cuda.is_available():
        pytest.skip('needs a HIP device')
    return torch.device('cuda:0')


def _phong():
    from lasr_amd import phong
    return phong


def _sphere(rings=16, segments=16, radius=1.):
    from lasr_amd import vis
    v, f = vis.uv_sphere(radius, rings, segments)
    f = vis.fix_inversion(torch.as_tensor(v), f).numpy()
    return v, f


def _check_against_restatement(verts, faces, colors, S, bg=(1., 1., 1.)):
    out, maps = _phong().render(verts, faces, colors, S, background=bg, return_maps=True)
    got = out.cpu().numpy()
    fmap = maps['raster'][:, 1].cpu().numpy()
    assert (fmap >= 0).any()
    for n in range(verts.shape[0]):
        want = pr.shade(verts[n].cpu().double().numpy(), np.asarray(faces), colors[n].cpu().double().numpy(), fmap[n], bg)
        err_rgb = np.abs(got[n, ..., :3] - want[..., :3]).max()
        err_a = np.abs(got[n, ..., 3] - want[..., 3]).max()
        assert err_rgb <= 2e-5 and err_a <= 1e-3, (n, err_rgb, err_a)
    return got, fmap


def test_kernel_matches_the_restatement_on_random_meshes(cuda):
    g = torch.Generator().manual_seed(0)
    for S, F in ((64, 40), (96, 200)):
        N, V = 3, 3 * F
        verts = torch.rand(N, V, 3, generator=g) * torch.tensor([1.6, 1.6, 3.]) + torch.tensor([-0.8, -0.8, 0.5])
        faces = torch.arange(V).view(F, 3)
        colors = torch.rand(N, V, 3, generator=g)
        _check_against_restatement(verts.to(cuda), faces, colors.to(cuda), S, bg=(0.2, 0.5, 1.))


@pytest.mark.parametrize('S', [256, 512])
def test_kernel_matches_the_restatement_on_lasr_sized_meshes(cuda, S):
    v, f = _sphere(36, 36, 0.7)                                              # 2 520 faces
    assert 2400 <= len(f) <= 2600
    g = torch.Generator().manual_seed(1)
    v = torch.as_tensor(v, dtype=torch.float32)
    verts = torch.stack([v * (1 + 0.1 * torch.rand(v.shape[0], 1, generator=g)) + torch.tensor([0.1, -0.05, 3.]),
                         v * torch.tensor([1.2, 0.8, 1.]) + torch.tensor([0., 0., 2.])])
    colors = torch.rand(2, v.shape[0], 3, generator=g)
    got, fmap = _check_against_restatement(verts.to(cuda), f, colors.to(cuda), S)
    assert (fmap >= 0).mean() > 0.3


def _box(a, b, c, z):
    """Closed box of extents a x b x c centred at (0, 0, z), outward winding: verts [8,3], faces [12,3]."""
    v = np.array([[x, y, w] for x in (-a / 2, a / 2) for y in (-b / 2, b / 2) for w in (-c / 2, c / 2)]) + [0, 0, z]
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    f = np.array([t for q in quads for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))])
    from lasr_amd import vis
    return v, vis.fix_inversion(torch.as_tensor(v), f).numpy()


def test_open_box_seen_through_its_missing_face_is_background(cuda):
    v, f = _box(1., 1., 1., 3.)
    vt = torch.as_tensor(v, dtype=torch.float32, device=cuda)[None]
    # the face nearest the camera (z = 2.5) removed: the inner sides of the others face away and are culled
    near_face = [i for i, t in enumerate(f) if np.allclose(v[t][:, 2], 2.5)]
    assert len(near_face) == 2
    opened = np.delete(f, near_face, 0)
    img = _phong().render(vt, opened, torch.full_like(vt, 0.5), 64)[0].cpu().numpy()
    assert np.all(img[..., 3] == 0) and np.all(img[..., :3] == 1)
    closed = _phong().render(vt, f, torch.full_like(vt, 0.5), 64)[0].cpu().numpy()
    assert (closed[..., 3] > 0.5).sum() > 100


def test_closed_sphere_renders_the_same_with_and_without_culling(cuda):
    v, f = _sphere(24, 24, 0.8)
    vt = torch.as_tensor(v, dtype=torch.float32, device=cuda)[None] + torch.tensor([0., 0., 3.], device=cuda)
    col = torch.rand_like(vt)
    a = _phong().render(vt, f, col, 128).cpu().numpy()
    b = _phong().render(vt, f, col, 128, cull_backfaces=False).cpu().numpy()
    assert np.array_equal(a[..., 3] > 0, b[..., 3] > 0) and (a[..., 3] > 0).sum() > 1000
    assert np.abs(a - b).max() <= 1e-5                                        # fp32 rounding where a front face meets the rim


def test_swapping_the_winding_of_one_triangle_removes_it(cuda):
    v = torch.tensor([[[0., 0., 2.], [0.5, 0., 2.], [0., 0.5, 2.]]], device=cuda)
    f = np.array([[0, 2, 1]])                                                 # normal (0, 0, -1): toward the camera
    col = torch.full_like(v, 0.5)
    assert (_phong().render(v, f, col, 64)[0, ..., 3] > 0).sum() > 50
    assert float(_phong().render(v, f[:, [0, 2, 1]], col, 64)[0, ..., 3].max()) == 0.


def test_surface_behind_the_camera_and_beyond_zfar(cuda):
    v, f = _box(1., 1., 1., 3.)
    vt = torch.as_tensor(v, dtype=torch.float32, device=cuda)[None]
    col = torch.full_like(vt, 0.5)
    behind = _phong().render(vt - torch.tensor([0., 0., 10.], device=cuda), f, col, 32)[0].cpu().numpy()
    assert np.all(behind[..., 3] == 0)                                        # z < 0: not drawn
    far = _phong().render(vt + torch.tensor([0., 0., 200.], device=cuda), f, col, 32, background=(0., 1., 0.))[0].cpu().numpy()
    cov = far[..., 3] > 0.6
    assert cov.sum() > 20 and np.allclose(far[cov, :3], [0., 1., 0.], atol=1e-6)


def _silhouette_extent(alpha):
    rows, cols = np.nonzero(alpha > 0)
    return cols.max() - cols.min() + 1, rows.max() - rows.min() + 1


def test_views_of_an_elongated_box_have_the_right_aspect_ratios(cuda):
    import extract
    a, b, c = 0.6, 0.3, 0.45                                                  # extents along x, y, z of the body frame
    v, f = _box(a, b, c, 0.)
    deform = torch.as_tensor(v, dtype=torch.float32, device=cuda)[None]
    R = torch.eye(3, device=cuda)
    T = torch.tensor([0., 0., 40.], device=cuda)
    fl = torch.tensor([40.], device=cuda)                                     # NDC units per unit at depth 40: nearly orthographic
    pp = torch.zeros(1, 2, device=cuda)
    eye = torch.tensor([0., 0., -2.732], device=cuda)
    S = 256
    ext = {}
    for key in ('front', 'right', 'top'):
        if key == 'front':
            cam = deform.matmul(R) + T
        else:
            Rq = extract.quaternion_to_rotation_matrix(torch.tensor([extract.VIEW_QUATS[key]], device=cuda))[0]
            cam = deform.matmul(R.matmul(Rq)) + T
        pv = extract.view_verts(cam, pp, fl, eye, 1. if key == 'front' else extract.VIEW_SHRINK)
        from lasr_amd import vis
        ff = vis.fix_inversion(pv[0], f)
        ext[key] = _silhouette_extent(_phong().render(pv, ff, torch.full_like(pv, 0.5), S)[0, ..., 3].cpu().numpy())
    px = S / 2.                                                               # pixels per NDC unit
    for key, (w, h) in (('front', (a, b)), ('right', (c, b)), ('top', (a, c))):
        s = 1. if key == 'front' else 1. / extract.VIEW_SHRINK
        gw, gh = ext[key]
        assert abs(gw - w * s * px) <= 2 + 0.05 * w * s * px and abs(gh - h * s * px) <= 2 + 0.05 * h * s * px, (key, ext[key])
        assert abs(gw / gh - w / h) <= 2 * (1. / gh + gw / gh ** 2) + 0.03, (key, gw, gh, w / h)


def _iou(a, b):
    return (a & b).sum() / max((a | b).sum(), 1)


@pytest.fixture(scope='module')
def extracted(cuda, tmp_path_factory):
    """extract.export with and without --render on a fresh five-bone model of a rendered sequence, its mean shape pushed out of
    symmetry so that a flipped silhouette differs from the true one."""
    import extract
    import optimize
    from lasr_amd.nnutils import train_utils
    tmp = tmp_path_factory.mktemp('phong_extract')
    root = str(tmp / 'data')
    rc = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'render_syn.py'), '--outdir', 'ph3', '--nframes', '3',
                         '--img_size', '64', '--root', root], cwd=ROOT, timeout=600, capture_output=True, text=True)
    assert rc.returncode == 0, rc.stderr[-2000:]
    os.makedirs(os.path.join(root, 'configs'), exist_ok=True)
    opts = optimize.parse_flags(['--name', 't', '--checkpoint_dir', str(tmp), '--img_size', '64', '--subdivide', '2',
                                 '--n_bones', '5', '--n_hypo', '1', '--batch_size', '1', '--opt_tex', 'yes', '--nouse_gtpose',
                                 '--only_mean_sym', '--noperceptual', '--nouse_graph', '--nosymmetric', '--dataname', 'ph3',
                                 '--data_root', root])
    torch.manual_seed(0)
    tr = train_utils.LASRTrainer(opts).init_training()
    tr.reinit_bones()
    m = tr.module
    with torch.no_grad():
        mv = m.mean_v.data
        bump = (mv[..., 0] > 0) & (mv[..., 1] > 0)                            # one quadrant pushed out: no mirror symmetry
        mv[bump] *= 1.6
    plain, rend = str(tmp / 'plain'), str(tmp / 'render')
    def seeded():                                                            # the loader's pairing order decides each frame's
        import random                                                        # principal point: the same order for both runs
        random.seed(0)
        np.random.seed(0)
        torch.manual_seed(0)
    seeded()
    done0 = extract.export(tr, plain)
    seeded()
    extract.export(tr, plain + '2')                                          # the spread of two runs without --render
    panels = {}
    seeded()
    done1 = extract.export(tr, rend, render=True, panels=panels)
    # the forward's own soft-raster silhouette of each frame, from one more forward of the same batches
    masks = {}
    seeded()                                                                 # the render run's pairs
    tr.model.train()
    with torch.no_grad():
        for batch in tr.dataloader:
            m.iters = 1
            bi = tr.set_input(batch)
            tr.model(bi)
            ids = bi['frameid'].view(-1, 2).t().reshape(-1)
            for k, fid in enumerate(int(x) for x in ids.tolist()):
                masks.setdefault(fid, m.mask_pred.view(len(ids), -1, 64, 64)[k, 0].cpu().numpy())
            if len(masks) >= 3:
                break
    return dict(tr=tr, plain=plain, render=rend, done0=done0, done1=done1, panels=panels, masks=masks, root=root)


def test_extract_render_writes_every_file(extracted):
    import extract
    d = extracted['render']
    fids = sorted(extracted['done1'])
    assert fids == [0, 1, 2] and sorted(extracted['panels']) == fids
    for fid in fids:
        for name in ('render-%05d.png' % fid, 'renderskin-%05d.png' % fid, 'vp2pred%d.ply' % fid, 'vp3pred%d.ply' % fid,
                     'bone%d.ply' % fid):
            assert os.path.getsize(os.path.join(d, name)) > 0, name
        p = extracted['panels'][fid]
        assert p['overlay'].dtype == np.uint8 and p['overlay'].shape == (64, 64, 3)
        for key in ('front', 'right', 'top'):
            assert p[key].shape == (64, 64, 3) and (p[key] < 0.999).any(), key
    can = extract.canonical_frame(extracted['tr'].opts)
    assert can in fids
    for name in ('clusters.obj', 'cpoints.ply', 'skin.npy'):
        assert os.path.exists(os.path.join(d, name)), name
    skin = np.load(os.path.join(d, 'skin.npy'))
    assert skin.shape[0] == 4 and np.allclose(skin.sum(0), 1, atol=1e-5)


def test_front_view_alpha_agrees_with_the_forward_silhouette(extracted):
    for fid, p in extracted['panels'].items():
        ours = p['alpha'] > 0
        sil = extracted['masks'][fid] > 0.5
        iou = _iou(ours, sil)
        mirrored = max(_iou(ours, sil[::-1]), _iou(ours, sil[:, ::-1]))
        assert iou >= 0.98 and mirrored < iou - 0.05, (fid, iou, _iou(ours, sil[::-1]), _iou(ours, sil[:, ::-1]))


def test_turned_views_are_the_closed_form_rotations_of_pred(extracted):
    from lasr_amd.ext_utils.ply import read_ply
    import extract
    d = extracted['render']
    for fid in extracted['done1']:
        pred = read_ply(os.path.join(d, 'pred%d.ply' % fid))['verts']
        rtk = np.loadtxt(os.path.join(d, 'cam%d.txt' % fid))
        T = rtk[:3, 3]
        for name, key in (('vp2pred', 'right'), ('vp3pred', 'top')):
            q = np.asarray(extract.VIEW_QUATS[key]) / np.linalg.norm(extract.VIEW_QUATS[key])
            Rq = extract.quaternion_to_rotation_matrix(torch.tensor([list(q)], dtype=torch.float64))[0].numpy()
            # pred = d R + T, the turned view = d R Rq + T = (pred - T) Rq + T
            want = (pred - T) @ Rq + T
            got = read_ply(os.path.join(d, '%s%d.ply' % (name, fid)))['verts']
            assert np.abs(got - want).max() <= 1e-4 * max(1., np.abs(want).max()), (name, fid)


def test_without_render_the_outputs_are_unchanged(extracted):
    # --render adds files and changes none: each file a run without it writes is what a run with it writes.  Two runs without it
    # already differ in the last digits (the forward's library kernels are not bitwise reproducible), so where they differ the
    # run with it must stay within that spread, and where they agree it must agree byte for byte.
    plain, rend = extracted['plain'], extracted['render']
    names = sorted(os.listdir(plain))
    assert names == sorted(os.listdir(plain + '2'))
    assert all(re.match(r'^(pred\d+\.(obj|ply)|cam\d+\.txt|gauss\d+\.ply)$', n) for n in names), names
    num = re.compile(rb'-?\d+\.?\d*(?:e[-+]?\d+)?')

    def values(path):
        return np.array([float(x) for x in num.findall(open(path, 'rb').read())])
    for n in names:
        a, b, c = (open(os.path.join(d, n), 'rb').read() for d in (plain, plain + '2', rend))
        if a == b:
            assert c == a, n
        else:
            va, vb, vc = values(os.path.join(plain, n)), values(os.path.join(plain + '2', n)), values(os.path.join(rend, n))
            spread = np.abs(va - vb).max()
            assert len(vc) == len(va) and np.abs(vc - va).max() <= max(4 * spread, 1e-5 * np.abs(va).max()), n


def _eval(testdir, gtdir, gif=None):
    args = [sys.executable, os.path.join(ROOT, 'scripts', 'eval_mesh.py'), '--testdir', testdir, '--gtdir', gtdir]
    if gif:
        args += ['--render', '--gif', gif]
    rc = subprocess.run(args, cwd=ROOT, timeout=600, capture_output=True, text=True)
    assert rc.returncode == 0, rc.stderr[-2000:]
    return rc.stdout


def test_eval_mesh_render_images_and_unchanged_scores(cuda, tmp_path):
    from PIL import Image
    import matplotlib
    from lasr_amd.soft_renderer.functional import save_obj
    v, f = _sphere(32, 32, 1.)
    v = v * np.array([1.4, 1., 0.8])
    gt, test, moved = tmp_path / 'gt', tmp_path / 'test', tmp_path / 'moved'
    for d in (gt, test, moved):
        os.makedirs(d)
    save_obj(str(gt / 'a.obj'), torch.as_tensor(v, dtype=torch.float32), torch.as_tensor(f))
    save_obj(str(test / 'pred0.obj'), torch.as_tensor(v, dtype=torch.float32), torch.as_tensor(f))
    w = v.copy()
    region = (v[:, 0] > 0.8)                                                  # one end pushed out
    w[region] *= 1.3
    save_obj(str(moved / 'pred0.obj'), torch.as_tensor(w, dtype=torch.float32), torch.as_tensor(f))
    plain = _eval(str(test), str(gt))
    gif = str(tmp_path / 'out' / 'o.gif')
    rendered = _eval(str(test), str(gt), gif)
    assert plain == rendered
    ims = {k: np.asarray(Image.open(str(test / ('%s-000000.png' % k))).convert('RGB')) for k in ('gt', 'pd', 'cd')}
    assert all(im.shape == (512, 512, 3) for im in ims.values())
    agree = (np.abs(ims['gt'].astype(int) - ims['pd'].astype(int)).max(2) <= 2).mean()
    assert agree >= 0.99, agree
    obj = (ims['gt'] < 250).any(2)
    assert obj.mean() > 0.05
    # the error image in plasma(0) tones: blue-dominant, like the colour map's zero end
    p0 = np.asarray(matplotlib.colormaps['plasma'](0.)[:3])
    cd = ims['cd'][obj].astype(float).mean(0) / 255
    assert cd[2] > cd[0] and cd[2] > cd[1] and p0[2] > p0[0], cd
    g = Image.open(gif)
    assert g.n_frames == 1 and g.size == (3 * 512, 512)
    # a displaced region turns brighter in the error image
    plain_m = _eval(str(moved), str(gt))
    assert plain_m == _eval(str(moved), str(gt), str(tmp_path / 'm.gif'))
    cdm = np.asarray(Image.open(str(moved / 'cd-000000.png')).convert('RGB')).astype(float)
    base = ims['cd'].astype(float)
    assert cdm[obj].sum(1).max() > base[obj].sum(1).max() + 60
