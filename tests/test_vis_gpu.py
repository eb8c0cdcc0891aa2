"""render_vis.py's shading pass on the GPU (lasr_amd/vis.py over csrc/vis.hip): against the numpy restatement on the same
face-index maps, closed-form shading, shadow and transparency cases, and the camera convention end to end."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vis_restated as vr                         # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def cuda():
    if not torch.cuda.is_available():
        pytest.skip('needs a HIP device')
    return torch.device('cuda', 0)


def vis():
    from lasr_amd import vis as v
    return v


def blob(rng, centre, radius, rings=10, segments=14):
    v, f = vis().uv_sphere(1.0, rings, segments)
    r = radius * (1 + 0.25 * rng.standard_normal((1, 3))) * (1 + 0.05 * rng.standard_normal((len(v), 1)))
    return torch.from_numpy(v * r + np.asarray(centre)).float(), torch.from_numpy(f)


def quad(centre, t1, t2, a, b):
    c, t1, t2 = (np.asarray(x, np.float64) for x in (centre, t1, t2))
    v = np.stack([c - a * t1 - b * t2, c + a * t1 - b * t2, c + a * t1 + b * t2, c - a * t1 + b * t2])
    return torch.from_numpy(v).float(), torch.tensor([[0, 1, 2], [0, 2, 3]])


def scene(parts):
    """[(verts, faces, colours [V,3] or (3,))] -> verts, faces, colours concatenated."""
    vs, fs, cs, base = [], [], [], 0
    for v, f, c in parts:
        vs.append(v)
        fs.append(f + base)
        cs.append(torch.as_tensor(c, dtype=torch.float32).expand(len(v), 3))
        base += len(v)
    return torch.cat(vs), torch.cat(fs), torch.cat(cs)


def random_scene(rng, two_layers):
    mesh = blob(rng, (rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.1), 5.0), 0.8)
    cm = torch.from_numpy(rng.uniform(0, 1, (len(mesh[0]), 3))).float()
    floor = vis().floor_quad(mesh[0])
    if two_layers:
        bones = [blob(rng, (rng.uniform(-0.5, 0.5), rng.uniform(-0.4, 0.4), rng.uniform(4.6, 5.4)), 0.25, 6, 8) for _ in range(3)]
        parts = [(b[0], b[1], rng.uniform(0, 1, 3)) for b in bones] + [floor, (mesh[0], mesh[1], cm)]
        n_opaque = sum(len(p[1]) for p in parts[:-1])
    else:
        parts = [(mesh[0], mesh[1], cm), floor]
        n_opaque = None
    v, f, c = scene(parts)
    casters = torch.ones(len(v), dtype=torch.bool)
    fo = sum(len(p[0]) for p in parts[:len(parts) - 2 if two_layers else 1])
    casters[fo:fo + 4] = False                                                 # the floor need not be in the shadow map
    return v, f, c, n_opaque, casters


@pytest.mark.parametrize('smooth', [True, False])
@pytest.mark.parametrize('two_layers', [False, True])
def test_shading_matches_the_restatement(cuda, smooth, two_layers):
    rng = np.random.default_rng(3 + 2 * smooth + two_layers)
    IS, H, W, N = 96, 80, 96, 2
    scenes = [random_scene(rng, two_layers)]
    f = scenes[0][1]
    # one face list per call: frame 1 is frame 0's scene moved and scaled
    verts = torch.stack([scenes[0][0], scenes[0][0] * 1.05 + torch.tensor([0.1, 0.0, 0.2])])
    cols = torch.stack([scenes[0][2], scenes[0][2].flip(1)])
    K = torch.tensor([[120., 110., 47., 41.], [100., 100., 50., 38.]])
    frames = torch.from_numpy(rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8))
    for overlay in (False, True):
        rgb, maps = vis().shade(verts.to(cuda), f.to(cuda), cols.to(cuda), K, IS, H, W, n_opaque=scenes[0][3],
                                casters=scenes[0][4], smooth=smooth, background=(0., 0., 0.) if overlay else (1., 1., 1.),
                                frames=frames.to(cuda) if overlay else None, return_maps=True)
        got = rgb.cpu().numpy().astype(np.int64)
        want, margin = vr.shade(maps, H, W)
        err = np.abs(got - want.astype(np.int64)).max(-1)
        sure = margin > 1e-3                                  # float32 and float64 agree on every shadow tap of these pixels
        assert (~sure).mean() < 0.01
        assert err[sure].max() <= 1, (np.argwhere(err * sure > 1)[:5], err.max())
        cover = maps['raster0'][:, 1, :H, :W].cpu().numpy() >= 0
        assert cover.mean() > 0.3 and len(np.unique(got[cover.nonzero()][:, 0])) > 20     # a real image, not a flat fill
        if two_layers:
            assert (maps["raster1"][:, 1, :H, :W] >= 0).float().mean() > 0.02


def test_pixel_convention_barycentrics_of_covered_pixels(cuda):
    rng = np.random.default_rng(11)
    v, f, c, n_opaque, casters = random_scene(rng, False)
    IS, H, W = 128, 100, 128
    _, maps = vis().shade(v[None].to(cuda), f.to(cuda), c.to(cuda), [[150., 150., 64., 50.]], IS, H, W, casters=casters,
                          return_maps=True)
    g = maps['raster0'][0, 1, :H, :W].cpu().numpy().reshape(-1)
    cov = g >= 0
    assert cov.sum() > 1000
    vrec = maps['vert_rec'][0].cpu().numpy().astype(np.float64)
    tri = f.numpy()[g[cov].astype(np.int64)]
    xp, yp = vr.pixel_centres(IS, H, W)
    w = vr.barycentric(vrec[tri, 3], vrec[tri, 7], xp.reshape(-1)[cov], yp.reshape(-1)[cov])
    assert w.min() >= -1e-5 and w.max() <= 1 + 1e-5, (w.min(), w.max())
    # the shadow raster follows the same convention: every stored light-space face covers its texel centre
    S = maps['S']
    sm = maps['shadow'][0, 1].cpu().numpy().reshape(-1)
    sc = sm >= 0
    xs, ys = vr.pixel_centres(S, S, S)
    xf = maps['shadow_xf'][0].cpu().numpy().astype(np.float64)
    u, vv, _ = (np.asarray(a) for a in vis().light_frame())
    pos = vrec[:, :3]
    lu, lv = (pos @ u - xf[0]) * xf[2], (pos @ vv - xf[1]) * xf[2]
    t = f.numpy()[sm[sc].astype(np.int64)]
    w = vr.barycentric(lu[t], lv[t], xs.reshape(-1)[sc], ys.reshape(-1)[sc])
    assert sc.sum() > 1000 and w.min() >= -1e-4 and w.max() <= 1 + 1e-4, (w.min(), w.max())


def lit(c, ndl, s=1.):
    v = vis()
    return np.rint(255 * v.ALBEDO_SCALE * np.asarray(c) * (v.K_AMBIENT + v.K_DIFFUSE * ndl * s))


def test_closed_form_shading_of_quads(cuda):
    v = vis()
    d = np.asarray(v.LIGHT_DIR)
    IS = H = W = 64
    K = [[80., 80., 32., 32.]]
    c = (0.9, 0.5, 0.25)
    qv, qf = quad((0, 0, 4), (1, 0, 0), (0, 1, 0), 1, 1)                        # faces the camera: n = (0, 0, -1)
    for smooth in (True, False):
        rgb = v.shade(qv[None].to(cuda), qf.to(cuda), torch.tensor(c).expand(4, 3).to(cuda), K, IS, H, W, smooth=smooth)
        ndl = max(0., float(np.dot((0, 0, -1), -d)))
        assert ndl > 0.7
        px = rgb[0, 16:48, 16:48].reshape(-1, 3).cpu().numpy()
        assert (px == lit(c, ndl)).all(), (px[:3], lit(c, ndl))
    n = np.array([0., 1., -0.3]) / np.linalg.norm([0., 1., -0.3])               # seen from below: turned away from the light
    assert np.dot(n, -d) < 0 and np.dot(n, (0, 0.5, 5)) < 0
    t2 = np.cross(n, (1, 0, 0))
    qv, qf = quad((0, 0.5, 5), (1, 0, 0), t2, 1.5, 1.5)
    rgb = v.shade(qv[None].to(cuda), qf.to(cuda), torch.tensor(c).expand(4, 3).to(cuda), K, IS, H, W)
    cov = v.shade(qv[None].to(cuda), qf.to(cuda), torch.tensor(c).expand(4, 3).to(cuda), K, IS, H, W, return_maps=True)[1]
    m = cov['raster0'][0, 1].cpu().numpy() >= 0
    assert m.sum() > 200
    assert (rgb[0].cpu().numpy()[m] == lit(c, 0.)).all()


def test_square_casts_its_closed_form_shadow_on_the_floor(cuda):
    v = vis()
    d = np.asarray(v.LIGHT_DIR)
    IS = H = W = 256
    fx, px = 400., 128.
    yf, ys = 1.0, 0.3
    fv, ff = quad((0, yf, 11), (1, 0, 0), (0, 0, 1), 4, 9)                        # floor y = 1, z in [2, 20]
    sv, sf = quad((0, ys, 5), (1, 0, 0), (0, 0, 1), 0.5, 0.5)                     # square x in [-.5, .5], z in [4.5, 5.5]
    verts, faces, cols = scene([(fv, ff, (1., 1., 1.)), (sv, sf, (0.5, 0.5, 0.5))])
    casters = torch.tensor([False] * 4 + [True] * 4)
    rgb, maps = v.shade(verts[None].to(cuda), faces.to(cuda), cols.to(cuda), [[fx, fx, px, px]], IS, H, W, casters=casters,
                        return_maps=True)
    img = rgb[0].cpu().numpy()
    g = maps['raster0'][0, 1].cpu().numpy()
    # the floor point seen at each pixel and whether the light reaches it: the square moved along d down to the floor
    r, c = np.mgrid[:H, :W] + 0.5
    t = yf / ((r - px) / fx)
    X, Z = t * (c - px) / fx, t
    shift = (yf - ys) / d[1] * d[2]
    inside = (np.abs(X) < 0.5) & (Z > 4.5 + shift) & (Z < 5.5 + shift) & (r > px)
    floor = (g >= 0) & (g < 2)
    from scipy.ndimage import binary_erosion
    deep_in = binary_erosion(inside & floor, np.ones((5, 5)))
    deep_out = binary_erosion(~inside & floor, np.ones((5, 5)))
    assert deep_in.sum() > 300 and deep_out.sum() > 5000
    ndl = float(np.dot((0, -1, 0), -d))
    assert (img[deep_in] == lit((1, 1, 1), ndl, 0.)).all()
    assert (img[deep_out] == lit((1, 1, 1), ndl, 1.)).all()


def test_convex_mesh_does_not_shadow_itself(cuda):
    v = vis()
    d = np.asarray(v.LIGHT_DIR)
    sv, sf = v.uv_sphere(1.0, 24, 32)
    verts = torch.from_numpy(sv * (1., 0.8, 1.2) + (0.2, -0.1, 5.)).float()
    IS = H = W = 128
    for smooth in (True, False):
        rgb, maps = v.shade(verts[None].to(cuda), torch.from_numpy(sf).to(cuda), torch.ones(len(verts), 3).to(cuda),
                            [[150., 150., 64., 64.]], IS, H, W, smooth=smooth, return_maps=True)
        s, ok = vr.shadow_fraction(maps, H, W)
        g = maps['raster0'][0, 1].cpu().numpy()
        gi = np.where(ok, g, 0).astype(np.int64)
        fn = maps['face_rec'][0, :, :3].cpu().numpy()[gi]
        cam = (fn * verts.numpy()[sf].mean(1)[gi]).sum(-1) > 0                  # turned toward the camera, as the kernel does
        fn = np.where(cam[..., None], -fn, fn)
        toward = ok & (fn @ -d > 0.1)
        assert toward.sum() > 1000 and (s[toward] == 1).all()
        want, margin = vr.shade(maps, H, W)
        assert np.abs(rgb[0].cpu().numpy().astype(int) - want[0]).max() <= 1


def test_translucent_surface_over_bones(cuda):
    v = vis()
    d = np.asarray(v.LIGHT_DIR)
    IS = H = W = 64
    K = [[80., 80., 32., 32.]]
    a = v.SURFACE_ALPHA
    cb, cs = (0.2, 0.9, 0.4), (0.8, 0.3, 0.6)
    ndl = float(np.dot((0, 0, -1), -d))
    for z_bone, z_surf in ((6., 5.), (5., 6.)):
        bv, bf = quad((0, 0, z_bone), (1, 0, 0), (0, 1, 0), 0.3 * z_bone / 5, 0.3 * z_bone / 5)
        qv, qf = quad((0, 0, z_surf), (1, 0, 0), (0, 1, 0), 0.3 * z_surf / 5, 0.3 * z_surf / 5)
        verts, faces, cols = scene([(bv, bf, cb), (qv, qf, cs)])
        rgb = v.shade(verts[None].to(cuda), faces.to(cuda), cols.to(cuda), K, IS, H, W, n_opaque=2)
        px = rgb[0, 28:36, 28:36].reshape(-1, 3).cpu().numpy().astype(np.float64)
        bone = 255 * v.ALBEDO_SCALE * np.asarray(cb) * (v.K_AMBIENT + v.K_DIFFUSE * ndl)
        surf = 255 * v.ALBEDO_SCALE * np.asarray(cs) * (v.K_AMBIENT + v.K_DIFFUSE * ndl)
        if z_surf < z_bone:
            assert np.abs(px - (a * surf + (1 - a) * bone)).max() <= 1
        else:
            assert (px == np.rint(bone)).all()


def _iou(a, b):
    return (a & b).sum() / max((a | b).sum(), 1)


def test_render_vis_end_to_end_camera_convention(cuda, tmp_path):
    from PIL import Image, ImageSequence
    root = str(tmp_path)
    n = 5
    rc = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'render_syn.py'), '--outdir', 'vis5', '--nframes', str(n),
                         '--img_size', '512', '--root', root], cwd=root, timeout=600, capture_output=True, text=True)
    assert rc.returncode == 0, rc.stderr[-2000:]
    base = os.path.join(root, 'database', 'DAVIS')
    test = os.path.join(root, 'vis-out')
    os.makedirs(test)
    from lasr_amd.soft_renderer.functional import load_obj, save_obj
    size, focal = 512, 10.
    for i in range(n):
        v, f = load_obj(os.path.join(base, 'Meshes', 'Full-Resolution', 'vis5', '%05d.obj' % i))
        save_obj(os.path.join(test, 'pred%d.obj' % i), v.cpu(), f.cpu())         # camera space, as extract.py writes it
        cam = np.loadtxt(os.path.join(base, 'Camera', 'Full-Resolution', 'vis5', '%05d.txt' % i))
        from lasr_amd.nnutils.mesh_net import quaternion_to_rotation_matrix
        R = quaternion_to_rotation_matrix(torch.tensor(np.r_[cam[4:7], cam[3]]).float()).numpy()
        rtk = np.zeros((4, 4))
        rtk[:3, :3], rtk[:3, 3] = R, (0, 0, cam[7])
        rtk[3] = (focal * size / 2, focal * size / 2, size / 2, size / 2)          # NDC focal 10 -> pixels of the 512 frame
        np.savetxt(os.path.join(test, 'cam%d.txt' % i), rtk)
    sys.path.insert(0, ROOT)
    import render_vis
    args = render_vis.parse_args(['--testdir', test, '--seqname', 'vis5', '--overlay'])
    meshes = [render_vis.load_mesh(test, i) for i in range(n)]
    meshes = [(mv, vis().fix_inversion(mv, mf), mc) for mv, mf, mc in meshes]
    for m in meshes:
        m[2][:, :2], m[2][:, 2] = 0, 255
    cams = [np.loadtxt(os.path.join(test, 'cam%d.txt' % i)) for i in range(n)]
    scenes = render_vis.build_scenes(args, meshes, [], cams, n, size, size, size)
    black = [np.zeros((size, size, 3), np.uint8)] * n
    rgb = vis().render_sequence(scenes, size, size, size, overlay=True, frames=black, device=cuda).cpu().numpy()
    sils = [np.asarray(Image.open(os.path.join(base, 'Annotations', 'Full-Resolution', 'vis5', '%05d.png' % i))) for i in range(n)]
    for i in range(n):
        assert _iou(rgb[i, ..., 2] > 0, sils[i] > 0) >= 0.99, (i, _iou(rgb[i, ..., 2] > 0, sils[i] > 0))
    # the script itself, in a fresh process.  With black input frames the --overlay GIF is black where no mesh is and blue where
    # the mesh is: its frames must match the silhouettes, brought to the GIF's 480 x 480 by the same bilinear resize
    for name in sorted(glob.glob(os.path.join(base, 'JPEGImages', 'Full-Resolution', 'vis5', '*.jpg'))):
        Image.fromarray(np.zeros((size, size, 3), np.uint8)).save(name, quality=95)
    small = render_vis.resize(torch.from_numpy(np.stack(sils))[..., None].expand(-1, -1, -1, 3).contiguous(), (480, 480))
    small = small[..., 0].numpy().astype(np.float64)                       # 128 inside, 0 outside, blended at the edge
    for extra, frames in (([], n), (['--append_img', 'yes'], n + n // 5), (['--freeze'], 150)):
        out = os.path.join(root, 'out.gif')
        rc = subprocess.run([sys.executable, os.path.join(ROOT, 'render_vis.py'), '--testdir', test, '--seqname', 'vis5',
                             '--outpath', out, '--overlay'] + extra, cwd=root, timeout=900, capture_output=True, text=True)
        assert rc.returncode == 0, rc.stderr[-2000:]
        g = Image.open(out)
        assert g.n_frames == frames and g.size == (480, 480), (extra, g.n_frames, g.size)
        if extra:
            continue
        gif = np.stack([np.asarray(f.convert('RGB')) for f in ImageSequence.Iterator(g)]).astype(np.int64)
        assert (gif[..., :2] <= 1).all()                              # blue mesh over black: red and green stay 0
        for i in range(n):
            # a pixel counts when a little of it is covered: the render's blue at >= 3, the silhouette's 128 scaled by the darkest
            # blue of the render's interior (a bright interior counts somewhat smaller coverages: a sliver of the edge pixels)
            dark = np.percentile(gif[i, ..., 2][small[i] >= 127.5], 1)
            got, want = gif[i, ..., 2] >= 3, small[i] >= 3 * 128. / dark
            assert dark >= 20 and _iou(got, want) >= 0.99, (i, dark, _iou(got, want))


def test_extract_writes_the_ply_files_render_vis_reads(cuda, tmp_path, monkeypatch):
    # extract.export on a fresh two-hypothesis, five-bone model of a rendered sequence: pred<i>.ply holds pred<i>.obj's mesh with
    # the exported hypothesis's vertex colours, gauss<i>.ply one ellipsoid per bone around its posed control point
    sys.path.insert(0, ROOT)
    import extract
    import optimize
    from lasr_amd.ext_utils.ply import read_ply
    from lasr_amd.nnutils import train_utils
    from lasr_amd.soft_renderer.functional import load_obj
    root = str(tmp_path / 'data')
    rc = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'render_syn.py'), '--outdir', 'ply3', '--nframes', '3',
                         '--img_size', '64', '--root', root], cwd=ROOT, timeout=600, capture_output=True, text=True)
    assert rc.returncode == 0, rc.stderr[-2000:]
    opts = optimize.parse_flags(['--name', 't', '--checkpoint_dir', str(tmp_path), '--img_size', '64', '--subdivide', '2',
                                 '--n_bones', '5', '--n_hypo', '2', '--batch_size', '1', '--opt_tex', 'yes', '--nouse_gtpose',
                                 '--only_mean_sym', '--noperceptual', '--nouse_graph', '--dataname', 'ply3', '--data_root', root])
    torch.manual_seed(0)
    tr = train_utils.LASRTrainer(opts).init_training()
    tr.reinit_bones()
    m = tr.module
    with torch.no_grad():                                          # distinct bone shapes and orientations
        m.ctl_rs.add_(0.3 * torch.randn_like(m.ctl_rs))
        m.log_ctl.copy_(torch.randn_like(m.log_ctl))
    tr.epoch_nscore = torch.tensor([1., 0.], device=cuda)          # the second hypothesis scores best
    calls = []
    real = extract.vis.gaussian_spheres

    def spy(ctl_ts, ctl_rs, log_ctl, Rmat, Tmat):
        calls.append([t.detach().cpu().double() for t in (ctl_ts, ctl_rs, log_ctl, Rmat, Tmat)])
        return real(ctl_ts, ctl_rs, log_ctl, Rmat, Tmat)
    monkeypatch.setattr(extract.vis, 'gaussian_spheres', spy)
    out_dir = os.path.join(str(tmp_path), 'out')
    done = extract.export(tr, out_dir)
    assert sorted(done) == [0, 1, 2] and len(calls) == 3
    H, J = 2, 4
    tex = m.get_mean_shape(1)[1].detach().view(2, H, -1, 3)[0, 1].cpu().double().numpy()
    ctl = [p.detach().view(H, J, -1)[1].cpu().double() for p in (m.ctl_ts, m.ctl_rs, m.log_ctl)]
    sv, sf = vis().uv_sphere()
    Vs = len(sv)
    for fid in done:
        ply = read_ply(os.path.join(out_dir, 'pred%d.ply' % fid))
        v, f = load_obj(os.path.join(out_dir, 'pred%d.obj' % fid))
        np.testing.assert_allclose(ply['verts'], v.cpu().numpy(), atol=1e-6)
        assert (ply['faces'] == f.cpu().numpy()).all()
        assert np.abs(ply['colors'].astype(np.float64) - np.floor(255 * tex)).max() <= 1
        rtk = np.loadtxt(os.path.join(out_dir, 'cam%d.txt' % fid))
        # the spy call of this frame: its body transform is the one cam<i>.txt records
        c = [c for c in calls if np.abs(c[3][0].numpy() - rtk[:3, :3]).max() < 1e-5 and np.abs(c[4][0].numpy() - rtk[:3, 3]).max() < 1e-4]
        assert len(c) == 1
        ctl_ts, ctl_rs, log_ctl, Rm, Tm = c[0]
        for a, b in zip((ctl_ts, ctl_rs, log_ctl), ctl):
            assert torch.equal(a, b)                                   # the exported hypothesis's bones
        g = read_ply(os.path.join(out_dir, 'gauss%d.ply' % fid))
        assert g['verts'].shape == (J * Vs, 3) and g['faces'].shape == (J * len(sf), 3)
        centre = ((ctl_ts[:, None] @ Rm[1:]).squeeze(1) + Tm[1:]) @ Rm[0] + Tm[0]     # bone, then body (identity skin)
        np.testing.assert_allclose(g['verts'].reshape(J, Vs, 3).mean(1), centre.numpy(), atol=5e-5)
        assert (g['colors'].reshape(J, Vs, 3) == vis().label_colormap(J)[:, None]).all()
