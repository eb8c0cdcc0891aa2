"""BADJA keypoint transfer on the GPU: lasr_kp_transfer (csrc/keypoints.hip) bit for bit against the restatement
(badja_restated.py) and torch on the device, render_flow_soft_3 in closed form, and scripts/eval_badja.py end to end on a
rendered synthetic sequence."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import badja_restated as br                       # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32


@pytest.fixture(scope='module')
def cuda():
    if not torch.cuda.is_available():
        pytest.skip('needs a HIP device')
    return torch.device('cuda', 0)


def kp_transfer(colors, kp, H, W):
    from lasr_amd.nnutils.keypoints import kp_transfer as k
    return k(colors, kp, H, W)


def torch_dense(colors, kp, H, W):
    """The reference's torch operations on the device (geom_utils.py:82-93, eval_badja.py:227-242) on given raster colours."""
    px = colors.permute(0, 2, 3, 1).clone()
    S = px.shape[1]
    bg = px[..., 2] < 1e-9
    px[bg] = 10
    g = torch.tensor(np.stack(np.meshgrid(range(S), range(S))), dtype=torch.float32, device=colors.device)
    g[0] = g[0] * 2 / (S - 1) - 1
    g[1] = g[1] * 2 / (S - 1) - 1
    flow = px[..., :2] - g.permute(1, 2, 0)[None]
    flow[bg] = 0.
    idxs, preds = [], []
    x0, y0 = np.meshgrid(range(W), range(H))
    x0 = torch.tensor(x0, dtype=torch.float32, device=colors.device)
    y0 = torch.tensor(y0, dtype=torch.float32, device=colors.device)
    for b in range(colors.shape[0]):
        f = torch.cat([flow[b:b + 1], torch.zeros_like(flow[b:b + 1])[..., :1]], -1)[:, :H, :W].contiguous()
        k = kp[b]
        idx = ((f[..., :2].norm(2, -1) < 1e-6).float().view(1, -1) * 1e6 + torch.pow(k[:, 0:1] - y0.view(1, -1), 2)
               + torch.pow(k[:, 1:2] - x0.view(1, -1), 2)).argmin(-1)
        s = f.view(-1, 3)[idx][:, :2]
        p = k.clone()
        p[:, 0] = p[:, 0] + s[:, 1] * H / 2
        p[:, 1] = p[:, 1] + s[:, 0] * W / 2
        idxs.append(idx)
        preds.append(p)
    return torch.stack(idxs).cpu().numpy(), torch.stack(preds).cpu().numpy()


def check_against_restatement(colors, kp, H, W, dense=False):
    idx, pred = kp_transfer(colors, kp, H, W)
    idx, pred = idx.cpu().numpy(), pred.cpu().numpy()
    c, k = colors.cpu().numpy(), kp.cpu().numpy()
    for b in range(c.shape[0]):
        ei, ep = br.transfer(br.flow_from_colors(c[b]), k[b], H, W)
        np.testing.assert_array_equal(idx[b], ei, err_msg='pair %d' % b)
        np.testing.assert_array_equal(pred[b].view(np.uint32), ep.view(np.uint32), err_msg='pair %d' % b)
    if dense:
        di, dp = torch_dense(colors, kp, H, W)
        np.testing.assert_array_equal(idx, di)
        np.testing.assert_array_equal(pred.view(np.uint32), dp.view(np.uint32))
    return idx, pred


def random_case(rng, B, J, S, H, W, dev):
    """Random raster colours with pair b's background fraction b / (B - 1) (0 to 100 %), some covered pixels whose flow is exactly
    zero (invalid on the mesh), and integer keypoints on, inside and outside the border of the crop."""
    c = rng.uniform(-1.2, 1.2, (B, 4, S, S)).astype(F32)
    c[:, 2] = rng.uniform(1., 10., (B, S, S))
    for b in range(B):
        frac = b / max(B - 1, 1)
        m = rng.random((S, S)) < frac
        c[b, 2][m] = rng.choice([0., 1e-10, -1.], m.sum())
    g = (np.arange(S, dtype=F32) * F32(2)) * (F32(1) / F32(S - 1)) - F32(1)
    z = rng.random((B, S, S)) < 0.05                                  # colour == grid: zero flow on a covered pixel
    c[:, 0] = np.where(z, g[None, None, :], c[:, 0])
    c[:, 1] = np.where(z, g[None, :, None], c[:, 1])
    kp = np.stack([rng.integers(-5, H + 5, (B, J)), rng.integers(-5, W + 5, (B, J))], -1).astype(F32)
    border = [(0, 0), (H - 1, W - 1), (0, W - 1), (H - 1, 0), (-3, W + 7)]
    for k in range(min(J, len(border))):
        kp[:, k] = border[k]
    return torch.from_numpy(c).to(dev), torch.from_numpy(kp).to(dev)


@pytest.mark.parametrize('S,H,W,B', [(256, 256, 256, 4), (640, 360, 640, 9), (1920, 1080, 1920, 17), (255, 200, 131, 3),
                                     (64, 64, 40, 2)])
def test_kernel_matches_restatement_bit_for_bit(cuda, S, H, W, B):
    rng = np.random.default_rng(S + H + W)
    colors, kp = random_case(rng, B, 20, S, H, W, cuda)
    check_against_restatement(colors, kp, H, W, dense=S <= 640)


def test_up_to_64_keypoints(cuda):
    rng = np.random.default_rng(7)
    for J in (1, 25, 64):
        colors, kp = random_case(rng, 3, J, 128, 96, 128, cuda)
        check_against_restatement(colors, kp, 96, 128, dense=True)


def test_ties_take_the_lowest_flat_index(cuda):
    S = H = W = 64
    c = np.zeros((1, 4, S, S), F32)                                  # all background but four pixels around (20, 30)
    kp = np.array([[[20., 30.], [40., 10.]]], F32)
    for r, col in ((17, 30), (20, 27), (20, 33), (23, 30), (40, 14), (36, 10)):   # distance 3 and 4
        c[0, :3, r, col] = (0.25, -0.5, 2.)
    idx, pred = check_against_restatement(torch.from_numpy(c).to(cuda), torch.from_numpy(kp).to(cuda), H, W, dense=True)
    assert idx[0, 0] == 17 * W + 30                                   # four at distance 3: the first in row-major order
    assert idx[0, 1] == 36 * W + 10                                   # distance 4 twice: the first


def test_flow_norms_at_the_threshold(cuda):
    """Covered pixels near the raster's centre (small grid values, fine flow steps) get flows whose norm lies within a few ulp of
    1e-6 on either side; all other pixels but one far corner are background.  Each keypoint sits on one of them, so idx shows
    whether it counted as valid."""
    S = H = W = 512
    rng = np.random.default_rng(3)
    g = (np.arange(S, dtype=F32) * F32(2)) * (F32(1) / F32(S - 1)) - F32(1)
    c = np.zeros((1, 4, S, S), F32)
    c[0, :3, 0, 0] = (0.5, 0.5, 1.)                                   # the fallback, far from every keypoint
    pts, n_inside = [], 0
    for r in range(250, 262):
        for col in range(250, 262):
            best = None
            for _ in range(400):
                th = rng.uniform(0, 2 * np.pi)
                t = 1e-6 * (1 + rng.uniform(-3e-6, 3e-6))
                c0 = F32(float(g[col]) + t * np.cos(th))
                c1 = F32(float(g[r]) + t * np.sin(th))
                fx, fy = c0 - g[col], c1 - g[r]
                nrm = np.sqrt(fx * fx + fy * fy)
                d = abs(float(nrm) - 1e-6)
                if best is None or d < best[0]:
                    best = (d, c0, c1, nrm)
            c[0, :3, r, col] = (best[1], best[2], 1.)
            pts.append((r, col))
            n_inside += best[3] < F32(1e-6)
    assert 0 < n_inside < len(pts)
    kp = np.array([pts[k::2][:32] for k in range(2)], F32).reshape(-1, 2)[:64][None]
    dev_colors = torch.from_numpy(c).to(cuda)
    idx, _ = check_against_restatement(dev_colors, torch.from_numpy(kp).to(cuda), H, W, dense=True)
    own = idx[0] == kp[0, :, 0].astype(np.int64) * W + kp[0, :, 1].astype(np.int64)
    assert 0 < own.sum() < kp.shape[1]                                 # some keypoints keep their own pixel, some move on


def test_zero_flow(cuda):
    rng = np.random.default_rng(11)
    for H, W in ((1080, 1920), (480, 270)):
        kp = torch.from_numpy(np.stack([rng.integers(-4, H + 4, (5, 20)), rng.integers(-4, W + 4, (5, 20))], -1).astype(F32)).to(cuda)
        idx, pred = kp_transfer(None, kp, H, W)
        k = kp.cpu().numpy()
        np.testing.assert_array_equal(pred.cpu().numpy(), k)
        z = np.zeros((max(H, W), max(H, W), 2), F32)
        for b in range(5):
            np.testing.assert_array_equal(idx[b].cpu().numpy(), br.transfer(z, k[b], H, W)[0])


def test_host_checks(cuda):
    from lasr_amd import _lib
    h = _lib.lib()
    kp = torch.zeros(1, 20, 2, device=cuda)
    idx = torch.empty(1, 20, dtype=torch.int64, device=cuda)
    pred = torch.empty(1, 20, 2, device=cuda)
    c = torch.zeros(1, 4, 64, 64, device=cuda)
    st = torch.cuda.current_stream().cuda_stream
    ok = (c.data_ptr(), kp.data_ptr(), idx.data_ptr(), pred.data_ptr(), 1, 20, 64, 64, 64, st)
    assert h.lasr_kp_transfer(*ok) == 0
    torch.cuda.synchronize()
    for k, v in ((5, 0), (5, 65), (6, 1), (6, 16385), (7, 65), (8, 65), (7, 0), (1, None), (2, None), (3, None)):
        bad = list(ok)
        bad[k] = v
        assert h.lasr_kp_transfer(*bad) == -1, (k, v)


def renderer():
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    import eval_badja
    return eval_badja.make_renderer()


def test_render_flow_soft_3_constant_shift(cuda):
    from lasr_amd.nnutils.geom_utils import render_flow_soft_3
    S = 128
    r = renderer()
    r.rasterizer.image_size = S
    # a quad of two triangles at depth 5, and a target shifted by a constant NDC step
    v = torch.tensor([[[-0.5, -0.4, 5.], [0.6, -0.5, 5.], [0.5, 0.6, 5.], [-0.6, 0.5, 5.]]], device=cuda)   # one depth: affine
    f = torch.tensor([[[0, 1, 2], [0, 2, 3]]], dtype=torch.int32, device=cuda)
    shift = torch.tensor([0.125, -0.0625, 0.], device=cuda)
    flow, bg, fg = render_flow_soft_3(r, v, v + shift, f)
    cov = fg[0] == 1                          # fgmask is a view of the colours: the background fill writes 10 into it too
    assert cov.sum() > 0.2 * S * S and bool((fg[0][~cov] == 10).all())
    assert torch.equal(bg[0], ~cov)
    px = np.meshgrid(range(S), range(S))
    grid = np.stack([(p.astype(F32) * F32(2)) * (F32(1) / F32(S - 1)) - F32(1) for p in px], -1)
    # covered pixels: the target position is the interpolated source position + shift; the source position at pixel centre p
    # is the centre itself ((2p + 1 - S) / S, y flipped by the renderer), so flow = shift + centre - grid
    centre = np.stack([(2 * p + 1 - S) / S for p in px], -1)
    want = centre - grid + np.array([0.125, -0.0625])
    got = flow[0].cpu().numpy()
    m = cov.cpu().numpy()
    assert np.abs(got[m] - want[m]).max() < 1e-5


def _iou(a, b):
    return (a & b).sum() / max((a | b).sum(), 1)


def test_eval_badja_end_to_end(cuda, tmp_path):
    from PIL import Image
    from lasr_amd import vis, _lib
    from lasr_amd.ext_utils.badja_data import ANNOTATED_JOINTS
    from lasr_amd.ext_utils.ply import write_ply
    from lasr_amd.nnutils.geom_utils import render_flow_soft_3
    from lasr_amd.soft_renderer.functional import load_obj
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    import eval_badja
    root = str(tmp_path)
    n, size, focal, seq = 6, 512, 10., 'spot6'
    rc = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'render_syn.py'), '--outdir', seq, '--nframes', str(n),
                         '--img_size', str(size), '--root', root, '--obj', os.path.join(ROOT, 'tests', 'golden', 'spot',
                                                                                        'spot_triangulated.obj'),
                         '--model', 'spot'], cwd=root, timeout=600, capture_output=True, text=True)
    assert rc.returncode == 0, rc.stderr[-2000:]
    base = os.path.join(root, 'database', 'DAVIS')
    test = os.path.join(root, 'out')
    os.makedirs(test)
    verts = []
    for i in range(n):
        v, f = load_obj(os.path.join(base, 'Meshes', 'Full-Resolution', seq, '%05d.obj' % i))
        faces = f.cpu().numpy()
        verts.append(v.cpu().numpy().astype(np.float64))
        write_ply(os.path.join(test, 'pred%d.ply' % i), verts[-1], faces)        # camera space: R = I, T = 0
        rtk = np.zeros((4, 4))
        rtk[:3, :3] = np.eye(3)
        rtk[3] = (focal * size / 2, focal * size / 2, size / 2, size / 2)
        np.savetxt(os.path.join(test, 'cam%d.txt' % i), rtk)
    from lasr_amd.ext_utils.ply import read_ply                                   # what the script reads (rounded text)
    verts = np.stack([read_ply(os.path.join(test, 'pred%d.ply' % i))['verts'] for i in range(n)]).astype(np.float64)
    cams = np.stack([np.loadtxt(os.path.join(test, 'cam%d.txt' % i)) for i in range(n)])
    vproj = eval_badja.project(verts, cams, size, cuda)
    ft = torch.tensor(faces, dtype=torch.int32, device=cuda)[None]
    r = eval_badja.make_renderer()
    r.rasterizer.image_size = size
    sils = [np.asarray(Image.open(os.path.join(base, 'Annotations', 'Full-Resolution', seq, '%05d.png' % i))) for i in range(n)]
    # synthetic annotations: 20 vertices projected with the ground-truth camera, visible where the face map shows an incident face
    rng = np.random.default_rng(0)
    pick = rng.choice(verts.shape[1], 20, replace=False)
    F = faces.shape[0]
    h = _lib.lib()
    annos = []
    for i in range(n):
        with torch.no_grad():
            _, bgm, _ = render_flow_soft_3(r, vproj[i:i + 1], vproj[i:i + 1], ft)
        cover = ~bgm[0].cpu().numpy()
        assert _iou(cover, sils[i] > 0) >= 0.99, (i, _iou(cover, sils[i] > 0))
        p = vproj[i].clone()
        p[:, 1] = -p[:, 1]
        fv = p[:, :3][ft[0].long()][None].contiguous()
        aggrs = vis._raster(h, fv, size, 1., 100., torch.cuda.current_stream().cuda_stream)
        fmap = aggrs[0, 1].cpu().numpy()
        q = vproj[i, pick, :2].cpu().numpy().astype(np.float64)
        col = np.floor((q[:, 0] + 1) * size / 2).astype(np.int64)
        row = np.floor((q[:, 1] + 1) * size / 2).astype(np.int64)
        joints = np.zeros((37, 2), np.int64)
        visible = np.zeros(37, bool)
        for k, vi in enumerate(pick):
            fi = int(fmap[row[k], col[k]]) if 0 <= row[k] < size and 0 <= col[k] < size else -1
            visible[ANNOTATED_JOINTS[k]] = fi >= 0 and vi in faces[fi % F]
            joints[ANNOTATED_JOINTS[k]] = (row[k], col[k])
        assert visible.sum() >= 5, i
        annos.append({'image_path': 'DAVIS/JPEGImages/Full-Resolution/%s/%05d.jpg' % (seq, i),
                      'segmentation_path': 'DAVIS/Annotations/Full-Resolution/%s/%05d.png' % (seq, i),
                      'joints': joints.tolist(), 'visibility': visible.tolist()})
    os.makedirs(os.path.join(root, 'database', 'joint_annotations'))
    with open(os.path.join(root, 'database', 'joint_annotations', '%s.json' % seq), 'w') as fh:
        json.dump(annos, fh)

    def run(*extra, testdir=test):
        out = os.path.join(root, 'res.json')
        rc = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'eval_badja.py'), '--testdir', testdir, '--seqname', seq,
                             '--json', out] + list(extra), cwd=root, timeout=900, capture_output=True, text=True)
        assert rc.returncode == 0, rc.stderr[-2000:]
        return rc.stdout.strip().splitlines()[-1], json.load(open(out))

    line, res = run('--type', 'mesh')
    assert line == 'PCK 100.00', line
    line_d, res_d = run('--type', 'mesh', '--dense')
    assert line_d == line and res_d['pairs'] == res['pairs']
    # the restatement on flows rendered pair by pair through render_flow_soft_3
    kps = [np.asarray(a['joints'])[ANNOTATED_JOINTS] for a in annos]
    vis_ = [np.asarray(a['visibility'])[ANNOTATED_JOINTS] for a in annos]
    sil3 = [np.asarray(Image.open(os.path.join(base, 'Annotations', 'Full-Resolution', seq, '%05d.png' % i)).convert('RGB'))
            for i in range(n)]
    k = 0
    for i in range(n):
        for j in range(n):
            if i == j:
                continue
            with torch.no_grad():
                flow, bg, _ = render_flow_soft_3(r, vproj[i:i + 1], vproj[j:j + 1], ft)
                flow[bg] = 0.
            ei, ep = br.transfer(flow[0].cpu().numpy(), kps[i], size, size)
            pr = res['pairs'][k]
            assert (pr['ref'], pr['tar']) == (i, j)
            assert pr['idx'] == ei.tolist()
            np.testing.assert_array_equal(np.asarray(pr['pred'], np.float64), ep.astype(np.float64))
            assert pr['correct'] == br.score(ep, sil3[i], kps[j], vis_[i], vis_[j]).tolist()
            k += 1
    # the zero flow
    line, res = run('--type', 'zero')
    flags = [br.score(kps[i].astype(F32), sil3[i], kps[j], vis_[i], vis_[j]) for i in range(n) for j in range(n) if i != j]
    assert line == 'PCK %.02f' % br.pck(flags), line
    # one frame's camera turned by 90 degrees about y: its transfers go wrong
    bad = os.path.join(root, 'bad')
    os.makedirs(bad)
    for i in range(n):
        for name in ('pred%d.ply' % i, 'cam%d.txt' % i):
            with open(os.path.join(test, name)) as a, open(os.path.join(bad, name), 'w') as b:
                b.write(a.read())
    rtk = np.loadtxt(os.path.join(bad, 'cam2.txt'))
    rtk[:3, :3] = np.array([[0., 0., -1.], [0., 1., 0.], [1., 0., 0.]])
    rtk[:3, 3] = (0., 0., 10.) - np.array([0., 0., 10.]) @ rtk[:3, :3]           # turn about the mesh's centre at depth 10
    np.savetxt(os.path.join(bad, 'cam2.txt'), rtk)
    line, _ = run('--type', 'mesh', testdir=bad)
    assert line.startswith('PCK ') and float(line[4:]) < 100., line
