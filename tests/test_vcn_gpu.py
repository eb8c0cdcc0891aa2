"""The VCN matching kernels (csrc/vcn.hip) against their float64 restatements (tests/vcn_restated.py), known answers, the GPU
model against the reference's own outputs (tests/golden/vcn/), determinism, and preprocess/auto_gen.py end to end."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vcn_restated as R                                     # noqa: E402
from lasr_amd.ext_nnutils import vcn                         # noqa: E402
from lasr_amd.ext_utils import util_flow                     # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GOLD = os.path.join(ROOT, 'tests', 'golden', 'vcn')


def _features(b, C, h, w, seed, nonneg=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(b, C, h, w, generator=g)
    return (x.abs() if nonneg else x).to(DEV)


def _proj(F_, C, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(F_, C, generator=g) / C ** 0.5).to(DEV), (0.5 + torch.rand(F_, generator=g)).to(DEV), \
        (0.1 * torch.randn(F_, generator=g)).to(DEV)


def _flow(b, h, w, seed, scale):
    g = torch.Generator().manual_seed(seed)
    f = scale * torch.randn(b, 2, h, w, generator=g)
    f[:, :, ::3] = f[:, :, ::3].round()                       # integer flows: samples exactly on the lattice
    f[:, 0, :, -2] = 1.                                       # exactly onto the last column (|vgrid| = 1: dropped)
    f[:, 1, -2, :] = 1.                                       # exactly onto the last row
    f[:, 0, 1, :] = -5. - 0.5 * torch.arange(w, dtype=f.dtype)  # pushed out across the left border
    return f.to(DEV)


# levels of the 320x384 fixture pair, DAVIS 1088x1920 (levels 0 and 4) and a non-square odd size
CASES = [
    # b, C, F, h, w, md, fac, flow
    (1, 128, 16, 5, 6, 4, 1, False), (1, 128, 16, 5, 6, 4, 2, False), (1, 128, 16, 10, 12, 4, 1, True),
    (1, 128, 16, 20, 24, 4, 1, True), (1, 64, 16, 40, 48, 4, 1, True), (1, 64, 12, 80, 96, 4, 1, True),
    (1, 128, 16, 17, 30, 4, 1, False), (1, 128, 16, 17, 30, 4, 2, False), (1, 64, 12, 272, 480, 4, 1, True),
    (2, 64, 12, 37, 53, 4, 1, True), (2, 128, 16, 37, 53, 3, 2, False), (1, 64, 16, 37, 53, 7, 1, True),
    (1, 100, 12, 9, 70, 1, 1, True),
]


@pytest.mark.parametrize('b,C,F_,h,w,md,fac,with_flow', CASES)
def test_corr_proj_matches_the_float64_restatement(b, C, F_, h, w, md, fac, with_flow):
    mdv = int(md // fac)
    c1, c2 = _features(b, C, h, w, 1), _features(b, C, h, w, 2)
    W, sc, sh = _proj(F_, C, 3)
    fl = _flow(b, h, w, 4, 2.) if with_flow else None
    out = vcn.corr_proj(c1, c2, fl, W, sc, sh, md, mdv)
    ref = R.corr_proj64(c1, c2, fl, W, sc, sh, md, mdv)
    assert out.shape == (b, F_, 2 * md + 1, 2 * mdv + 1, h, w)
    err = float((out.double() - ref).abs().max())
    assert err <= 1e-5 * float(ref.abs().max()), (err, float(ref.abs().max()))


@pytest.mark.parametrize('dx,dy,md,mdv', [(2, -1, 4, 4), (-4, 3, 4, 4), (0, 0, 4, 2), (3, 2, 4, 2)])
def test_corr_proj_known_answer_on_a_shifted_copy(dx, dy, md, mdv):
    b, C, h, w = 1, 64, 23, 41
    c1 = _features(b, C, h, w, 7, nonneg=True)
    c2 = torch.zeros_like(c1)                                  # c2[q] = c1[q - d]: the match of p sits at p + d
    ys, xs = slice(max(0, dy), min(h, h + dy)), slice(max(0, dx), min(w, w + dx))
    c2[:, :, ys, xs] = c1[:, :, max(0, -dy):min(h, h - dy), max(0, -dx):min(w, w - dx)]
    shift = 0.375
    out = vcn.corr_proj(c1, c2, None, torch.ones(12, C, device=DEV), torch.ones(12, device=DEV),
                        torch.full((12,), shift, device=DEV), md, mdv)
    plane = out[0, 0, dx + md, dy + mdv].cpu().numpy()
    yy, xx = np.mgrid[:h, :w]
    inside = (yy + dy >= 0) & (yy + dy < h) & (xx + dx >= 0) & (xx + dx < w)
    assert np.abs(plane[inside] - (1. + shift)).max() <= 1e-6  # the cosine of a vector with itself
    assert np.all(plane[~inside] == shift)                     # outside the image: exactly the BN shift
    o = out[0, 3].cpu().numpy()                                # every displacement: out of range -> exactly shift
    for u in range(2 * md + 1):
        for v in range(2 * mdv + 1):
            far = ~((yy + v - mdv >= 0) & (yy + v - mdv < h) & (xx + u - md >= 0) & (xx + u - md < w))
            assert np.all(o[u, v][far] == shift)


def _cost(b, F_, U, V, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    return (3 * torch.randn(b, F_, U, V, h, w, generator=g)).to(DEV)


def test_flow_reg_planted_peaks_edges_and_ties():
    b, F_, md, mdv, h, w = 1, 4, 4, 4, 6, 70
    U, V = 2 * md + 1, 2 * mdv + 1
    cost = torch.zeros(b, F_, U, V, h, w, device=DEV)
    rng = np.random.default_rng(5)
    pu, pv = rng.integers(0, U, (F_, h, w)), rng.integers(0, V, (F_, h, w))
    pu[0], pv[0] = 0, V - 1                                    # a corner of the grid: window clipped to 4 x 4
    f_i, y_i, x_i = np.meshgrid(range(F_), range(h), range(w), indexing='ij')
    cost[0, f_i, pu, pv, y_i, x_i] = 60.                       # single peak: softmax mass e^-60 elsewhere
    up = torch.randn(b, 2, h, w, device=DEV)
    flow, ent = vcn.flow_reg(cost, up, md, mdv)
    rf, re = R.flow_reg64(cost, up, md, mdv)
    fl = flow.view(b, F_, 2, h, w).cpu().double()
    assert torch.allclose(fl[0, :, 0] - up[0, 0].cpu().double(), torch.from_numpy(pu - md).double(), atol=1e-6)
    assert torch.allclose(fl[0, :, 1] - up[0, 1].cpu().double(), torch.from_numpy(pv - mdv).double(), atol=1e-6)
    assert float(ent.view(b, F_, 2, h, w)[:, :, 0].abs().max()) < 1e-6
    assert float((flow.double() - rf).abs().max()) < 1e-5 and float((ent.double() - re).abs().max()) < 1e-5
    # a flat cost clipped at an edge: local entropy log(16 or 28 or 49) / log 49, the normalisation of the unclipped window
    flat = torch.zeros(1, 1, U, V, 1, 1, device=DEV)
    _, e = vcn.flow_reg(flat, None, md, mdv)                   # argmax of all-equal costs = index 0: window 4 x 4
    assert abs(float(e[0, 0]) - np.log(16) / np.log(49)) < 1e-6 and abs(float(e[0, 1]) - 1.) < 1e-6
    # exact ties: first index wins
    tie = torch.zeros(1, 1, U, V, 1, 2, device=DEV)
    tie[0, 0, 8, 8, 0, 0] = tie[0, 0, 1, 2, 0, 0] = 5.          # first in flat order: (1, 2)
    tie[0, 0, 6, 0, 0, 1] = tie[0, 0, 6, 5, 0, 1] = 5.          # (6, 0) then (6, 5)
    f2, _ = vcn.flow_reg(tie, None, md, mdv)
    rf2, _ = R.flow_reg64(tie, None, md, mdv)
    assert float((f2.double() - rf2).abs().max()) < 1e-6
    assert float(f2[0, 0, 0, 0]) < -1.5 and float(f2[0, 1, 0, 1]) < -2      # pulled towards (1, 2) and (6, 0)


@pytest.mark.parametrize('b,F_,h,w,md,fac,up', [(1, 16, 5, 6, 4, 2, False), (2, 16, 20, 24, 4, 1, True),
                                                 (1, 12, 68, 120, 4, 1, True), (1, 16, 17, 30, 7, 1, True)])
def test_flow_reg_matches_the_float64_restatement(b, F_, h, w, md, fac, up):
    mdv = int(md // fac)
    cost = _cost(b, F_, 2 * md + 1, 2 * mdv + 1, h, w, 11)
    upf = torch.randn(b, 2, h, w, device=DEV) if up else None
    flow, ent = vcn.flow_reg(cost, upf, md, mdv)
    rf, re = R.flow_reg64(cost, upf, md, mdv)
    x = cost.double().reshape(b * F_, -1, h, w)
    top2 = x.topk(2, 1).values
    near = ((top2[:, 0] - top2[:, 1]) <= 1e-6 * top2[:, 0].abs()).view(b, F_, h, w)
    near = near.repeat_interleave(2, 1)
    df, de = (flow.double() - rf).abs(), (ent.double() - re).abs()
    print('near-tie pixels (either window allowed): %d of %d' % (int(near.sum()) // 2, b * F_ * h * w))
    assert float(df[~near].max()) < 1e-5 and float(de[~near].max()) < 1e-5


def _gpu_model():
    return R.fill_state_dict(vcn.VCN()).eval().to(DEV)


def test_gpu_model_matches_the_reference_fixture():
    m = _gpu_model()
    with torch.no_grad():
        flow, occ, levels = m(R.pair_input(*R.input_pair()).to(DEV), return_levels=True)
    fin = np.load(os.path.join(GOLD, 'final.npz'))
    lv = np.load(os.path.join(GOLD, 'levels.npz'))
    d = np.abs(flow.cpu().numpy() - fin['flow'])
    frac = float((d.max(1) <= 1e-2).mean())
    docc = float(np.abs(occ.cpu().numpy() - fin['occ']).max())
    lev = [float(np.abs(f.cpu().numpy() - lv['flow%d' % i]).max()) for i, (f, _, _) in enumerate(levels)]
    print('final flow: %.4f%% of pixels within 1e-2 px (worst %.2e); occ worst %.2e; per level %s'
          % (100 * frac, d.max(), docc, ', '.join('%.1e' % e for e in lev)))
    assert frac >= 0.99 and docc <= 1e-3


def test_two_runs_are_bit_identical():
    m = _gpu_model()
    im = R.pair_input(*R.input_pair()).to(DEV)
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True                 # MIOpen's convolutions; the matching kernels use no atomics
    try:
        with torch.no_grad():
            m(im)
            a = m(im)
            b = m(im)
    finally:
        torch.backends.cudnn.deterministic = det
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    c1, c2 = _features(1, 64, 40, 48, 1), _features(1, 64, 40, 48, 2)
    W, sc, sh = _proj(16, 64, 3)
    fl = _flow(1, 40, 48, 4, 2.)
    assert torch.equal(vcn.corr_proj(c1, c2, fl, W, sc, sh, 4, 4), vcn.corr_proj(c1, c2, fl, W, sc, sh, 4, 4))


def test_auto_gen_dry_run_on_a_rendered_sequence(tmp_path):
    root, seq = str(tmp_path), 'synvcn'
    rc = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'render_syn.py'), '--outdir', seq, '--nframes', '4',
                         '--img_size', '128', '--root', root], cwd=root, timeout=600, capture_output=True, text=True)
    assert rc.returncode == 0, rc.stderr[-2000:]
    dp = os.path.join(root, 'database', 'DAVIS', 'JPEGImages', 'Full-Resolution', seq) + '/'
    out = os.path.join(root, 'out')
    rc = subprocess.run([sys.executable, os.path.join(ROOT, 'preprocess', 'auto_gen.py'), '--datapath', dp, '--outdir', out,
                         '--flow_threshold', '0.01'], cwd=root, timeout=600, capture_output=True, text=True)
    assert rc.returncode == 0, rc.stdout[-2000:] + rc.stderr[-2000:]
    assert 'dry run' in rc.stdout
    fw = sorted(f for f in os.listdir(os.path.join(out, 'FlowFW')) if f.startswith('flo-'))
    n = len(os.listdir(os.path.join(out, 'JPEGImages')))
    assert n == len(fw) + 1 and len(fw) >= 1
    assert sorted(os.listdir(os.path.join(out, 'FlowBW'))) == sorted(
        ['flo-%05d.pfm' % (i + 1) for i in range(len(fw))] + ['occ-%05d.pfm' % (i + 1) for i in range(len(fw))])
    # the skipping, recomputed from the forward flows written for the kept pairs: each exceeds the threshold
    spec = importlib.util.spec_from_file_location('auto_gen', os.path.join(ROOT, 'preprocess', 'auto_gen.py'))
    ag = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ag)
    from PIL import Image
    for i, f in enumerate(fw):
        flow = util_flow.readPFM(os.path.join(out, 'FlowFW', f))[0][::-1]
        mask = np.asarray(Image.open(os.path.join(out, 'Annotations', '%05d.png' % i))) > 0
        assert flow.shape[2] == 3 and np.all(flow[:, :, 2] == 1)
        assert ag.median_flow(flow, mask) > 0.01
    # the frames the script skipped: their forward flows (recomputed in-process) stay at or under the threshold
    args = ag.parse_args(['--datapath', dp, '--outdir', os.path.join(root, 'again'), '--flow_threshold', '0.01'])
    model = ag.build_model(args)
    kept = ag.run(args, lambda a, b: ag.flow_inference(model, a, b))
    assert len(kept) == len(fw)
    again = util_flow.readPFM(os.path.join(root, 'again', 'FlowFW', fw[0]))[0]
    first = util_flow.readPFM(os.path.join(out, 'FlowFW', fw[0]))[0]
    assert np.abs(again - first).max() <= 1e-4 * max(np.abs(first).max(), 1.)     # MIOpen may pick other algorithms per process
    # the loader consumes the tree (auto_gen.sh's copy into the DAVIS layout)
    import shutil
    from types import SimpleNamespace
    from lasr_amd.dataloader import vid
    for d in ('JPEGImages', 'Annotations', 'FlowFW', 'FlowBW'):
        shutil.copytree(os.path.join(out, d), os.path.join(root, 'database', 'DAVIS', d, 'Full-Resolution', 'r' + seq))
    os.makedirs(os.path.join(root, 'configs'), exist_ok=True)
    with open(os.path.join(root, 'configs', 'r%s.config' % seq), 'w') as fh:
        fh.write('[data]\ndatapath = database/DAVIS/JPEGImages/Full-Resolution/r%s/\ndframe = 1\ninit_frame = 0\n'
                 'end_frame = -1\ncan_frame = 0\n' % seq)
    opts = SimpleNamespace(dataname='r' + seq, sil_path='none', batch_size=1, ngpu=1, local_rank=0, img_size=64,
                           n_data_workers=0)
    loader, length = vid.data_loader(opts, shuffle=False, root=root)
    e = loader.dataset[0]
    assert length == n and e['flow'].shape == (3, 64, 64) and np.isfinite(e['flow']).all()
