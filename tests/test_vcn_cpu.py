"""VCN model and preprocess/auto_gen.py without a GPU: state_dict compatibility with the reference, the model with the float64
restatements of the two matching kernels against the reference's own outputs (tests/golden/vcn/, tools/gen_vcn_golden.py),
and the script's frame selection and file layout on a stub flow."""
import importlib.util
import json
import os
import shutil
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vcn_restated as R                                     # noqa: E402
from lasr_amd.ext_nnutils import vcn                         # noqa: E402
from lasr_amd.ext_utils import util_flow                     # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden', 'vcn')


def _ref_names():
    return {k: tuple(s) for k, s in json.load(open(os.path.join(GOLD, 'state_dict.json')))}


def _auto_gen():
    spec = importlib.util.spec_from_file_location('auto_gen', os.path.join(ROOT, 'preprocess', 'auto_gen.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_state_dict_is_a_subset_of_the_reference():
    ref = _ref_names()
    sd = vcn.VCN().state_dict()
    bad = [(k, tuple(v.shape), ref.get(k)) for k, v in sd.items() if ref.get(k) != tuple(v.shape)]
    assert not bad, bad[:10]
    assert len(sd) > 1000


def test_reference_keyed_checkpoint_sets_every_parameter():
    ref = _ref_names()
    sd = {'module.' + k: torch.from_numpy(R.vcn_test_weights(k, s)) for k, s in ref.items()
          if not k.startswith(('flow_reg', 'warp', 'reg_modules', 'warp_modules'))}
    ck = {'state_dict': sd, 'mean_L': [[0.1, 0.2, 0.3]], 'mean_R': [[0.4, 0.5, 0.6]]}
    m = vcn.VCN()
    for p in m.parameters():
        p.data.fill_(float('nan'))
    missing, unexpected = vcn.load_checkpoint(m, ck, verbose=False)
    assert missing == [] and len(unexpected) > 0              # aliases and heads the inference path does not use
    assert all(torch.isfinite(p).all() for p in m.parameters())
    assert torch.equal(m.state_dict()['f6.proj.0.conv1.weight'], sd['module.f6.proj.0.conv1.weight'])
    assert torch.allclose(m.mean_L, torch.tensor([[0.1, 0.2, 0.3]])) and torch.allclose(m.mean_R, torch.tensor([[0.4, 0.5, 0.6]]))


def test_checkpoint_load_reports_key_counts(tmp_path, capsys):
    path = str(tmp_path / 'ck.pth')
    m0 = vcn.VCN()
    torch.save({'state_dict': {'module.' + k: v for k, v in m0.state_dict().items()}, 'mean_L': [[0.33] * 3],
                'mean_R': [[0.33] * 3]}, path)
    vcn.load_checkpoint(vcn.VCN(), path)
    assert 'VCN checkpoint: 0 missing keys, 0 unexpected keys' in capsys.readouterr().out


def test_size_independent_model_rejects_unpadded_input():
    with pytest.raises(ValueError):
        vcn.VCN()(torch.zeros(2, 3, 100, 128))


def test_cpu_model_with_restated_matching_matches_the_reference_fixture():
    m = R.fill_state_dict(vcn.VCN()).eval()
    undo = R.patch_vcn_matching(vcn)
    try:
        with torch.no_grad():
            flow, occ, levels = m(R.pair_input(*R.input_pair()), return_levels=True)
    finally:
        undo()
    fin = np.load(os.path.join(GOLD, 'final.npz'))
    lv = np.load(os.path.join(GOLD, 'levels.npz'))
    report = []

    def close(name, a, b, rel):
        err, mag = float(np.abs(a - b).max()), float(np.abs(b).max())
        report.append('%s %.2e of %.1f' % (name, err, mag))
        assert err <= rel * max(mag, 1.), (name, err, mag)
    # random weights give flows of up to ~200 px: fp32 rounding through five levels of convolutions leaves ~1.5e-5 relative
    for lvl, (f, fh, eh) in enumerate(levels):
        close('flow%d' % lvl, f.numpy(), lv['flow%d' % lvl], 5e-5)
        if lvl <= 2:
            close('flowh%d' % lvl, fh.numpy(), lv['flowh%d' % lvl], 5e-6)
            close('enth%d' % lvl, eh.numpy(), lv['enth%d' % lvl], 5e-6)
    close('flow', flow.numpy(), fin['flow'], 5e-5)
    close('occ', occ.numpy(), fin['occ'], 5e-6)
    print('worst cases: ' + ', '.join(report))


# ---- preprocess/auto_gen.py on a stub flow ---------------------------------------------------------------------------------
def _sequence(root, seq='toy', n=6, H=48, W=64):
    from PIL import Image
    img_dir = os.path.join(root, 'database', 'DAVIS', 'JPEGImages', 'Full-Resolution', seq)
    ann_dir = img_dir.replace('JPEGImages', 'Annotations')
    os.makedirs(img_dir)
    os.makedirs(ann_dir)
    yy, xx = np.mgrid[:H, :W]
    for i in range(n):
        img = np.stack([(xx * 3 + i * 20) % 256, (yy * 5) % 256, np.full_like(xx, 90)], -1).astype(np.uint8)
        Image.fromarray(img).save(os.path.join(img_dir, '%05d.jpg' % i), quality=95)
        mask = (np.abs(xx - 32) < 11) & (np.abs(yy - 24) < 9)        # 21 x 17 box: half extents 10 and 8
        Image.fromarray((255 * mask).astype(np.uint8)).save(os.path.join(ann_dir, '%05d.png' % i))
    return img_dir + '/'


def _stub(speeds):
    """flow_fn whose forward flow i -> j is a constant (speed_i, 0) px, read off the red channel's frame offset."""
    calls = []

    def fn(a, b):
        i, j = int(round(a[0, 0, 0] / 20.)), int(round(b[0, 0, 0] / 20.))
        calls.append((i, j))
        v = sum(speeds[min(i, j):max(i, j)]) * (1 if j > i else -1)
        flow = np.zeros(a.shape[:2] + (3,), np.float32)
        flow[:, :, 0] = v
        flow[:, :, 1] = 0.5 * v
        flow[:, :, 2] = 1
        occ = np.full(a.shape[:2], 0.25 * v, np.float32)
        occ[0] = -1                                                    # marks the top row
        return flow, occ
    return fn, calls


def test_frame_skipping_follows_the_median_normalised_flow(tmp_path):
    ag = _auto_gen()
    dp = _sequence(str(tmp_path))
    speeds = [1., 0.2, 0.2, 0.2, 1.5]                                  # px per frame step
    fn, calls = _stub(speeds)
    args = ag.parse_args(['--datapath', dp, '--flow_threshold', '0.05', '--outdir', str(tmp_path / 'out')])
    kept = ag.run(args, fn)
    # normalised |flow| = sqrt((v/10)^2 + (0.5 v/8)^2) = 0.1180 v: v = 1 kept; 0.2, 0.4 not (0.047), 0.6 kept (0.071); 1.5 kept
    assert kept == [(0, 1), (1, 4), (4, 5)]
    assert calls == [(0, 1), (1, 0), (1, 2), (1, 3), (1, 4), (4, 1), (4, 5), (5, 4)]


def test_output_names_pfm_rows_and_ones_channel(tmp_path):
    ag = _auto_gen()
    dp = _sequence(str(tmp_path), n=3)
    fn, _ = _stub([1., 1.])
    out = tmp_path / 'out'
    ag.run(ag.parse_args(['--datapath', dp, '--outdir', str(out)]), fn)
    names = {d: sorted(os.listdir(out / d)) for d in ('FlowFW', 'FlowBW', 'JPEGImages', 'Annotations')}
    assert names == {'FlowFW': ['flo-00000.pfm', 'flo-00001.pfm', 'occ-00000.pfm', 'occ-00001.pfm'],
                     'FlowBW': ['flo-00001.pfm', 'flo-00002.pfm', 'occ-00001.pfm', 'occ-00002.pfm'],
                     'JPEGImages': ['00000.jpg', '00001.jpg', '00002.jpg'],
                     'Annotations': ['00000.png', '00001.png', '00002.png']}
    fl, _ = util_flow.readPFM(str(out / 'FlowFW' / 'flo-00000.pfm'))
    occ, _ = util_flow.readPFM(str(out / 'FlowFW' / 'occ-00000.pfm'))
    assert fl.shape == (48, 64, 3) and np.all(fl[:, :, 2] == 1) and np.all(fl[:, :, 0] == 1)
    assert np.all(occ[-1] == -1) and np.all(occ[:-1] == 0.25)           # rows flipped before write_pfm, as the reference
    bw, _ = util_flow.readPFM(str(out / 'FlowBW' / 'flo-00001.pfm'))
    assert np.all(bw[:, :, 0] == -1)
    from PIL import Image
    m = np.asarray(Image.open(out / 'Annotations' / '00000.png'))
    assert m.dtype == np.uint8 and set(np.unique(m)) == {0, 1}


def test_video_loader_reads_the_written_tree(tmp_path):
    from lasr_amd.dataloader import vid
    ag = _auto_gen()
    dp = _sequence(str(tmp_path), seq='toy', n=4)
    fn, _ = _stub([1., 1., 1.])
    out = tmp_path / 'out'
    ag.run(ag.parse_args(['--datapath', dp, '--outdir', str(out)]), fn)
    for d in ('JPEGImages', 'Annotations', 'FlowFW', 'FlowBW'):              # auto_gen.sh's copy into the DAVIS layout
        dst = tmp_path / 'database' / 'DAVIS' / d / 'Full-Resolution' / 'rtoy'
        shutil.copytree(out / d, dst)
    os.makedirs(tmp_path / 'configs')
    (tmp_path / 'configs' / 'rtoy.config').write_text('[data]\ndatapath = database/DAVIS/JPEGImages/Full-Resolution/rtoy/\n'
                                                      'dframe = 1\ninit_frame = 0\nend_frame = -1\ncan_frame = 1\n')
    opts = SimpleNamespace(dataname='rtoy', sil_path='none', batch_size=1, ngpu=1, local_rank=0, img_size=32, n_data_workers=0)
    loader, length = vid.data_loader(opts, shuffle=False, root=str(tmp_path))
    assert length == 4
    e = loader.dataset[1]
    assert e['img'].shape == (3, 32, 32) and e['flow'].shape == (3, 32, 32) and e['occ'].shape == (32, 32)
    assert np.isfinite(e['flow']).all() and e['mask'].sum() > 0


def test_empty_mask_stops_with_the_file_name(tmp_path):
    from PIL import Image
    ag = _auto_gen()
    dp = _sequence(str(tmp_path), n=3)
    bad = os.path.join(dp.replace('JPEGImages', 'Annotations'), '00001.png')
    Image.fromarray(np.zeros((48, 64), np.uint8)).save(bad)
    fn, _ = _stub([1., 1.])
    with pytest.raises(ag.EmptyMask, match='00001.png'):
        ag.run(ag.parse_args(['--datapath', dp, '--outdir', str(tmp_path / 'out')]), fn)


def test_resize_follows_the_pixel_centre_convention():
    ag = _auto_gen()
    a = np.array([[0, 100], [200, 255]], np.uint8)
    up = ag.resize(a, 4, 4)
    assert up.dtype == np.uint8 and up[0, 0] == 0 and up[3, 3] == 255 and up[0, 1] == 25    # 0.75 * 0 + 0.25 * 100
    f = ag.resize(np.arange(8, dtype=np.float32).reshape(2, 4), 2, 1)
    assert f.dtype == np.float32 and np.allclose(f, [[2.5, 4.5]])


def test_flags_match_the_reference():
    ag = _auto_gen()
    a = ag.parse_args([])
    assert (a.loadmodel, a.testres, a.maxdisp, a.fac, a.flow_threshold, a.outdir) == (None, 1, 256, 1, 0.05, None)
    assert ag.seqname_of('database/DAVIS/JPEGImages/Full-Resolution/camel/') == 'camel'
