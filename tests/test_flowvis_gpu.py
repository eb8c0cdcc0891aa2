"""lasr_amd/csrc/flowvis.hip on the device against the numpy restatement (tests/flowvis_restated.py): the Middlebury colour coding,
the epoch contact sheet, the scalar ring, and the monitor end to end through the trainer and scripts/render_syn.py.

Colour-coding criterion: at most 1 level per channel from the float64 restatement, outside the pixels whose
normalised radius lies within 1e-5 of 1 (at most 4 per image; tests/test_flowvis_cpu.py checks that on these inputs), and a share
of values off by one level of at most 4 x the share at which the restatement evaluated in float32 differs from itself in float64
on the same inputs, pooled over every colour-coded image of this file (measured: 1 of 212 250 values)."""
import importlib.util
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import flowvis_cases as cases          # noqa: E402
import flowvis_restated as restated    # noqa: E402


def _tally(got, ref64, ref32, rad):
    """(max level difference, values off, values compared, float32-restatement values off) outside the exclusion band."""
    keep = np.abs(rad - 1) >= cases.EXCLUDE_BAND
    d = np.abs(got.astype(int) - ref64.astype(int))[keep]
    d32 = np.abs(ref32.astype(int) - ref64.astype(int))[keep]
    return int(d.max()) if d.size else 0, int((d > 0).sum()), int(d.size), int((d32 > 0).sum())


@pytest.fixture(scope='module')
def coded(cuda):
    """Every colour-coding case through lasr_flow_to_image once (one statistics scratch serves them all, so a call that left
    it dirty would show in the next), with the restatement in float64 and float32."""
    import torch
    from lasr_amd.ext_utils import flowlib
    out = {}
    for name, (flow, mask) in cases.colour_cases().items():
        t = torch.from_numpy(flow).to(cuda)
        m = None if mask is None else torch.from_numpy(mask).to(cuda)
        got = flowlib.flow_to_image(t, m)
        assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == flow.shape[:3] + (3,)
        ref64, rad = restated.flow_to_image(flow.astype(np.float64), mask)
        ref32, _ = restated.flow_to_image(flow, mask, np.float32)
        out[name] = dict(got=got.cpu().numpy(), ref64=ref64, ref32=ref32, rad=rad, flow=flow, mask=mask)
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope='module')
def sheets(cuda):
    import torch
    from lasr_amd.nnutils import monitor
    scratch = torch.zeros(16, dtype=torch.int32, device=cuda)
    out = {}
    for cs in cases.SHEET_CASES:
        c = cases.sheet_case(*cs)
        IS, B, H, cam = c['IS'], c['batch_size'], c['n_hypo'], c['optim_cam']
        t = {k: torch.from_numpy(v).to(cuda) for k, v in c.items() if isinstance(v, np.ndarray) and k != 'part_render'}
        px = t['px']
        # a view of a wider render, as the trainer holds it
        part = torch.from_numpy(c['part_render'].base).to(cuda)[:, :3] if c['n_bones'] > 1 else None
        planes = dict(flow_obs=(t['flow'][0, :2], 0), flow_rd=(t['flow_rd'].view(2 * B, H, IS, IS, 2)[0, cam], -1),
                      vis_mask=(t['vis_mask'][0, cam], None), flow_err=(t['flow_rd_map'][0, cam], None), mask_pred=(px[:, 9][cam], None),
                      mask_gt=(t['masks'][0], None), part=(part[0] if part is not None else None, 0), img1=(t['imgs'][0], 0),
                      img2=(t['imgs'][B], 0), texture=(px[:, :3][cam], 0))
        ctl = t['ctl_proj'][cam] if c['n_bones'] > 1 else None
        from lasr_amd import synth
        pal = torch.from_numpy(synth.label_palette(max(c['n_bones'] - 1, 1))).to(cuda)
        got = monitor.sheet(planes, ctl, pal, IS, scratch)
        p = cases.sheet_planes(c)
        ref32, _ = restated.sheet(p, IS, np.float32)
        ref64, radii = restated.sheet({k: None if v is None else np.asarray(v, np.float64) for k, v in p.items()}, IS)
        out[cs] = dict(got=got.cpu().numpy(), ref32=ref32, ref64=ref64, radii=radii, IS=IS)
    assert int(scratch.abs().sum()) == 0                                      # the calls leave the statistics words zero
    return out


@pytest.mark.parametrize('name', list(cases.colour_cases()))
def test_colour_coding_within_one_level_of_the_restatement(coded, name):
    r = coded[name]
    worst, off, n, off32 = _tally(r['got'], r['ref64'], r['ref32'], r['rad'])
    excluded = (np.abs(r['rad'] - 1) < cases.EXCLUDE_BAND).reshape(len(r['rad']), -1).sum(1)
    print('%s: max diff %d, off by one %d of %d (float32 restatement: %d), excluded per image %s' % (name, worst, off, n, off32, excluded))
    assert excluded.max() <= cases.EXCLUDE_MAX_PER_IMAGE
    assert worst <= 1


def test_colour_coding_special_pixels(coded):
    assert (coded['zeros_8x8']['got'] == 255).all()                            # maximum 0: white, as the reference gives
    g = coded['unknown_and_nan']['got'][0]
    assert (g[3, 5] == 0).all() and (g[11, 2] == 0).all()                      # unknown and NaN samples: black
    m = coded['masked']
    assert (m['got'][m['mask'] == 0] == 255).all()                             # masked samples are (0, 0): white
    assert coded['one_pixel']['got'].shape == (1, 1, 1, 3)


def test_share_of_values_off_by_one_level(coded, sheets):
    off = n = off32 = 0
    for r in coded.values():
        _, a, b, c = _tally(r['got'], r['ref64'], r['ref32'], r['rad'])
        off, n, off32 = off + a, n + b, off32 + c
    for s in sheets.values():
        IS = s['IS']
        for j, rad in enumerate(s['radii']):
            tile = (slice(0, IS), slice(j * IS, (j + 1) * IS))
            _, a, b, c = _tally(s['got'][tile], s['ref64'][tile], s['ref32'][tile], rad)
            off, n, off32 = off + a, n + b, off32 + c
    cap = 4 * off32
    print('off by one level: kernel %d of %d (%.3g), float32 restatement %d (%.3g), cap %d' % (off, n, off / n, off32, off32 / n, cap))
    assert off <= cap


def test_numpy_input_returns_numpy(cuda):
    from lasr_amd.ext_utils import flowlib
    flow, _ = cases.colour_cases()['three_channels']
    got = flowlib.flow_to_image(flow[0])
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == (12, 20, 3)
    ref, rad = restated.flow_to_image(flow[:1].astype(np.float64))
    assert np.abs(got.astype(int) - ref[0].astype(int))[np.abs(rad[0] - 1) >= cases.EXCLUDE_BAND].max() <= 1
    with pytest.raises(ValueError):
        flowlib.flow_to_image(np.zeros((4, 4, 4), np.float32))


@pytest.mark.parametrize('cs', cases.SHEET_CASES, ids=lambda c: 'IS%d_bones%d%s' % (c[0], c[1], '_const' if c[2] else ''))
def test_contact_sheet(sheets, cs):
    s = sheets[cs]
    IS, got, ref = s['IS'], s['got'], s['ref32']
    assert got.shape == (3 * IS, 3 * IS, 3) and got.dtype == np.uint8
    names = ('flowobs', 'flowrd', 'flow_error', 'mask', 'maskgt', 'part', 'img1', 'img2', 'texture')
    for k, name in enumerate(names):
        tile = (slice((k // 3) * IS, (k // 3 + 1) * IS), slice((k % 3) * IS, (k % 3 + 1) * IS))
        if k < 2:                                                              # the two flow panels: the colour-coding criterion
            worst, off, n, off32 = _tally(got[tile], s['ref64'][tile], s['ref32'][tile], s['radii'][k])
            print('%s: max diff %d, off %d of %d' % (name, worst, off, n))
            assert worst <= 1, name
        else:                                                                  # everything else: exact in float32
            assert (got[tile] == ref[tile]).all(), (name, int(np.abs(got[tile].astype(int) - ref[tile].astype(int)).max()))
    if cs[1] == 1:
        assert (got[IS:2 * IS, 2 * IS:] == 0).all()                            # n_bones = 1: black part tile
    if cs[2]:
        assert (got[:IS, 2 * IS:] == 0).all()                                  # constant flow_error panel: 0


def test_scalar_ring_wraps_and_sums_in_fixed_order(cuda):
    import torch
    from lasr_amd.nnutils import monitor
    K, cap = len(cases.RING_COUNTS), 4
    pushes = cases.ring_pushes(5)
    ring = monitor.ScalarRing(K, cap, cuda)
    # two tables at different addresses feed one ring: pushes alternate between two sets of device tensors
    sets = [[torch.empty(n, device=cuda) for n in cases.RING_COUNTS] for _ in range(2)]
    rows_seen = []
    for n, vals in enumerate(pushes):
        dst = sets[n % 2]
        for d, v in zip(dst, vals):
            d.copy_(torch.from_numpy(v))
        ring.push(dst)
        if n == 2:
            rows_seen = ring.drain(0)                                           # three rows, oldest first
    assert len(ring._tables) == 2
    ref, head = restated.ring(pushes, cap)
    torch.cuda.synchronize()
    assert int(ring.head) == head == 5 and ring.pushed == 5
    got = ring.ring.cpu().numpy()
    for n, vals in enumerate(pushes):
        for k, v in enumerate(vals):
            bound = len(v) * 2. ** -24 * np.abs(v.astype(np.float64)).mean()
            mean = v.astype(np.float64).mean()
            if n >= 1:                                                          # push 0 was overwritten by push 4
                assert abs(float(got[n % cap, k]) - mean) <= bound, (n, k, got[n % cap, k], mean, bound)
            if n <= 2:
                assert abs(float(rows_seen[n, k]) - mean) <= bound
    assert np.allclose(got, ref, rtol=1e-5)
    last = ring.drain(1)                                                         # pushes 1..4 in push order, across the wrap
    assert last.shape == (4, K) and (last == got[[1, 2, 3, 0]]).all()
    with pytest.raises(ValueError):
        ring.drain(0)                                                            # push 0 is gone
    # the same push twice gives the same bits; a missing value is NaN
    a = monitor.ScalarRing(K, 2, cuda)
    a.push(sets[0])
    a.push(sets[0])
    a.push([None] + sets[0][1:])
    r = a.ring.cpu().numpy()
    assert np.isnan(r[0, 0]) and (r[0, 1:].view(np.uint32) == r[1, 1:].view(np.uint32)).all()


def _trainer(tmp_path, name, use_graph, monitor_on):
    import torch
    import optimize
    from lasr_amd.nnutils import train_utils
    # the sizes of tests/test_reconstruction_deterministic_gpu.py (stage 0), on the in-memory synthetic sequence
    argv = ['--name', name, '--checkpoint_dir', str(tmp_path), '--dataname', 'synthetic', '--n_frames', '4', '--img_size', '128',
            '--n_hypo', '4', '--n_bones', '21', '--subdivide', '3', '--batch_size', '1', '--opt_tex', 'yes', '--nouse_gtpose',
            '--only_mean_sym', '--num_epochs', '2', '--iters_per_epoch', '3', '--deterministic',
            '--use_graph' if use_graph else '--nouse_graph'] + (['--monitor'] if monitor_on else [])
    opts = optimize.parse_flags(argv)
    torch.manual_seed(0)
    np.random.seed(0)
    tr = train_utils.LASRTrainer(opts).init_training()
    returned = []
    step = tr.train_step

    def recording(batch):
        loss, aux = step(batch)
        returned.append(loss.clone())
        return loss, aux
    tr.train_step = recording
    assert tr.train() == 6
    torch.cuda.synchronize()
    return tr, [float(x) for x in returned]


@pytest.mark.parametrize('use_graph', [True, False], ids=['graph', 'eager'])
def test_monitor_end_to_end(tmp_path, cuda, use_graph):
    import torch
    from PIL import Image
    from lasr_amd.nnutils import monitor
    try:
        tr, returned = _trainer(tmp_path, 'mon', use_graph, True)
        plain, returned_plain = _trainer(tmp_path, 'plain', use_graph, False)
    finally:
        torch.cuda.set_stream(torch.cuda.default_stream())                      # the trainer switched the current stream
        torch.use_deterministic_algorithms(False)
        torch.backends.cudnn.deterministic = False
    mdir = os.path.join(str(tmp_path), 'mon', 'monitor')
    assert sorted(os.listdir(mdir)) == ['epoch-0000.png', 'epoch-0001.png', 'scalars.csv']
    for e in range(2):
        im = np.asarray(Image.open(os.path.join(mdir, 'epoch-%04d.png' % e)))
        assert im.shape == (3 * 128, 3 * 128, 3) and im.dtype == np.uint8
        assert im[256:, :256].std() > 0 and im[:128, :256].std() > 0            # input frames and flow panels are not blank
    names, steps, vals = monitor.read_scalar_rows(os.path.join(mdir, 'scalars.csv'))
    assert names == monitor.scalar_names(tr.opts) and steps.tolist() == [1, 2, 3, 4, 5, 6] and vals.shape == (6, len(names))
    assert [float(v) for v in vals[:, 0]] == [float(np.float32(x)) for x in returned]      # total_loss, bit for bit
    assert np.isfinite(vals[:, :names.index('grad_meanv_norm')]).all()
    assert np.isfinite(vals[1:]).all()                                                        # the gradient norms from their first step on
    assert not os.path.exists(os.path.join(str(tmp_path), 'plain', 'monitor'))
    # watching changes nothing: same losses, same final parameters
    assert returned == returned_plain
    for (n, a), (_, b) in zip(tr.module.named_parameters(), plain.module.named_parameters()):
        assert torch.equal(a, b), n


def test_render_syn_writes_the_coloured_flow(tmp_path, cuda):
    from PIL import Image
    spec = importlib.util.spec_from_file_location('render_syn', os.path.join(ROOT, 'scripts', 'render_syn.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.main(['--outdir', 'fv', '--nframes', '2', '--img_size', '64', '--root', str(tmp_path), '--flowvis'])
    base = os.path.join(str(tmp_path), 'database', 'DAVIS')
    for d, i in (('FlowFW', 0), ('FlowBW', 1)):
        im = np.asarray(Image.open(os.path.join(base, d, 'Full-Resolution', 'fv', 'col-%05d.jpg' % i)))
        assert im.shape == (64, 64, 3) and (im[0, 0] >= 250).all() and im.min() < 200       # white background, a coloured object
    mod.main(['--outdir', 'plain', '--nframes', '2', '--img_size', '64', '--root', str(tmp_path)])
    assert not [f for f in os.listdir(os.path.join(base, 'FlowFW', 'Full-Resolution', 'plain')) if f.startswith('col-')]
