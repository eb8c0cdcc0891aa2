"""The training monitor without a device: the restatement of the colour coding against the reference's recorded outputs, the
exported symbols and their host-side argument checks, the command-line surface and the CSV writer."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flowvis_cases as cases          # noqa: E402
import flowvis_restated as restated    # noqa: E402


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'flowvis.npz'))


def test_restatement_equals_the_reference_outputs_bit_for_bit(golden):
    names = [k[3:] for k in golden.files if k.startswith('in_')]
    assert len(names) >= 5
    for n in names:
        flow = golden['in_' + n]
        mask = golden['mask_' + n][None] if 'mask_' + n in golden.files else None
        assert flow.dtype == np.float64
        out, _ = restated.flow_to_image(flow[None], mask)
        assert out.dtype == np.uint8 and (out[0] == golden['out_' + n]).all(), n
    assert (golden['out_zeros'] == 255).all()                       # maximum 0: white
    assert (golden['out_unknown_c3'][3, 5] == 0).all()              # unknown flow: black


def test_color_wheel_shape_and_corners():
    w = restated.color_wheel()
    assert w.shape == (55, 3) and w[0].tolist() == [255, 0, 0] and w[15].tolist() == [255, 255, 0] and w[54].tolist() == [255, 0, 43]


def test_exclusion_band_covers_at_most_four_pixels_per_image_of_the_gpu_inputs():
    for name, (flow, mask) in cases.colour_cases().items():
        _, rad = restated.flow_to_image(flow.astype(np.float64), mask)
        n = (np.abs(rad - 1) < cases.EXCLUDE_BAND).reshape(len(flow), -1).sum(1)
        assert n.max() <= cases.EXCLUDE_MAX_PER_IMAGE, (name, n)
    for cs in cases.SHEET_CASES:
        c = cases.sheet_case(*cs)
        _, radii = restated.sheet({k: None if v is None else np.asarray(v, np.float64) for k, v in cases.sheet_planes(c).items()}, c['IS'])
        assert all((np.abs(r - 1) < cases.EXCLUDE_BAND).sum() <= cases.EXCLUDE_MAX_PER_IMAGE for r in radii)


def test_nan_and_unknown_samples_are_black_and_stay_out_of_the_maximum():
    flow, _ = cases.colour_cases()['unknown_and_nan']
    clean = flow.copy()
    clean[0, 3, 5] = 0
    clean[0, 11, 2] = 0
    a, _ = restated.flow_to_image(flow.astype(np.float64))
    b, _ = restated.flow_to_image(clean.astype(np.float64))
    assert (a[0, 3, 5] == 0).all() and (a[0, 11, 2] == 0).all()
    keep = np.ones((16, 16), bool)
    keep[3, 5] = keep[11, 2] = False
    assert (a[0][keep] == b[0][keep]).all()


def test_sheet_restatement_layout():
    c = cases.sheet_case(16, 4)
    p = cases.sheet_planes(c)
    s, _ = restated.sheet(p, 16, np.float32)
    assert s.shape == (48, 48, 3) and s.dtype == np.uint8
    assert (s[32:48, 0:16] == np.clip(np.floor(255 * c['imgs'][0]), 0, 255).astype(np.uint8).transpose(1, 2, 0)).all()
    assert (s[32:48, 16:32] == np.clip(np.floor(255 * c['imgs'][2]), 0, 255).astype(np.uint8).transpose(1, 2, 0)).all()   # imgs[batch_size]
    ring = restated.ring_mask(16, p['ctl'][2][0], p['ctl'][2][1], np.float32)
    assert 20 <= ring.sum() <= 70 and not restated.ring_mask(16, 1.6, 0.2, np.float32).any()
    assert 0 < restated.ring_mask(16, -1., 0.1, np.float32).sum() < ring.sum()                                             # clipped at the border
    one = cases.sheet_case(16, 1)
    s1, _ = restated.sheet(cases.sheet_planes(one), 16, np.float32)
    assert (s1[16:32, 32:48] == 0).all()                                                                                   # n_bones = 1: black part tile
    const = cases.sheet_case(32, 4, True)
    sc, _ = restated.sheet(cases.sheet_planes(const), 32, np.float32)
    assert (sc[0:32, 64:96] == 0).all()                                                                                    # constant panel: 0


def test_symbols_are_exported_and_validate_on_the_host():
    from lasr_amd import _lib
    h = _lib.lib()
    assert h.lasr_abi_version() == _lib.ABI_VERSION >= 12
    n, p = None, ctypes.c_void_p(64)
    for B, H, W in ((0, 8, 8), (2, 0, 8), (2, 8, 0)):
        assert h.lasr_flow_to_image(n, n, n, n, B, H, W, 2, n) == 0                  # empty: nothing launched
    assert h.lasr_flow_to_image(p, n, p, p, 1, 8, 8, 4, n) == -1                     # channels
    assert h.lasr_flow_to_image(p, n, p, p, 1, 8, 8, 1, n) == -1
    assert h.lasr_flow_to_image(n, n, p, p, 1, 8, 8, 2, n) == -1                     # null pointers
    assert h.lasr_flow_to_image(p, n, n, p, 1, 8, 8, 2, n) == -1
    assert h.lasr_flow_to_image(p, n, p, n, 1, 8, 8, 2, n) == -1
    assert h.lasr_flow_to_image(p, n, p, p, -1, 8, 8, 2, n) == -1
    assert h.lasr_flow_to_image(p, n, ctypes.c_void_p(66), p, 1, 8, 8, 2, n) == -1   # output not 4-byte aligned
    assert h.lasr_flow_to_image_scratch_bytes(3) == 16 and h.lasr_flow_to_image_scratch_bytes(-1) == 0
    inp = _lib.SheetInputs()
    assert h.lasr_monitor_sheet(ctypes.byref(inp), p, p, 0, n) == 0
    assert h.lasr_monitor_sheet(ctypes.byref(inp), p, p, 16, n) == -1                # null planes
    assert h.lasr_monitor_sheet(n, p, p, 16, n) == -1 and h.lasr_monitor_sheet(ctypes.byref(inp), p, p, -1, n) == -1
    assert h.lasr_monitor_sheet(ctypes.byref(inp), p, p, _lib.SHEET_MAX_SIZE + 1, n) == -1
    assert h.lasr_monitor_sheet_scratch_bytes() == 36
    assert h.lasr_scalar_ring_bytes(4, 3) == 48 and h.lasr_scalar_ring_bytes(0, 3) == 0 and h.lasr_scalar_ring_bytes(4, _lib.RING_MAX_SCALARS + 1) == 0
    assert h.lasr_scalar_ring_push(n, 0, n, n, 4, n) == 0
    assert h.lasr_scalar_ring_push(n, 2, p, p, 4, n) == -1 and h.lasr_scalar_ring_push(p, 2, p, p, 0, n) == -1
    assert h.lasr_scalar_ring_push(p, -1, p, p, 4, n) == -1 and h.lasr_scalar_ring_push(p, 2, n, p, 4, n) == -1
    names = [h.lasr_prof_kernel_name(i) for i in range(h.lasr_prof_kernel_count())]
    for k in (b'flow_maxrad_kernel', b'flow_colour_kernel', b'sheet_stats_kernel', b'sheet_compose_kernel', b'scalar_ring_push_kernel'):
        assert k in names


def test_header_constants_and_struct_match_the_python_mirror():
    import re
    from lasr_amd import _lib
    ops = open(os.path.join(ROOT, 'include', 'lasr_ops.h')).read()
    assert int(re.search(r'#define\s+LASR_SHEET_MAX_SIZE\s+(\d+)', ops).group(1)) == _lib.SHEET_MAX_SIZE
    assert int(re.search(r'#define\s+LASR_RING_MAX_SCALARS\s+(\d+)', ops).group(1)) == _lib.RING_MAX_SCALARS
    body = re.search(r'typedef struct lasr_sheet_inputs \{(.*?)\} lasr_sheet_inputs;', ops, re.S).group(1)
    planes = re.search(r'lasr_sheet_plane ([^;]+);', body).group(1).replace(' ', '').split(',')
    assert planes == [n for n, _ in _lib.SheetInputs._fields_[:10]]
    assert [n for n, _ in _lib.SheetInputs._fields_[10:]] == ['ctl', 'palette', 'n_ctl', 'ctl_stride']
    assert ctypes.sizeof(_lib.SheetPlane) == 24 and ctypes.sizeof(_lib.SheetInputs) == 10 * 24 + 24


def test_monitor_flag_defaults_to_off():
    sys.path.insert(0, ROOT)
    import optimize
    o = optimize.parse_flags([])
    assert o.monitor is False and o.monitor_dir == ''
    assert optimize.parse_flags(['--monitor']).monitor is True and optimize.parse_flags(['--monitor', '--nomonitor']).monitor is False
    assert optimize.parse_flags(['--monitor_dir', '/tmp/x']).monitor_dir == '/tmp/x'
    src = open(os.path.join(ROOT, 'scripts', 'render_syn.py')).read()
    assert "'--flowvis', action='store_true'" in src


def test_trainer_builds_no_monitor_without_the_flag(tmp_path):
    sys.path.insert(0, ROOT)
    import optimize
    from lasr_amd.nnutils import train_utils
    tr = train_utils.LASRTrainer(optimize.parse_flags(['--checkpoint_dir', str(tmp_path)]))
    assert tr._monitor() is None
    tr.opts.monitor, tr.rank = True, 1                              # rank 0 only
    assert tr._monitor() is None


def test_csv_writer_round_trips(tmp_path):
    from types import SimpleNamespace
    from lasr_amd.nnutils import monitor
    names = monitor.scalar_names(SimpleNamespace(n_hypo=2, n_bones=3))
    assert names[:4] == ['total_loss', 'mask_loss', 'flow_rd_loss', 'texture_loss'] and 'tex_hypo_1' in names
    assert names[-3:] == ['lmotion_loss', 'grad_meanv_norm', 'grad_cam_norm']
    assert 'lmotion_loss' not in monitor.scalar_names(SimpleNamespace(n_hypo=1, n_bones=1))
    rng = np.random.default_rng(0)
    rows = (rng.standard_normal((5, len(names))) * 10. ** rng.integers(-8, 8, (5, len(names)))).astype(np.float32)
    rows[1, 2] = np.nan
    rows[3, 0] = np.float32(1e-42)                                   # a denormal
    path = str(tmp_path / 'scalars.csv')
    monitor.write_scalar_rows(path, names, [1, 2, 3], rows[:3])
    monitor.write_scalar_rows(path, names, [4, 5], rows[3:])         # appended: one header
    text = open(path).read().splitlines()
    assert text[0] == 'step,' + ','.join(names) and len(text) == 6 and text[1].startswith('1,total_loss=')
    got_names, steps, vals = monitor.read_scalar_rows(path)
    assert got_names == names and steps.tolist() == [1, 2, 3, 4, 5]
    assert vals.dtype == np.float32 and (vals.view(np.uint32) == rows.view(np.uint32))[~np.isnan(rows)].all() and np.isnan(vals[1, 2])
