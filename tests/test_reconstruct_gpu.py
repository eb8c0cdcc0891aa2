"""scripts/reconstruct.py on the GPU (lasr_amd/pipeline.py), as a user runs it: the driver is one child process
under one overall `timeout -k 10`, and the tests assert on what it left behind.

G1, the preprocessing leg: on the 8 frames of motionseg_restated.sequence('pan') the driver must leave, byte for byte, what
auto_mask.py and the two passes of auto_gen.py leave when they are run by hand in this process with the same flags and
varflow.make_flow_fn() (the pieces promise identical bits on two runs): the driver adds nothing and loses nothing.  No quality bar is
set here.  The driver runs `--until config`, not `--until flow`: the config step follows the flow passes in the plan and the configs
are part of what is compared.  The frames are 64 x 80 and the object covers about 520 pixels, so --min_area 100 goes through to
auto_mask.py after `--` (its default, 1000, would write no mask).

G2, the reconstruction leg: on a 4-frame sequence of scripts/render_syn.py (its own masks and flows), `--from config --glb` with a
schedule file of two stages at the sizes of tests/test_reconstruction_deterministic_gpu.py; the second stage has --n_faces 1600, so
the re-mesh hand-off is crossed.  An epoch of a sequence on disk is the loader's 200 iterations whatever --iters_per_epoch says.
The .glb is read with the independent reader of tests/rig_restated.py, which tests/test_rig_cpu.py holds against the writer of
lasr_amd/ext_utils/gltf.py (the writer's module has no reader of its own).  The explicit limit of 300 s per stage is the measured
cold start of a stage, 74.4 s, times the margin of 4.  Measured on an MI355X: see the numbers at the end of
DESIGN.md section 4.20; the test is long because it starts nine processes, not because of the work.
"""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import motionseg_restated as ms
import rig_restated

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
PY = sys.executable
DRIVER = os.path.join(ROOT, 'scripts', 'reconstruct.py')
KINDS = ('JPEGImages', 'Annotations', 'FlowFW', 'FlowBW')


def davis(root, kind, seq):
    return os.path.join(str(root), 'database', 'DAVIS', kind, 'Full-Resolution', seq)


def drive(limit, *argv):
    """The driver as one child under one overall limit.  -> (return code, output)."""
    p = subprocess.run(['timeout', '-k', '10', str(limit), PY, DRIVER] + list(argv), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       universal_newlines=True)
    print(p.stdout)
    return p.returncode, p.stdout


def tree(folder):
    """relative path -> bytes of every file under folder."""
    out = {}
    for d, _, files in os.walk(folder):
        for f in files:
            with open(os.path.join(d, f), 'rb') as fh:
                out[os.path.relpath(os.path.join(d, f), folder)] = fh.read()
    return out


def test_preprocessing_leg_leaves_what_the_scripts_leave_by_hand(cuda, tmp_path, monkeypatch):
    from PIL import Image
    seq = ms.sequence('pan')
    src = tmp_path / 'in'
    os.makedirs(str(src))
    for t, f in enumerate(seq.frames):
        Image.fromarray(f).save(str(src / ('f%d.png' % t)))
    work = tmp_path / 'driver'
    rc, out = drive(600, '--frames', str(src), '--seqname', 'pan', '--workdir', str(work), '--until', 'config', '--', '--min_area', '100')
    assert rc == 0, out
    assert not os.path.isdir(str(work / 'log')) and not os.path.exists(str(work / 'reconstruct' / 'steps' / '05-stage-0.log'))

    # the same by hand, in this process
    for p in (ROOT, os.path.join(ROOT, 'preprocess')):
        if p not in sys.path:
            sys.path.insert(0, p)
    import auto_gen
    import auto_mask
    from lasr_amd.nnutils import varflow
    hand = tmp_path / 'hand'
    os.makedirs(davis(hand, 'JPEGImages', 'pan'))
    for t, f in enumerate(seq.frames):
        Image.fromarray(f).save(os.path.join(davis(hand, 'JPEGImages', 'pan'), '%05d.jpg' % t), quality=95)
    monkeypatch.chdir(str(hand))
    datapath = 'database/DAVIS/JPEGImages/Full-Resolution/pan/'
    flow_fn = varflow.make_flow_fn()
    auto_mask.run(auto_mask.parse_args(['--datapath', datapath, '--flow_method', 'variational', '--force', '--min_area', '100']), flow_fn)
    common = ['--datapath', datapath, '--flow_method', 'variational', '--testres', '1']
    kept = auto_gen.run(auto_gen.parse_args(common + ['--outdir', './rpan']), flow_fn)
    for k in KINDS:
        shutil.copytree(os.path.join('rpan', k), davis(hand, k, 'rpan'))
    auto_gen.run(auto_gen.parse_args(common + ['--flow_threshold', '0', '--outdir', './pan']), flow_fn)
    for k in ('FlowFW', 'FlowBW'):
        shutil.copytree(os.path.join('pan', k), davis(hand, k, 'pan'))
    os.makedirs('configs')
    for name in ('pan', 'rpan'):
        with open('configs/%s.config' % name, 'w') as fh:
            fh.write('[data]\ndatapath = database/DAVIS/JPEGImages/Full-Resolution/%s/\ndframe = 1\ninit_frame = 0\nend_frame = -1\ncan_frame = 0\n' % name)

    for name in ('pan', 'rpan'):
        for k in KINDS:
            want, have = tree(davis(hand, k, name)), tree(davis(work, k, name))
            assert sorted(want) == sorted(have) and want, (name, k, sorted(want), sorted(have))
            differ = [f for f in want if want[f] != have[f]]
            assert not differ, (name, k, differ)
    assert len(tree(davis(hand, 'FlowFW', 'pan'))) == 2 * 7 and len(tree(davis(hand, 'FlowFW', 'rpan'))) == 2 * len(kept) > 0
    assert 'maskprop.json' in tree(davis(hand, 'Annotations', 'pan'))
    assert tree(str(hand / 'configs')) == tree(str(work / 'configs')) and len(tree(str(work / 'configs'))) == 2
    from lasr_amd import recon_io
    assert len(recon_io.frame_list('pan')) == 8 and len(recon_io.frame_list('rpan')) == len(kept) + 1


def test_reconstruction_leg_resumes_and_ends_in_a_report(cuda, tmp_path):
    work = tmp_path / 'work'
    os.makedirs(str(work))
    syn = subprocess.run(['timeout', '-k', '10', '300', PY, os.path.join(ROOT, 'scripts', 'render_syn.py'), '--nframes', '4', '--outdir', 'syn',
                          '--root', str(work)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert syn.returncode == 0, syn.stdout
    small = {'use_gtpose': False, 'subdivide': 3, 'img_size': 128, 'num_epochs': 1, 'iters_per_epoch': 20, 'deterministic': True,
             'batch_size': 1, 'timeout_s': 300}
    schedule = tmp_path / 'two.json'
    schedule.write_text(json.dumps([dict(small, only_mean_sym=True, n_bones=21, n_hypo=4),
                                    dict(small, symmetric=False, n_bones=26, n_faces=1600, n_hypo=1)]))
    argv = ['--seqname', 'syn', '--workdir', str(work), '--from', 'config', '--glb', '--schedule', str(schedule)]
    rc, out = drive(1100, *argv)
    assert rc == 0, out
    last = work / 'log' / 'syn-1'
    for i in range(4):
        assert os.path.exists(str(last / ('pred%d.ply' % i))) and os.path.exists(str(last / ('cam%d.txt' % i)))
    assert os.path.exists(str(last / 'rig.npz'))
    for name in ('reproj', 'shape'):
        means = json.load(open(str(work / 'reconstruct' / (name + '.json'))))['means']
        values = [v for v in means.values() if v is not None]
        assert values and np.isfinite(values).all(), (name, means)
    assert all(json.load(open(str(work / 'reconstruct' / 'reproj.json')))['means'][k] is not None for k in ('J', 'F', 'JF'))
    assert json.load(open(str(work / 'reconstruct' / 'shape.json')))['means']['ratio'] is not None
    report = json.load(open(str(work / 'reconstruct' / 'report.json')))
    assert [s['name'] for s in report['stages']] == ['stage-0', 'stage-1'] and all(s['seconds'] > 0 for s in report['stages'])
    assert report['stages'][1]['flags']['n_faces'] == 1600 and report['sequence']['frames'] == 4
    assert 'reconstruct/syn.glb' in report['exports'] and os.path.exists(str(work / 'reconstruct' / 'report.md'))
    with open(str(work / 'reconstruct' / 'syn.glb'), 'rb') as fh:
        gltf, binary = rig_restated.read_glb(fh.read())
    pos = rig_restated.read_accessor(gltf, binary, gltf['meshes'][0]['primitives'][0]['attributes']['POSITION'])
    assert pos.shape[1] == 3 and np.isfinite(pos).all() and len(gltf['animations']) == 1
    print({k: v for k, v in report['seconds'].items()})

    sdir = str(work / 'reconstruct' / 'steps')
    ran = sorted(f for f in os.listdir(sdir) if f.endswith('.json'))
    assert ran == ['04-config.json', '05-stage-0.json', '06-stage-1.json', '07-extract.json', '08-scores-reproj.json', '09-scores-shape.json',
                   '10-glb.json']
    before = {f: (os.stat(os.path.join(sdir, f)).st_mtime_ns, open(os.path.join(sdir, f), 'rb').read()) for f in os.listdir(sdir)}
    rc, out = drive(300, *argv)
    assert rc == 0, out
    after = {f: (os.stat(os.path.join(sdir, f)).st_mtime_ns, open(os.path.join(sdir, f), 'rb').read()) for f in os.listdir(sdir)}
    assert after == before                                                     # no stamp rewritten, no log touched: no child started
    assert out.count('up to date') == 7 and 'limit' not in out
