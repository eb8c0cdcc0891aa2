"""scripts/reconstruct.py without a GPU (lasr_amd/pipeline.py): the plan as data, the flags every step hands
to the script it runs held against that script's own parser, the in-process steps on real files, and the runner's rules (one child at a
time, its own time limit, stop at the first failure, no retry, stamps and resume) on children that are `python -c` one-liners."""
import importlib.util
import io
import json
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lasr_amd import pipeline as pl          # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'reconstruct_schedules.json')
PY = sys.executable


def load(*parts):
    name = os.path.splitext(parts[-1])[0]
    folder = os.path.join(ROOT, *parts[:-1])
    if folder not in sys.path:
        sys.path.insert(0, folder)                           # auto_mask.py imports its neighbours by name
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, *parts))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_args(tmp_path, *extra, frames=8, size=(80, 64)):
    argv = ['--frames', str(tmp_path / 'in'), '--seqname', 'cat', '--workdir', str(tmp_path / 'work')] + list(extra)
    args = pl.parse_args(argv, cwd=str(tmp_path))
    args.n_frames, (args.width, args.height) = frames, size
    return args


def by_name(steps):
    return {s.name: s for s in steps}


def explicit_flags(tokens, defaults):
    """The flags named on an optimize.py command line, --noflag counted as flag."""
    out = set()
    for t in tokens:
        if t.startswith('--'):
            key = t[2:].split('=')[0]
            out.add(key[2:] if key not in defaults and key.startswith('no') and key[2:] in defaults else key)
    return out


# ---- the plan ------------------------------------------------------------------------------------------------------------------
def test_plan_is_pure_and_ordered(tmp_path):
    a = pl.plan(make_args(tmp_path, '--glb', '--gif', '--atlas', '--tracks'))
    b = pl.plan(make_args(tmp_path, '--glb', '--gif', '--atlas', '--tracks'))
    assert a == b and not (tmp_path / 'work').exists()
    assert [s.name for s in a] == ['install', 'masks', 'flow-r', 'flow', 'config', 'stage-0', 'stage-1', 'extract', 'scores-reproj',
                                   'scores-shape', 'gif', 'atlas', 'glb', 'tracks']
    work = str(tmp_path / 'work')
    for s in a:
        assert s.cwd == work and s.timeout_s > 0 and (s.argv is None or s.argv[0] == PY)
        assert all(not os.path.isabs(o) for o in s.outputs)
    assert all(not os.path.isabs(i) for s in a[2:] for i in s.inputs)          # only install and masks read outside the work directory
    glb = by_name(a)['glb'].argv
    assert glb[glb.index('--texture_obj') + 1] == 'reconstruct/baked.obj'     # the atlas before it is embedded
    assert '--texture_obj' not in by_name(pl.plan(make_args(tmp_path, '--glb')))['glb'].argv
    assert [s.name for s in pl.plan(make_args(tmp_path))][-1] == 'scores-shape'


def test_plan_needs_the_frames_count_and_size(tmp_path):
    args = make_args(tmp_path)
    args.n_frames = None
    with pytest.raises(pl.PipelineError):
        pl.plan(args)


@pytest.mark.parametrize('schedule', ['template', 'quick'])
def test_stage_flags_equal_the_recorded_schedule_and_parse(tmp_path, schedule):
    import optimize
    golden = json.load(open(GOLDEN))[schedule]
    stages = [s for s in pl.plan(make_args(tmp_path, '--schedule', schedule)) if s.name.startswith('stage-')]
    assert [s.name for s in stages] == ['stage-%d' % k for k in range(len(golden))] and len(golden) == dict(template=6, quick=2)[schedule]
    for k, (step, want) in enumerate(zip(stages, golden)):
        assert step.argv[1] == os.path.join(ROOT, 'optimize.py')
        opts = optimize.parse_flags(list(step.argv[2:]))
        driver = {'name', 'checkpoint_dir'} | ({'model_path'} if k else set())
        assert explicit_flags(step.argv[2:], optimize.DEFAULTS) == set(want) | driver, (k, step.argv)
        for key, val in want.items():
            assert getattr(opts, key) == (val.replace('{seq}', 'cat') if key == 'dataname' else val), (k, key)
        assert opts.name == 'cat-%d' % k and opts.checkpoint_dir == 'log/'
        assert opts.model_path == ('log/cat-%d/pred_net_latest.pth' % (k - 1) if k else '')
        assert step.outputs == ('log/cat-%d/pred_net_latest.pth' % k,)
        assert (opts.model_path in step.inputs) == bool(k) and 'configs/%s.config' % opts.dataname in step.inputs


def test_a_schedule_file_of_the_user_and_its_explicit_limits(tmp_path):
    path = tmp_path / 'mine.json'
    path.write_text(json.dumps([{'n_bones': 21, 'num_epochs': 1, 'timeout_s': 77, 'monitor': True},
                                {'symmetric': False, 'num_epochs': 2, 'dataname': 'r{seq}'}]))
    steps = by_name(pl.plan(make_args(tmp_path, '--schedule', str(path), '--timeout_scale', '3')))
    one = by_name(pl.plan(make_args(tmp_path, '--schedule', str(path))))
    assert steps['stage-0'].timeout_s == 77 == one['stage-0'].timeout_s                      # explicit: not scaled
    assert steps['stage-1'].timeout_s >= 3 * one['stage-1'].timeout_s - 3 > one['stage-1'].timeout_s
    assert '--monitor' in steps['stage-0'].argv and '--nosymmetric' in steps['stage-1'].argv
    assert steps['stage-1'].argv[steps['stage-1'].argv.index('--dataname') + 1] == 'rcat'
    assert steps['extract'].argv[steps['extract'].argv.index('--dataname') + 1] == 'cat'   # extract always reads the full sequence
    bad = tmp_path / 'bad.json'
    bad.write_text(json.dumps([{'ngpu': 2}]))
    with pytest.raises(pl.PipelineError):
        pl.plan(make_args(tmp_path, '--schedule', str(bad)))
    bad.write_text('{}')
    with pytest.raises(SystemExit):
        make_args(tmp_path, '--schedule', str(bad))


def test_limits_come_from_the_measured_table(tmp_path):
    assert pl.MARGIN == 4 and re.fullmatch(r'\d{4}-\d{2}-\d{2}', pl.MEASURED_ON)
    assert set(pl.MEASURED) == {'masks', 'flow', 'stage', 'extract', 'eval_reproj', 'eval_shape', 'render_vis', 'bake_texture',
                                'export_gltf', 'export_tracks'}
    assert all(s > 0 and r > 0 for s, r in pl.MEASURED.values())
    steps = by_name(pl.plan(make_args(tmp_path, '--schedule', 'quick')))
    s, r = pl.MEASURED['flow']
    assert steps['flow'].timeout_s == int(np.ceil((s + 2 * 7 * 80 * 64 / r) * 4)) == steps['flow-r'].timeout_s
    s, r = pl.MEASURED['stage']
    assert steps['stage-0'].timeout_s == int(np.ceil((s + 5 * 200 / r) * 4))                 # spot3 stage 0: the measured configuration
    assert steps['stage-1'].timeout_s == int(np.ceil((s + 10 * 200 * 1600 / 1280 / r) * 4))
    s, r = pl.MEASURED['extract']
    assert steps['extract'].timeout_s == int(np.ceil((s + 8 / r) * 4))
    twice = by_name(pl.plan(make_args(tmp_path, '--timeout_scale', '2')))
    assert abs(twice['flow'].timeout_s - 2 * steps['flow'].timeout_s) <= 1


def test_every_argv_parses_with_the_parser_of_the_script_it_starts(tmp_path):
    import extract
    import optimize
    key = str(tmp_path / 'first.png')
    steps = by_name(pl.plan(make_args(tmp_path, '--key', '0:' + key, '--key', '5:' + key, '--glb', '--gif', '--atlas', '--tracks', '--worst', '3')))
    data = 'database/DAVIS/JPEGImages/Full-Resolution/cat/'
    for name in ('stage-0', 'stage-1'):
        optimize.parse_flags(list(steps[name].argv[2:]))
    e = extract.parse_flags(list(steps['extract'].argv[2:]))
    last = optimize.parse_flags(list(steps['stage-1'].argv[2:]))
    assert e.rig and not e.render and e.model_path == 'log/cat-1/pred_net_latest.pth' and e.name == 'cat-1' and e.dataname == 'cat'
    assert all(getattr(e, k) == getattr(last, k) for k in vars(last) if k not in ('model_path', 'dataname'))
    pm = load('preprocess', 'propagate_mask.py').parse_args(list(steps['masks'].argv[2:]))
    assert steps['masks'].argv[1].endswith('preprocess/propagate_mask.py') and pm.key == [(0, key), (5, key)] and pm.datapath == data and pm.force
    gen = load('preprocess', 'auto_gen.py')
    r, full = gen.parse_args(list(steps['flow-r'].argv[2:])), gen.parse_args(list(steps['flow'].argv[2:]))
    assert (r.flow_threshold, r.outdir, full.flow_threshold, full.outdir) == (0.05, './rcat', 0., './cat') and r.datapath == full.datapath == data
    for name, parts, out in (('scores-reproj', ('scripts', 'eval_reproj.py'), 'reconstruct/reproj.json'),
                             ('scores-shape', ('scripts', 'eval_shape.py'), 'reconstruct/shape.json'),
                             ('atlas', ('scripts', 'bake_texture.py'), 'reconstruct/baked'),
                             ('tracks', ('scripts', 'export_tracks.py'), 'reconstruct/tracks.npz'),
                             ('glb', ('scripts', 'export_gltf.py'), 'reconstruct/cat.glb'), ('gif', ('render_vis.py',), 'reconstruct/cat.gif')):
        assert steps[name].argv[1] == os.path.join(ROOT, *parts)
        a = load(*parts).parse_args(list(steps[name].argv[2:]))
        assert a.testdir == 'log/cat-1/' and a.outpath == out and getattr(a, 'seqname', 'cat') == 'cat' and getattr(a, 'worst', 3) == 3
    am = load('preprocess', 'auto_mask.py').parse_args(list(by_name(pl.plan(make_args(tmp_path)))['masks'].argv[2:]))
    assert am.datapath == data and am.force and not am.keys_only


def test_flags_after_the_double_dash_reach_the_scripts_that_own_them(tmp_path):
    extra = ['--', '--vf_alpha', '0.05', '--ms_gap', '3', '--min_area', '100', '--hi', '0.8', '--roundtrip', '--testres', '0.5', '--n_keys', '2']
    steps = by_name(pl.plan(make_args(tmp_path, *extra)))
    am = load('preprocess', 'auto_mask.py').parse_args(list(steps['masks'].argv[2:]))
    assert (am.vf_alpha, am.ms_gap, am.min_area, am.hi, am.roundtrip, am.testres, am.ms_n_keys) == (0.05, 3, 100, 0.8, True, 0.5, 2)
    for name in ('flow-r', 'flow'):
        g = load('preprocess', 'auto_gen.py').parse_args(list(steps[name].argv[2:]))
        assert (g.vf_alpha, g.testres) == (0.05, 0.5) and not {'--ms_gap', '--min_area', '--hi', '--roundtrip', '--n_keys'} & set(steps[name].argv)
        assert list(steps[name].argv[-4:]) == ['--vf_alpha', '0.05', '--testres', '0.5']       # verbatim, in the user's order
    key = str(tmp_path / 'k.png')
    pm = load('preprocess', 'propagate_mask.py').parse_args(list(by_name(pl.plan(make_args(tmp_path, '--key', '2:' + key, *extra)))['masks'].argv[2:]))
    assert (pm.vf_alpha, pm.min_area, pm.hi, pm.roundtrip, pm.testres) == (0.05, 100, 0.8, True, 0.5)
    with pytest.raises(SystemExit):
        make_args(tmp_path, '--', '--no_such_flag', '1')
    with pytest.raises(SystemExit):
        make_args(tmp_path, '--', 'stray')


def test_the_pass_through_table_names_flags_the_owning_parsers_know(tmp_path):
    mods = {n: load('preprocess', n + '.py') for n in pl.FLOW_OWNERS}
    base = {'auto_gen': [], 'auto_mask': ['--datapath', 'x/JPEGImages/y'], 'propagate_mask': ['--datapath', 'x/JPEGImages/y', '--key', '0:k.png']}
    for flag, owners in pl.PASS_FLAGS.items():
        for o in owners:
            mods[o].parse_args(base[o] + ['--' + flag] + ([] if flag == 'roundtrip' else ['1']))
    am = load('preprocess', 'auto_mask.py')
    for name, _, _, _ in mods['auto_gen'].FLOW_TUNING:
        assert pl.route_passthrough(['--vf_' + name, '1']) == {o: ['--vf_' + name, '1'] for o in pl.FLOW_OWNERS}
    for name, _, _, _ in am.MOTION:
        routed = pl.route_passthrough(['--ms_' + name, '1'])
        assert routed['auto_mask'] == ['--ms_' + name, '1'] and not routed['auto_gen'] and not routed['propagate_mask']
    for name, _, _, _ in mods['propagate_mask'].TUNING:
        assert pl.PASS_FLAGS[name] == pl.MASK_OWNERS


def test_three_mask_routes(tmp_path):
    given = by_name(pl.plan(make_args(tmp_path, '--masks', 'sil')))['masks']
    keyed = by_name(pl.plan(make_args(tmp_path, '--key', '0:a.png')))['masks']
    auto = by_name(pl.plan(make_args(tmp_path)))['masks']
    assert given.argv is None and given.pre == (('install_masks', str(tmp_path / 'sil'), 'cat'),)
    assert keyed.argv[1].endswith('propagate_mask.py') and auto.argv[1].endswith('auto_mask.py')
    assert keyed.argv[keyed.argv.index('--key') + 1] == '0:' + str(tmp_path / 'a.png')        # the child runs in the work directory
    assert len({given, keyed, auto}) == 3
    assert given.outputs == keyed.outputs == auto.outputs == ('database/DAVIS/Annotations/Full-Resolution/cat',)
    with pytest.raises(SystemExit):
        make_args(tmp_path, '--masks', 'sil', '--key', '0:a.png')


def test_nothing_downloaded_defaults_and_what_weights_change(tmp_path):
    plain = by_name(pl.plan(make_args(tmp_path)))
    for name in ('masks', 'flow-r', 'flow'):
        a = plain[name].argv
        assert a[a.index('--flow_method') + 1] == 'variational' and '--loadmodel' not in a
    for name in ('stage-0', 'stage-1', 'extract'):
        a = plain[name].argv
        assert a[a.index('--ptex_method') + 1] == 'ssim' and '--alexnet_weights' not in a and '--use_graph' in a
        assert a[a.index('--sil_path') + 1] == 'none' and a[a.index('--opt_tex') + 1] == 'yes' and a[a.index('--ngpu') + 1] == '1'
    full = by_name(pl.plan(make_args(tmp_path, '--loadmodel', 'vcn_rob.pth', '--alexnet_weights', 'alex.pth', '--encoder_weights', 'r18.pth')))
    for name in ('masks', 'flow-r', 'flow'):
        a = full[name].argv
        assert 'variational' not in a and a[a.index('--loadmodel') + 1] == str(tmp_path / 'vcn_rob.pth')
    for name in ('stage-0', 'stage-1', 'extract'):
        a = full[name].argv
        assert '--ptex_method' not in a and 'ssim' not in a and a[a.index('--alexnet_weights') + 1] == str(tmp_path / 'alex.pth')
        assert a[a.index('--encoder_weights') + 1] == str(tmp_path / 'r18.pth')
    assert 'variational' in pl.describe(make_args(tmp_path))['pieces'] and 'ssim' in pl.describe(make_args(tmp_path))['pieces']
    with pytest.raises(SystemExit):
        make_args(tmp_path, '--loadmodel', 'vcn_rob.pth', '--flow_method', 'variational')


# ---- the in-process steps ------------------------------------------------------------------------------------------------------
def write_images(folder, names, size=(40, 24), seed=0):
    from PIL import Image
    os.makedirs(str(folder), exist_ok=True)
    rng = np.random.default_rng(seed)
    imgs = {}
    for n in names:
        imgs[n] = rng.integers(0, 255, (size[1], size[0], 3), dtype=np.uint8)
        Image.fromarray(imgs[n]).save(os.path.join(str(folder), n), **(dict(quality=95) if n.endswith('.jpg') else {}))
    return imgs


def test_install_orders_naturally_and_writes_jpeg_95(tmp_path):
    from PIL import Image
    src, work = tmp_path / 'in', str(tmp_path / 'work')
    imgs = write_images(src, ['10.png', '1.png', '2.jpg'])
    (src / 'notes.txt').write_text('not a frame')
    assert pl.install_frames(work, str(src), 'cat') == 3
    out = os.path.join(work, 'database/DAVIS/JPEGImages/Full-Resolution/cat')
    assert sorted(os.listdir(out)) == ['00000.jpg', '00001.jpg', '00002.jpg']
    for i, n in enumerate(['1.png', '2.jpg', '10.png']):
        want = io.BytesIO()
        Image.open(os.path.join(str(src), n)).convert('RGB').save(want, format='JPEG', quality=95)
        assert open(os.path.join(out, '%05d.jpg' % i), 'rb').read() == want.getvalue(), n
    assert not np.array_equal(imgs['10.png'], imgs['2.jpg'])                  # (the frames differ, so the order shows in the bytes)
    args = pl.parse_args(['--frames', str(src), '--seqname', 'cat', '--workdir', work])
    pl.probe(args)
    assert (args.n_frames, args.width, args.height) == (3, 40, 24)


def test_install_refusals(tmp_path):
    work = str(tmp_path / 'work')
    os.makedirs(str(tmp_path / 'empty'))
    with pytest.raises(pl.PipelineError, match='no frames'):
        pl.install_frames(work, str(tmp_path / 'empty'), 'cat')
    write_images(tmp_path / 'two', ['0.png', '1.png'])
    with pytest.raises(pl.PipelineError, match='at least 3'):
        pl.install_frames(work, str(tmp_path / 'two'), 'cat')
    write_images(tmp_path / 'sizes', ['0.png', '1.png'])
    write_images(tmp_path / 'sizes', ['2.png'], size=(41, 24))
    with pytest.raises(pl.PipelineError, match='40 x 24'):
        pl.install_frames(work, str(tmp_path / 'sizes'), 'cat')
    assert not os.path.exists(work)                                            # refused before anything was written


def test_given_masks_are_installed_in_the_loaders_encoding(tmp_path):
    from PIL import Image
    work = str(tmp_path / 'work')
    write_images(tmp_path / 'in', ['0.png', '1.png', '2.png'])
    pl.install_frames(work, str(tmp_path / 'in'), 'cat')
    os.makedirs(str(tmp_path / 'sil'))
    m = np.zeros((24, 40), bool)
    m[5:12, 8:30] = True
    Image.fromarray(m.astype(np.uint8) * 255).save(str(tmp_path / 'sil' / 'a1.png'))                 # 0 / 255
    Image.fromarray(m.astype(np.uint8)).save(str(tmp_path / 'sil' / 'a2.png'))                       # 0 / 1
    enc = np.zeros((24, 40, 3), np.uint8)
    enc[..., 0] = m * 128
    Image.fromarray(enc).save(str(tmp_path / 'sil' / 'a10.png'))                                     # the loader's own
    pl.install_masks(work, str(tmp_path / 'sil'), 'cat')
    out = os.path.join(work, 'database/DAVIS/Annotations/Full-Resolution/cat')
    assert sorted(os.listdir(out)) == ['00000.png', '00001.png', '00002.png']
    for n in os.listdir(out):
        assert np.array_equal(np.asarray(Image.open(os.path.join(out, n))), enc)
    os.remove(str(tmp_path / 'sil' / 'a2.png'))
    with pytest.raises(pl.PipelineError, match='2 images'):
        pl.install_masks(work, str(tmp_path / 'sil'), 'cat')


def test_configs_read_back_for_both_names(tmp_path, monkeypatch):
    from lasr_amd import recon_io
    from lasr_amd.dataloader import vid
    work = str(tmp_path / 'work')
    write_images(tmp_path / 'in', ['%d.png' % i for i in range(7)])
    pl.install_frames(work, str(tmp_path / 'in'), 'cat')
    pl.copy_tree(work, 'database/DAVIS/JPEGImages/Full-Resolution/cat', 'database/DAVIS/JPEGImages/Full-Resolution/rcat')
    args = make_args(tmp_path, '--dframe', '2', '--init_frame', '1', '--end_frame', '6', '--can_frame', '3')
    config = by_name(pl.plan(args))['config']
    assert config.argv is None and config.outputs == ('configs/cat.config', 'configs/rcat.config')
    for act in config.pre:
        pl.ACTIONS[act[0]](work, *act[1:])
    monkeypatch.chdir(work)
    for name in ('cat', 'rcat'):
        cfg = vid.read_config(name, work)
        assert cfg == dict(datapath='database/DAVIS/JPEGImages/Full-Resolution/%s/' % name, dframe=2, init_frame=1, end_frame=6, can_frame=3)
        assert [os.path.basename(p) for p in recon_io.frame_list(name)] == ['00001.jpg', '00003.jpg', '00005.jpg']
    defaults = by_name(pl.plan(make_args(tmp_path)))['config'].pre
    assert defaults == (('write_configs', 'cat', 1, 0, -1, 0),)


# ---- the runner ----------------------------------------------------------------------------------------------------------------
FAKE = "import sys; open(sys.argv[1], 'a').write(sys.argv[2] + '\\n'); open(sys.argv[3], 'w').write(sys.argv[2]); print('ran', sys.argv[2:])"


def fake_plan(work, names, flags=None, code=None, limits=None):
    """A chain of fake children: each appends its name to started.txt and writes out/<name>, which the next one declares as input."""
    steps, prev = [], ()
    for n in names:
        argv = (PY, '-c', (code or {}).get(n, FAKE), 'started.txt', n, 'out/' + n) + tuple((flags or {}).get(n, ()))
        steps.append(pl.Step(n, 'local', argv, work, prev, ('out/' + n,), (limits or {}).get(n, 60), (), ()))
        prev = ('out/' + n,)
    return steps


def started(work):
    path = os.path.join(work, 'started.txt')
    return open(path).read().split() if os.path.exists(path) else []


@pytest.fixture
def work(tmp_path):
    os.makedirs(str(tmp_path / 'work' / 'out'))
    return str(tmp_path / 'work')


def test_runner_stamps_resumes_and_reruns_from_the_first_change(work):
    names = ['install', 'masks', 'stage-0', 'stage-1', 'stage-2', 'extract']
    out = io.StringIO()
    assert pl.run(fake_plan(work, names), work, out=out, meta=dict(seqname='cat')) == 0
    assert started(work) == names
    sdir = os.path.join(work, 'reconstruct', 'steps')
    assert sorted(os.listdir(sdir)) == sorted('%02d-%s.%s' % (i, n, e) for i, n in enumerate(names) for e in ('json', 'log'))
    stamp = json.load(open(os.path.join(sdir, '03-stage-1.json')))
    assert stamp['argv'][4] == 'stage-1' and stamp['returncode'] == 0 and stamp['seconds'] >= 0 and re.fullmatch('[0-9a-f]{64}', stamp['hash'])
    assert stamp['outputs'] == [['out/stage-1', len('stage-1')]]
    assert "ran ['stage-1'" in open(os.path.join(sdir, '03-stage-1.log')).read()
    assert json.load(open(os.path.join(work, 'reconstruct', 'run.json'))) == dict(seqname='cat')
    assert pl.run(fake_plan(work, names), work, out=io.StringIO()) == 0 and started(work) == names              # nothing started
    assert pl.run(fake_plan(work, names, flags={'stage-1': ('--n_bones', '31')}), work, out=io.StringIO()) == 0
    assert started(work) == names + ['stage-1', 'stage-2', 'extract']                                           # and nothing before it
    os.remove(os.path.join(work, 'out', 'stage-2'))                                                             # a declared output is gone
    assert pl.run(fake_plan(work, names, flags={'stage-1': ('--n_bones', '31')}), work, out=io.StringIO()) == 0
    assert started(work)[-2:] == ['stage-2', 'extract'] and len(started(work)) == len(names) + 5


def test_runner_force_from_and_until(work):
    names = ['install', 'masks', 'scores-reproj', 'scores-shape', 'glb']
    plan = fake_plan(work, names)
    assert pl.run(plan, work, until='masks', out=io.StringIO()) == 0 and started(work) == ['install', 'masks']
    assert pl.run(plan, work, until='scores', out=io.StringIO()) == 0 and started(work) == names[:4]          # a group: up to its last step
    assert pl.run(plan, work, out=io.StringIO()) == 0 and started(work) == names
    assert pl.run(plan, work, force=['masks'], until='masks', out=io.StringIO()) == 0 and started(work) == names + ['masks']
    assert pl.run(plan, work, start='scores', force=['scores-shape'], out=io.StringIO()) == 0
    assert started(work) == names + ['masks', 'scores-shape', 'glb']
    with pytest.raises(pl.PipelineError, match='no step'):
        pl.run(plan, work, start='nowhere', out=io.StringIO())


def test_a_child_that_aborts_stops_the_run(work):
    names = ['install', 'masks', 'flow', 'stage-0']
    abort = "import sys; open(sys.argv[1], 'a').write(sys.argv[2] + '\\n'); print('about to fail'); sys.stdout.flush(); sys.exit(134)"
    out = io.StringIO()
    assert pl.run(fake_plan(work, names, code={'masks': abort}), work, out=out) == pl.EXIT_FAILED == 2
    assert started(work) == ['install', 'masks']
    sdir = os.path.join(work, 'reconstruct', 'steps')
    assert sorted(os.listdir(sdir)) == ['00-install.json', '00-install.log', '01-masks.log']                    # no stamp for it, nothing later
    text = out.getvalue()
    assert 'masks' in text and '134' in text and 'about to fail' in text and 'Nothing further is started' in text
    assert pl.run(fake_plan(work, names), work, out=io.StringIO()) == 0 and started(work) == ['install', 'masks'] + names[1:]


def test_a_child_killed_by_a_signal_stops_the_run(work):
    kill = "import os, signal; os.kill(os.getpid(), signal.SIGSEGV)"
    out = io.StringIO()
    assert pl.run(fake_plan(work, ['install', 'masks'], code={'install': kill}), work, out=out) == 2
    assert started(work) == [] and '-11' in out.getvalue()


def process_gone(pid):
    try:
        with open('/proc/%d/stat' % pid) as fh:
            return fh.read().rsplit(')', 1)[1].split()[0] in 'ZX'
    except OSError:
        return True


def test_a_child_past_its_limit_is_ended_with_its_whole_group(work):
    slow = ("import subprocess, sys, time; open(sys.argv[1], 'a').write(sys.argv[2] + '\\n');"
            "p = subprocess.Popen([sys.executable, '-c', 'import time; time.sleep(600)']);"
            "open('grandchild.pid', 'w').write(str(p.pid)); print('sleeping'); sys.stdout.flush(); time.sleep(600)")
    names = ['install', 'masks', 'flow']
    out = io.StringIO()
    assert pl.run(fake_plan(work, names, code={'masks': slow}, limits={'masks': 1}), work, out=out) == pl.EXIT_TIMED_OUT == 3
    assert started(work) == ['install', 'masks']
    assert process_gone(int(open(os.path.join(work, 'grandchild.pid')).read()))
    assert 'masks' in out.getvalue() and 'timed out after 1 s' in out.getvalue() and 'sleeping' in out.getvalue()
    assert not os.path.exists(os.path.join(work, 'reconstruct', 'steps', '01-masks.json'))
    assert not os.path.exists(os.path.join(work, 'reconstruct', 'steps', '02-flow.log'))


def test_a_terminated_driver_takes_its_child_along_and_the_next_run_resumes_there(work):
    import signal
    import subprocess
    import time
    slow = ("import sys, time; open(sys.argv[1], 'a').write(sys.argv[2] + '\\n'); open('child.pid', 'w').write(str(__import__('os').getpid()));"
            "time.sleep(600)")
    driver = ("import signal, sys; sys.path[:0] = [%r, %r]; import test_reconstruct_cpu as t; script = t.load('scripts', 'reconstruct.py');"
              "signal.signal(signal.SIGTERM, script._stop);"
              "sys.exit(t.pl.run(t.fake_plan(%r, ['stage-0', 'stage-1', 'stage-2', 'extract'], code={'stage-2': %r}), %r))"
              % (ROOT, os.path.join(ROOT, 'tests'), work, slow, work))
    p = subprocess.Popen([PY, '-c', driver], stdout=subprocess.DEVNULL, stderr=subprocess.STDOUT)
    deadline = time.monotonic() + 60
    while not os.path.exists(os.path.join(work, 'child.pid')) and p.poll() is None and time.monotonic() < deadline:
        time.sleep(0.02)
    assert p.poll() is None and started(work) == ['stage-0', 'stage-1', 'stage-2']
    p.send_signal(signal.SIGTERM)
    assert p.wait(30) == 128 + signal.SIGTERM
    assert process_gone(int(open(os.path.join(work, 'child.pid')).read()))
    names = ['stage-0', 'stage-1', 'stage-2', 'extract']
    assert pl.run(fake_plan(work, names), work, out=io.StringIO()) == 0
    assert started(work) == ['stage-0', 'stage-1', 'stage-2', 'stage-2', 'extract']


def test_a_step_that_does_not_write_its_output_fails(work):
    quiet = "import sys; open(sys.argv[1], 'a').write(sys.argv[2] + '\\n')"
    out = io.StringIO()
    assert pl.run(fake_plan(work, ['install', 'masks'], code={'install': quiet}), work, out=out) == 2
    assert started(work) == ['install'] and 'without writing out/install' in out.getvalue()


def test_the_child_inherits_the_environment_untouched(work, monkeypatch):
    monkeypatch.setenv('RECONSTRUCT_TEST_MARK', 'kept')
    env = "import json, os, sys; json.dump(dict(os.environ), open(sys.argv[3], 'w'))"
    mine = dict(os.environ)
    assert pl.run(fake_plan(work, ['install'], code={'install': env}), work, out=io.StringIO()) == 0
    child = json.load(open(os.path.join(work, 'out', 'install')))
    # every variable of this process arrives unchanged (LC_CTYPE: the child interpreter's own locale coercion; the child may see
    # more than os.environ shows: what native libraries of this process have put into the C environment)
    diff = {k for k in mine if child.get(k) != mine[k]}
    assert diff <= {'LC_CTYPE'}, diff
    assert child['RECONSTRUCT_TEST_MARK'] == 'kept'


# ---- the command ---------------------------------------------------------------------------------------------------------------
def test_dry_run_prints_shell_lines_and_writes_nothing(tmp_path):
    write_images(tmp_path / 'in', ['0.png', '1.png', '2.png'])
    out = io.StringIO()
    workdir = tmp_path / 'work'
    argv = ['--frames', str(tmp_path / 'in'), '--seqname', 'cat', '--workdir', str(workdir), '--glb', '--dry_run', '--', '--min_area', '100']
    assert pl.main(argv, out=out) == 0 and not workdir.exists()
    lines = out.getvalue().splitlines()
    args = make_args(tmp_path, '--glb', '--', '--min_area', '100', frames=3, size=(40, 24))
    steps = pl.plan(args)
    assert len(lines) == len(steps) == 11
    for line, step in zip(lines, steps):
        assert line.startswith('timeout -k 10 ') and (line.endswith(' &&') != (step is steps[-1]))
        assert 'timeout -k 10 %d %s ' % (step.timeout_s, PY) in line
        if step.argv:
            assert ' '.join(step.argv[1:3]) in line
        else:
            assert 'scripts/reconstruct.py' in line and '--from %s --until %s' % (step.name, step.name) in line and '--dry_run' not in line
            assert line.index('--from') < line.index(' -- ')
    flow_r = lines[2]
    assert flow_r.startswith('timeout -k 10 %d rm -rf ./rcat && timeout' % pl.LOCAL_S)
    assert flow_r.count('cp -rf rcat/') == 4 and lines[3].count('cp -rf cat/') == 2


def test_the_script_is_argument_parsing_then_the_module(tmp_path):
    script = load('scripts', 'reconstruct.py')
    assert script.pipeline is pl
    write_images(tmp_path / 'in', ['0.png', '1.png'])
    out = io.StringIO()
    rc = pl.main(['--frames', str(tmp_path / 'in'), '--seqname', 'cat', '--workdir', str(tmp_path / 'w'), '--until', 'install'], out=out)
    assert rc == 2 and 'install' in out.getvalue() and 'at least 3' in out.getvalue()


def test_report_on_canned_scores(tmp_path):
    work = str(tmp_path / 'work')
    args = make_args(tmp_path, '--tracks', '--worst', '2', frames=4)
    odir = os.path.join(work, 'reconstruct')
    names = ['stage-0', 'stage-1', 'extract']
    os.makedirs(os.path.join(work, 'out'))
    assert pl.run(fake_plan(work, names), work, out=io.StringIO(), meta=pl.describe(args)) == 0
    json.dump(dict(frame_ids=[0, 1, 2, 3], means=dict(J=0.8, F=0.7, JF=0.75, epe=1.5, psnr=None),
                   per_frame=dict(JF=[0.9, 0.5, None, 0.6])), open(os.path.join(odir, 'reproj.json'), 'w'))
    json.dump(dict(frame_ids=[0, 1, 2, 3], means=dict(n_pairs=2.5, ratio=0.01, volume=1.0, area=6.0, jitter=1e-3),
                   per_frame=dict(ratio=[0., 0.03, 0.01, 0.])), open(os.path.join(odir, 'shape.json'), 'w'))
    ann = os.path.join(work, 'database/DAVIS/Annotations/Full-Resolution/cat')
    os.makedirs(ann)
    json.dump(dict(keys=[2], roundtrip_iou=None, motion=dict(scores=[0.5, 1.5, 3.0, 1.0], keys=[2])), open(os.path.join(ann, 'maskprop.json'), 'w'))
    write_images(os.path.join(work, 'database/DAVIS/JPEGImages/Full-Resolution/cat'), ['%05d.jpg' % i for i in range(4)])
    write_images(os.path.join(work, 'database/DAVIS/JPEGImages/Full-Resolution/rcat'), ['%05d.jpg' % i for i in range(3)])
    mon = os.path.join(work, 'log', 'cat-1', 'monitor')
    os.makedirs(mon)
    open(os.path.join(mon, 'scalars.csv'), 'w').write('step,total_loss,mask_loss\n1,0.9,0.5\n2,0.25,0.125\n')
    open(os.path.join(odir, 'tracks.npz'), 'w').write('x')
    doc = pl.report(work)
    assert doc == json.load(open(os.path.join(odir, 'report.json')))
    assert doc['sequence'] == dict(name='cat', frames=4, size=[80, 64], frames_kept_in_r=3)
    assert doc['masks'] == dict(route='auto_mask', keys=[2], motion_scores=[0.5, 1.5, 3.0, 1.0])
    assert doc['scores']['reproj']['means']['JF'] == 0.75 and doc['scores']['shape']['means']['ratio'] == 0.01
    assert doc['scores']['reproj']['worst'] == [dict(frame=1, value=0.5), dict(frame=3, value=0.6)]
    assert doc['scores']['shape']['worst'] == [dict(frame=1, value=0.03), dict(frame=2, value=0.01)]
    assert [s['name'] for s in doc['stages']] == ['stage-0', 'stage-1'] and all(s['seconds'] >= 0 for s in doc['stages'])
    assert doc['stages'][0]['flags']['n_hypo'] == 8 and doc['stages'][0]['total_loss'] is None and doc['stages'][1]['total_loss'] == 0.25
    assert doc['exports'] == ['reconstruct/tracks.npz']
    used = ['auto_mask', 'variational', 'ssim', 'encoder_random', 'one_gpu', 'eval_reproj', 'eval_shape', 'export_tracks']
    assert doc['caveats'] == [pl.CAVEATS[k] for k in used]
    assert sum('unverified' in c for c in doc['caveats']) >= 4 and 'half' in pl.CAVEATS['one_gpu']
    md = open(os.path.join(odir, 'report.md')).read()
    assert all(c in md for c in doc['caveats']) and 'frame 1 (0.5)' in md and 'JF 0.75' in md and 'reconstruct/tracks.npz' in md
    full = pl.describe(make_args(tmp_path, '--masks', 'sil', '--loadmodel', 'v.pth', '--alexnet_weights', 'a.pth', '--encoder_weights', 'e.pth'))
    assert full['pieces'] == ['one_gpu', 'eval_reproj', 'eval_shape']


def test_the_module_stays_light_and_outside_the_native_scan():
    text = open(os.path.join(ROOT, 'lasr_amd', 'pipeline.py')).read()
    assert not re.search(r'\bcall\(', text)                  # tests/test_guarded_alloc_cpu.py reads any such site as a native launch
    assert not re.search(r'^\s*(import|from)\s+torch', text, re.M) and '_lib' not in text
    code = 'import sys; import lasr_amd.pipeline; assert "torch" not in sys.modules and "lasr_amd._lib" not in sys.modules'
    import subprocess
    assert subprocess.run([PY, '-c', code], cwd=ROOT).returncode == 0
