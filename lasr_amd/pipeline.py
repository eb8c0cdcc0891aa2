"""From a folder of frames to a report: the plan, the runner and the report of scripts/reconstruct.py.

plan(args) lists the steps as data: frames installed in the DAVIS layout, silhouettes (given, propagated from painted keys, or from
motion alone), the two flow passes of preprocess/auto_gen.sh, the two configs, one optimize.py run per stage of a schedule, extract.py,
the two scores without ground truth and the optional exports.  run(steps, workdir) executes them one child process at a time, each in
its own process group and under its own time limit, stops at the first failure, never retries, and stamps what succeeded so that a
later run resumes.  report(workdir) gathers what the steps left into reconstruct/report.json and report.md.

Host only and light: no torch, no native library, nothing here touches the GPU; every GPU program is a child.  The scripts the
steps run are the ones a user would type by hand, with the flags a user would give them: the driver adds nothing to what they compute.
"""
import argparse
import collections
import hashlib
import json
import math
import os
import re
import shlex
import shutil
import signal
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DAVIS, RES = 'database/DAVIS', 'Full-Resolution'
OUT = 'reconstruct'                                    # the driver's own folder under the work directory
KILL_AFTER_S = 10                                      # SIGTERM at the limit, SIGKILL this much later (`timeout -k 10`)
TAIL_LINES = 40
EXIT_FAILED, EXIT_TIMED_OUT = 2, 3


class PipelineError(Exception):
    """A refusal of the driver itself (bad input, bad arguments); the text goes to the user as is."""


Step = collections.namedtuple('Step', 'name kind argv cwd inputs outputs timeout_s pre post')
Step.__doc__ = """name: unique; kind: the row of MEASURED its limit comes from; argv: the child's full command line (None: the step
runs in process); cwd: the work directory; inputs / outputs: paths relative to the work directory (a folder stands for its files);
timeout_s: the child's limit; pre / post: in-process actions (name, arguments...) of ACTIONS before / after the child."""

# ---- time limits ---------------------------------------------------------------------------------------------------------------
# limit = (start_up + work / rate) * MARGIN.  start_up [s] and rate [work / s] per kind were measured once, on one MI355X, with the
# existing scripts run by hand one after another as fresh processes (not through this driver); DESIGN.md section 4.20 has the table
# with the runs behind each row.  work: ordered frame pairs x pixels for masks and flow, iterations of the measured configuration for
# a stage (stage_work), frames for the rest.  MARGIN is 4: machines of one pool differ by a few percent, and the first call into
# MIOpen on a fresh machine has been seen to take 58 s (section 4.16).
MEASURED_ON = '2026-10-20'
MARGIN = 4
MEASURED = {                                           # kind: (start_up seconds, rate in work units per second)
    'masks': (2.6, 1.18e7),                            # auto_mask.py, variational flow: 8 frames of 64 x 80 in 2.6 s, of 640 x 800 in 3.2 s
    'flow': (2.1, 1.77e7),                             # auto_gen.py --flow_threshold 0, variational flow: the same frames in 2.1 s and 2.5 s
    'stage': (74.4, 216.),                             # spot3 stage 0 (ssim, graph): 200 iterations in 7.3 s, 1000 in 11.0 s; the first stage
                                                       # of a fresh machine (MIOpen's first calls) 75.3 s for the 200
    'extract': (74.4, 12.9),                           # 4 frames in 5.2 s, 40 in 8.0 s after a stage had run; it builds the same trainer and runs
                                                       # its forward, so its first-call set-up is bounded by the stage's, which was measured cold
    'eval_reproj': (2.4, 180.),                        # 4 / 40 frames of 512 x 512, 1600 faces: 2.4 / 2.6 s.  Where the two differ by no more than
    'eval_shape': (2.2, 180.),                         # the 0.2 s that repeated runs of one command differ by (2.2 / 2.4, 2.3 / 2.5, 2.0 / 2.0,
    'render_vis': (2.2, 40.),                          # 2.2 / 2.3 s), the rate is the lower bound 36 frames / 0.2 s; render_vis.py: 2.3 / 3.2 s
    'bake_texture': (2.3, 180.),
    'export_gltf': (2.0, 180.),
    'export_tracks': (2.2, 180.),
}
EPOCH_ITERS = 200                                      # the loader pads an epoch of a sequence on disk to about 200 iterations (vid.py)
STAGE_BASE = dict(n_hypo=8, n_faces=1280, batch_size=1)   # the configuration the stage rate was measured at: scripts/spot3.sh stage 0
LOCAL_S = 600                                          # in-process file copies: no child, no GPU; the number only fills the plan's column


def stage_work(flags):
    """Iterations of a stage in units of the measured configuration's: an iteration is never counted as cheaper than the measured
    one, and as dearer in proportion to the batch, the camera hypotheses and the faces beyond it (each render is per image and
    hypothesis and walks every face)."""
    f = lambda k, d: float(flags.get(k, d))            # noqa: E731
    return (f('num_epochs', 1000) * EPOCH_ITERS * max(f('batch_size', 8) / STAGE_BASE['batch_size'], 1.)
            * max(f('n_hypo', 1) / STAGE_BASE['n_hypo'], 1.) * max(f('n_faces', 1280) / STAGE_BASE['n_faces'], 1.))


def limit_s(kind, work, scale=1.):
    if kind == 'local':
        return LOCAL_S
    start_up, rate = MEASURED[kind]
    return int(math.ceil((start_up + work / rate) * MARGIN * scale))


# ---- caveats: what is unverified about each piece, quoted in the report for the pieces a run used -----------------------------------
CAVEATS = collections.OrderedDict([
    ('auto_mask', 'Silhouettes from motion alone (preprocess/auto_mask.py): quality on real footage is unverified.  Meant for one '
                  'object below half the frame that moves against a far, planar or rotating-camera background.'),
    ('propagate_mask', 'Silhouettes propagated from painted key frames (preprocess/propagate_mask.py): quality on real footage is '
                       'unverified; --roundtrip is the available check.'),
    ('variational', 'Optical flow without a checkpoint (--flow_method variational): quality on real footage is unverified; large '
                    'displacements and textureless regions are its known limits.'),
    ('gradient_constancy', 'Gradient-constancy term of the variational flow (-- --vf_gamma, preprocess/robust_flow.py): its weight '
                           'is derived on relit closed-form fixtures, not on footage, and quality on real footage is unverified.  '
                           'One flow takes 1.11 (640 x 800) to 1.13 (1080p) times as long with it as without, so the default '
                           'limits of the masks and flow steps, which carry a factor of 4, hold.'),
    ('large_displacement', 'Large-displacement matching stage of the variational flow (-- --vf_match, preprocess/flow_match.py): '
                           'its patch radius, acceptance ratio and propagation count are derived on closed-form fixtures, not on '
                           'footage: unverified on real footage.  A thin limb is only partly recovered.'),
    ('vcn_dry', 'No VCN checkpoint was given and the network was chosen: its weights are random, the flows are a dry run.'),
    ('ssim', 'Texture term --ptex_method ssim (no AlexNet weights): its weight is derived, not measured, and quality on real '
             'footage is unverified.'),
    ('alexnet_random', 'Texture term alexnet without --alexnet_weights: the features are a random projection.'),
    ('fold_penalty', 'Fold penalty on the posed meshes (--fold_wt, --pierce_wt; scripts/fold_penalty.py): its weights and its angle '
                     'of 30 degrees are derived from nothing measured on a real reconstruction: unmeasured, and its effect on real '
                     'footage is unverified.'),
    ('isect_penalty', 'Intersection penalty on the posed meshes (--isect_wt; scripts/isect_penalty.py): its weight is derived from '
                      'nothing measured: unmeasured, and its effect on real footage is unverified; it clears shallow pass-throughs and '
                      'does not separate two bodies that overlap wholesale.'),
    ('encoder_random', 'The ResNet-18 encoder starts from random weights (no --encoder_weights); the reference starts from '
                       'ImageNet weights.'),
    ('one_gpu', 'Stages run on one GPU (--ngpu 1).  The reference\'s scripts/template.sh runs two processes with its batch size '
                'each, so with the template schedule the effective batch is half the reference\'s.'),
    ('eval_reproj', 'scripts/eval_reproj.py scores against the silhouettes and flows the reconstruction was fitted to: agreement, '
                    'not ground truth.'),
    ('eval_shape', 'scripts/eval_shape.py does not see folds between neighbouring faces.'),
    ('eval_shape_neighbours', 'scripts/eval_shape.py --neighbours also tests faces that share a vertex or an edge.  Two faces that '
                              'share an edge count as folded (n_creased) below an interior dihedral angle of 20 degrees: an angle '
                              'criterion, not an intersection test, and the threshold is derived from nothing measured on a real '
                              'reconstruction: unverified on real footage.  Judge by min_dihedral.'),
    ('bake_texture', 'The baked atlas (scripts/bake_texture.py) is only as good as the fitted cameras; unseen texels stay unfilled '
                     'without --fill.'),
    ('export_tracks', 'Point tracks (scripts/export_tracks.py) follow the fitted surface, not the image: unverified on real footage.'),
])

# ---- the flags handed through to the preprocessing scripts (after `--`) ----------------------------------------------------------
# name -> the scripts that own it; tests/test_reconstruct_cpu.py holds every entry against the scripts' own parsers
FLOW_OWNERS = ('auto_gen', 'auto_mask', 'propagate_mask')
MASK_OWNERS = ('auto_mask', 'propagate_mask')
PASS_FLAGS = {name: FLOW_OWNERS for name in ('testres', 'maxdisp', 'fac')}
PASS_FLAGS.update({name: MASK_OWNERS for name in ('hi', 'lo', 'tau', 'w_p', 'w_a', 'eps', 'U', 'R', 'sigma_i', 'sigma_s', 'w_s', 'K',
                                                   'min_component', 'min_area', 'roundtrip')})
PASS_FLAGS.update({'n_keys': ('auto_mask',), 'keydir': ('auto_mask',)})
PASS_PREFIXES = {'vf_': FLOW_OWNERS, 'ms_': ('auto_mask',)}


def route_passthrough(tokens):
    """The tokens after `--` -> {script: its tokens, verbatim and in order}.  A flag is `--name` followed by its values (the tokens
    up to the next `--...`); a flag no script owns is refused."""
    out = {name: [] for name in FLOW_OWNERS}
    i = 0
    while i < len(tokens):
        tok = tokens[i]
        if not tok.startswith('--') or len(tok) < 3:
            raise PipelineError('after `--`: expected a flag, got %r' % tok)
        j = i + 1
        while j < len(tokens) and not tokens[j].startswith('--'):
            j += 1
        name = tok[2:].split('=', 1)[0]
        owners = PASS_FLAGS.get(name)
        if owners is None:
            owners = next((o for pre, o in PASS_PREFIXES.items() if name.startswith(pre)), None)
        if owners is None:
            raise PipelineError('after `--`: no preprocessing script takes --%s' % name)
        for o in owners:
            out[o] += tokens[i:j]
        i = j
    return out


# ---- arguments -----------------------------------------------------------------------------------------------------------------
SCHEDULE_DIR = os.path.join(ROOT, 'scripts', 'schedules')
DRIVER_STAGE_DEFAULTS = (('use_graph', True), ('sil_path', 'none'), ('opt_tex', 'yes'))     # + ptex_method ssim without AlexNet weights


def parse_key(text):
    idx, sep, path = text.partition(':')
    if not sep or not path or not idx.isdigit():
        raise argparse.ArgumentTypeError('--key takes FRAME:PNG, e.g. 0:first.png (got %r)' % text)
    return int(idx), path


def load_schedule(spec):
    """quick | template | FILE -> (name, stages): a list of dicts of optimize.py flag -> value plus dataname and timeout_s."""
    path = os.path.join(SCHEDULE_DIR, spec + '.json') if re.fullmatch(r'\w+', spec) else spec
    try:
        with open(path) as fh:
            stages = json.load(fh)
    except (OSError, ValueError) as e:
        raise PipelineError('--schedule %s: %s' % (spec, e))
    if not isinstance(stages, list) or not stages or not all(isinstance(s, dict) for s in stages):
        raise PipelineError('--schedule %s: a schedule is a non-empty list of stages, each a dict of optimize.py flags' % spec)
    for s in stages:
        if s.get('dataname', '{seq}') not in ('{seq}', 'r{seq}'):
            raise PipelineError('--schedule %s: dataname is "{seq}" or "r{seq}", not %r' % (spec, s['dataname']))
    return os.path.splitext(os.path.basename(path))[0], stages


def build_parser():
    p = argparse.ArgumentParser(description='from a folder of frames to a reconstruction and a report, one resumable command',
                                allow_abbrev=False)
    p.add_argument('--frames', default=None, help='folder of the video\'s frames (any format PIL opens; natural order of the names)')
    p.add_argument('--seqname', required=True, help='name of the sequence: a word')
    p.add_argument('--workdir', required=True, help='work directory: database/, configs/, log/ and reconstruct/ are written under it')
    p.add_argument('--masks', default=None, help='folder of silhouettes, one image per frame (non-zero = object)')
    p.add_argument('--key', action='append', type=parse_key, default=[], metavar='FRAME:PNG',
                   help='a painted frame for preprocess/propagate_mask.py; repeatable.  Without --masks and --key: preprocess/auto_mask.py')
    p.add_argument('--loadmodel', default=None, help='VCN checkpoint; without it the flow is --flow_method variational')
    p.add_argument('--flow_method', default=None, choices=('vcn', 'variational'))
    p.add_argument('--alexnet_weights', default='', help='optimize.py --alexnet_weights; without it --ptex_method ssim')
    p.add_argument('--encoder_weights', default='', help='optimize.py --encoder_weights')
    p.add_argument('--schedule', default='quick', help='quick, template or a JSON file (default quick)')
    for name, default in (('dframe', 1), ('init_frame', 0), ('end_frame', -1), ('can_frame', 0)):
        p.add_argument('--' + name, type=int, default=default, help='configs/<seq>.config: %s (default %d)' % (name, default))
    for name, text in (('gif', 'render_vis.py'), ('glb', 'scripts/export_gltf.py'), ('atlas', 'scripts/bake_texture.py'),
                       ('tracks', 'scripts/export_tracks.py')):
        p.add_argument('--' + name, action='store_true', help='also run ' + text)
    p.add_argument('--neighbours', action='store_true',
                   help='scripts/eval_shape.py --neighbours: also score folds between neighbouring faces (n_pierced, n_creased, min_dihedral)')
    p.add_argument('--fold_wt', type=float, default=0., help='optimize.py --fold_wt for every stage: the weight of the crease term of the '
                   'fold penalty on the posed meshes (default 0: off)')
    p.add_argument('--pierce_wt', type=float, default=0., help='optimize.py --pierce_wt for every stage: the weight of its pierce term '
                   '(default 0: off)')
    p.add_argument('--isect_wt', type=float, default=0., help='optimize.py --isect_wt for every stage: the weight of the intersection '
                   'penalty between faces of the posed meshes that share no vertex (default 0: off)')
    p.add_argument('--worst', type=int, default=5, help='frames listed as worst by each score (default 5)')
    p.add_argument('--dry_run', action='store_true', help='print the plan as shell lines; run nothing, write nothing')
    p.add_argument('--from', dest='start', default=None, metavar='STEP', help='first step to run')
    p.add_argument('--until', default=None, metavar='STEP', help='last step to run')
    p.add_argument('--force', action='append', default=[], metavar='STEP', help='run this step even if its stamp matches; repeatable')
    p.add_argument('--timeout_scale', type=float, default=1., help='multiplies every computed time limit (default 1.0)')
    return p


def parse_args(argv, cwd=None):
    """The command line of scripts/reconstruct.py -> a namespace plan() takes.  Paths of the user become absolute here (cwd: what
    they are relative to), the schedule file is read here: plan() itself opens nothing.  n_frames / width / height stay None until
    probe() or the caller sets them."""
    argv = list(argv)
    extra = []
    if '--' in argv:
        at = argv.index('--')
        argv, extra = argv[:at], argv[at + 1:]
    p = build_parser()
    args = p.parse_args(argv)
    cwd = cwd or os.getcwd()
    absolute = lambda x: os.path.normpath(os.path.join(cwd, os.path.expanduser(x)))    # noqa: E731
    if not re.fullmatch(r'[A-Za-z0-9][A-Za-z0-9_.-]*', args.seqname) or 'JPEGImages' in args.seqname:
        p.error('--seqname %r: a word of letters, digits, _ . -' % args.seqname)
    if args.masks and args.key:
        p.error('--masks and --key exclude each other: the silhouettes are given or they are propagated')
    if args.timeout_scale <= 0:
        p.error('--timeout_scale must be positive')
    for name in ('fold_wt', 'pierce_wt', 'isect_wt'):
        if not (math.isfinite(getattr(args, name)) and getattr(args, name) >= 0.):
            p.error('--%s must be finite and at least 0' % name)
    if args.flow_method is None:
        args.flow_method = 'vcn' if args.loadmodel else 'variational'
    if args.flow_method == 'variational' and args.loadmodel:
        p.error('--flow_method variational uses no network: drop --loadmodel')
    args.workdir = absolute(args.workdir)
    for name in ('frames', 'masks', 'loadmodel', 'alexnet_weights', 'encoder_weights'):
        if getattr(args, name):
            setattr(args, name, absolute(getattr(args, name)))
    args.key = [(k, absolute(path)) for k, path in args.key]
    try:
        args.passthrough = route_passthrough(extra)
        if not re.fullmatch(r'\w+', args.schedule):
            args.schedule = absolute(args.schedule)
        args.schedule_name, args.stages = load_schedule(args.schedule)
    except PipelineError as e:
        p.error(str(e))
    args.extra = extra
    args.n_frames = args.width = args.height = None
    return args


def natural_key(name):
    return [int(t) if t.isdigit() else t.lower() for t in re.split(r'(\d+)', name)]


def list_images(folder):
    """The files of a folder that carry an extension PIL has a reader for, in natural order of their names."""
    from PIL import Image
    known = set(Image.registered_extensions())
    try:
        names = os.listdir(folder)
    except OSError as e:
        raise PipelineError('%s: %s' % (folder, e))
    return [os.path.join(folder, n) for n in sorted(names, key=natural_key) if os.path.splitext(n)[1].lower() in known]


def probe(args):
    """Fills args.n_frames, width, height: from --frames, else from the sequence already installed under the work directory.  The
    plan's time limits are computed from them."""
    from PIL import Image
    folder = args.frames or os.path.join(args.workdir, seq_dir('JPEGImages', args.seqname))
    paths = list_images(folder)
    if not paths:
        raise PipelineError('no frames under %s' % folder)
    with Image.open(paths[0]) as im:
        args.width, args.height = im.size
    args.n_frames = len(paths)
    return args


# ---- the plan ------------------------------------------------------------------------------------------------------------------
def seq_dir(kind, seq):
    return '%s/%s/%s/%s' % (DAVIS, kind, RES, seq)


def mask_route(args):
    return 'given' if args.masks else 'propagate_mask' if args.key else 'auto_mask'


def flag_tokens(flags):
    """dict of optimize.py flag -> value -> its tokens: true is --flag, false --noflag, anything else --flag value."""
    out = []
    for key, val in flags.items():
        if isinstance(val, bool):
            out.append('--%s%s' % ('' if val else 'no', key))
        else:
            out += ['--' + key, str(val)]
    return out


def stage_flags(args, stage):
    """The optimize.py flags of one stage of the schedule: the stage's own, then the driver's defaults where the stage is silent."""
    flags = collections.OrderedDict((k, v) for k, v in stage.items() if k != 'timeout_s')
    flags['dataname'] = stage.get('dataname', '{seq}').replace('{seq}', args.seqname)
    flags.setdefault('ngpu', 1)
    for key, val in DRIVER_STAGE_DEFAULTS:
        flags.setdefault(key, val)
    if args.alexnet_weights:
        flags.setdefault('alexnet_weights', args.alexnet_weights)
    else:
        flags.setdefault('ptex_method', 'ssim')
    if args.encoder_weights:
        flags.setdefault('encoder_weights', args.encoder_weights)
    for key in ('fold_wt', 'pierce_wt', 'isect_wt'):                               # named only when asked for: the default plan keeps its bytes
        if getattr(args, key, 0.):
            flags.setdefault(key, getattr(args, key))
    if int(flags['ngpu']) != 1:
        raise PipelineError('a stage with --ngpu %s: the driver runs every stage on one GPU' % flags['ngpu'])
    return flags


def data_inputs(seq):
    return ['configs/%s.config' % seq] + [seq_dir(kind, seq) for kind in ('JPEGImages', 'Annotations', 'FlowFW', 'FlowBW')]


def plan(args):
    """-> [Step].  Pure: the same arguments give the same steps; no file is opened, no clock read."""
    if args.n_frames is None or not args.width or not args.height:
        raise PipelineError('plan() needs the number and the size of the frames: probe(args) reads them')
    py, seq, rseq, cwd, scale = sys.executable, args.seqname, 'r' + args.seqname, args.workdir, args.timeout_scale
    T = args.n_frames
    pair_pixels = 2 * max(T - 1, 1) * args.width * args.height
    script = lambda *parts: os.path.join(ROOT, *parts)                         # noqa: E731
    datapath = seq_dir('JPEGImages', seq) + '/'
    steps = []

    def add(name, kind, argv=None, inputs=(), outputs=(), work=0., pre=(), post=(), timeout_s=None):
        steps.append(Step(name, kind, tuple(argv) if argv else None, cwd, tuple(inputs), tuple(outputs),
                          timeout_s if timeout_s is not None else limit_s(kind, work, scale), tuple(pre), tuple(post)))

    add('install', 'local', inputs=[args.frames] if args.frames else [], outputs=[seq_dir('JPEGImages', seq)],
        pre=[('install_frames', args.frames, seq)])

    flow = ['--flow_method', args.flow_method] + (['--loadmodel', args.loadmodel] if args.loadmodel else [])
    route = mask_route(args)
    ann = seq_dir('Annotations', seq)
    if route == 'given':
        add('masks', 'local', inputs=[args.masks, seq_dir('JPEGImages', seq)], outputs=[ann], pre=[('install_masks', args.masks, seq)])
    elif route == 'propagate_mask':
        keys = [t for k, path in args.key for t in ('--key', '%d:%s' % (k, path))]
        add('masks', 'masks', [py, script('preprocess', 'propagate_mask.py'), '--datapath', datapath] + keys + flow + ['--force'] +
            args.passthrough['propagate_mask'], inputs=[seq_dir('JPEGImages', seq)] + [path for _, path in args.key], outputs=[ann],
            work=pair_pixels)
    else:
        add('masks', 'masks', [py, script('preprocess', 'auto_mask.py'), '--datapath', datapath] + flow + ['--force'] +
            args.passthrough['auto_mask'], inputs=[seq_dir('JPEGImages', seq)], outputs=[ann], work=pair_pixels)

    gen = [py, script('preprocess', 'auto_gen.py'), '--datapath', datapath] + flow + ['--testres', '1']
    kinds4, kinds2 = ('JPEGImages', 'Annotations', 'FlowFW', 'FlowBW'), ('FlowFW', 'FlowBW')
    add('flow-r', 'flow', gen + ['--outdir', './' + rseq] + args.passthrough['auto_gen'], inputs=[seq_dir('JPEGImages', seq), ann],
        outputs=[seq_dir(k, rseq) for k in kinds4], work=pair_pixels, pre=[('remove_tree', rseq)],
        post=[('copy_tree', '%s/%s' % (rseq, k), seq_dir(k, rseq)) for k in kinds4])
    add('flow', 'flow', gen + ['--flow_threshold', '0', '--outdir', './' + seq] + args.passthrough['auto_gen'],
        inputs=[seq_dir('JPEGImages', seq), ann], outputs=[seq_dir(k, seq) for k in kinds2], work=pair_pixels,
        pre=[('remove_tree', seq)], post=[('copy_tree', '%s/%s' % (seq, k), seq_dir(k, seq)) for k in kinds2])

    add('config', 'local', inputs=[], outputs=['configs/%s.config' % seq, 'configs/%s.config' % rseq],
        pre=[('write_configs', seq, args.dframe, args.init_frame, args.end_frame, args.can_frame)])

    flags, ckpt = None, None
    for k, stage in enumerate(args.stages):
        flags = stage_flags(args, stage)
        name = '%s-%d' % (seq, k)
        argv = [py, script('optimize.py'), '--name=' + name, '--checkpoint_dir', 'log/'] + flag_tokens(flags)
        if ckpt:
            argv += ['--model_path', ckpt]
        out = 'log/%s/pred_net_latest.pth' % name
        limit = stage.get('timeout_s')
        add('stage-%d' % k, 'stage', argv, inputs=data_inputs(flags['dataname']) + ([ckpt] if ckpt else []), outputs=[out],
            work=stage_work(flags), timeout_s=None if limit is None else int(math.ceil(float(limit))))
        ckpt = out
    last = '%s-%d' % (seq, len(args.stages) - 1)
    testdir = 'log/%s/' % last
    flags = collections.OrderedDict(flags, dataname=seq)
    add('extract', 'extract', [py, script('extract.py'), '--rig', '--name=' + last, '--checkpoint_dir', 'log/'] + flag_tokens(flags) +
        ['--model_path', ckpt], inputs=data_inputs(seq) + [ckpt], outputs=[testdir + 'rig.npz'], work=T)
    meshes = [testdir.rstrip('/')] + data_inputs(seq)
    common = ['--testdir', testdir, '--seqname', seq]
    add('scores-reproj', 'eval_reproj', [py, script('scripts', 'eval_reproj.py')] + common +
        ['--outpath', OUT + '/reproj.json', '--worst', str(args.worst)], inputs=meshes, outputs=[OUT + '/reproj.json'], work=T)
    add('scores-shape', 'eval_shape', [py, script('scripts', 'eval_shape.py')] + common +
        ['--outpath', OUT + '/shape.json', '--worst', str(args.worst)] + (['--neighbours'] if getattr(args, 'neighbours', False) else []),
        inputs=meshes, outputs=[OUT + '/shape.json'], work=T)
    if args.gif:
        add('gif', 'render_vis', [py, script('render_vis.py')] + common + ['--outpath', '%s/%s.gif' % (OUT, seq)], inputs=meshes,
            outputs=['%s/%s.gif' % (OUT, seq)], work=T)
    if args.atlas:
        add('atlas', 'bake_texture', [py, script('scripts', 'bake_texture.py')] + common + ['--outpath', OUT + '/baked'], inputs=meshes,
            outputs=[OUT + '/baked.obj', OUT + '/baked.mtl', OUT + '/baked.png'], work=T)
    if args.glb:
        tex = ['--texture_obj', OUT + '/baked.obj'] if args.atlas else []
        add('glb', 'export_gltf', [py, script('scripts', 'export_gltf.py'), '--testdir', testdir, '--outpath', '%s/%s.glb' % (OUT, seq)] + tex,
            inputs=[testdir + 'rig.npz'] + tex[1:], outputs=['%s/%s.glb' % (OUT, seq)], work=T)
    if args.tracks:
        add('tracks', 'export_tracks', [py, script('scripts', 'export_tracks.py')] + common + ['--outpath', OUT + '/tracks.npz'],
            inputs=meshes, outputs=[OUT + '/tracks.npz'], work=T)
    return steps


def passed_gamma(tokens, flag='--vf_gamma'):
    """The value of the last --vf_gamma (or `flag`) among a script's handed-through tokens (`--vf_gamma 5` or `--vf_gamma=5`); 0
    without one or with one the script itself will refuse."""
    val = 0.
    for i, tok in enumerate(tokens):
        if tok == flag or tok.startswith(flag + '='):
            text = tok.partition('=')[2] if '=' in tok else (tokens[i + 1] if i + 1 < len(tokens) else '')
            try:
                val = float(text)
            except ValueError:
                val = 0.
    return val


def describe(args):
    """What report() needs to know about the run and cannot read from the files the steps leave: stored as reconstruct/run.json."""
    route = mask_route(args)
    stages = [stage_flags(args, s) for s in args.stages]
    used = [] if route == 'given' else [route]
    used.append('variational' if args.flow_method == 'variational' else ('vcn_dry' if not args.loadmodel else None))
    if args.flow_method == 'variational' and passed_gamma(getattr(args, 'passthrough', {}).get('auto_gen', [])) > 0:
        used.append('gradient_constancy')
    if args.flow_method == 'variational' and passed_gamma(getattr(args, 'passthrough', {}).get('auto_gen', []), '--vf_match') > 0:
        used.append('large_displacement')
    used += ['ssim' if f.get('ptex_method', 'alexnet') == 'ssim' else ('alexnet_random' if not f.get('alexnet_weights') else None)
             for f in stages[:1]]
    if any(float(f.get(key, 0.)) != 0. for f in stages for key in ('fold_wt', 'pierce_wt')):
        used.append('fold_penalty')
    if any(float(f.get('isect_wt', 0.)) != 0. for f in stages):
        used.append('isect_penalty')
    used += [None if args.encoder_weights else 'encoder_random', 'one_gpu', 'eval_reproj',
             'eval_shape_neighbours' if getattr(args, 'neighbours', False) else 'eval_shape',
             'bake_texture' if args.atlas else None, 'export_tracks' if args.tracks else None]
    return dict(seqname=args.seqname, frames=args.n_frames, size=[args.width, args.height], mask_route=route,
                flow_method=args.flow_method, schedule=args.schedule_name, stages=[dict(f) for f in stages], worst=args.worst,
                pieces=[u for u in CAVEATS if u in used])


def driver_argv(args):
    """The driver's own command line again, from the parsed arguments: absolute paths (the printed lines run in the work directory),
    what differs from the defaults, without --dry_run, --from, --until, --force and what follows `--`."""
    p = build_parser()
    out = []
    for name in ('frames', 'seqname', 'workdir', 'masks', 'loadmodel', 'flow_method', 'alexnet_weights', 'encoder_weights', 'schedule',
                 'dframe', 'init_frame', 'end_frame', 'can_frame', 'fold_wt', 'pierce_wt', 'isect_wt', 'worst', 'timeout_scale'):
        val = getattr(args, name)
        if val != p.get_default(name) and not (name == 'flow_method' and val == ('vcn' if args.loadmodel else 'variational')):
            out += ['--' + name, str(val)]
    for k, path in args.key:
        out += ['--key', '%d:%s' % (k, path)]
    return out + ['--' + name for name in ('gif', 'atlas', 'glb', 'tracks', 'neighbours') if getattr(args, name, False)]


def shell_lines(steps, args):
    """The plan as one shell line per step, each under `timeout -k 10 <limit>` and ending in `&&` but the last.  A step without a
    child is the driver itself bounded to that step; the copies after a flow pass are the cp lines of preprocess/auto_gen.sh."""
    lines = []
    me = [sys.executable, os.path.join(ROOT, 'scripts', 'reconstruct.py')] + driver_argv(args)
    for st in steps:
        argv = list(st.argv) if st.argv else me + ['--from', st.name, '--until', st.name] + (['--'] + args.extra if args.extra else [])
        parts = ['timeout -k %d %d rm -rf ./%s' % (KILL_AFTER_S, LOCAL_S, shlex.quote(act[1])) for act in (st.pre if st.argv else ())
                 if act[0] == 'remove_tree']
        parts.append('timeout -k %d %d %s' % (KILL_AFTER_S, st.timeout_s, ' '.join(shlex.quote(a) for a in argv)))
        for act in st.post if st.argv else ():
            if act[0] == 'copy_tree':
                parts.append('mkdir -p %s && cp -rf %s/. %s/' % (shlex.quote(act[2]), shlex.quote(act[1]), shlex.quote(act[2])))
        lines.append(' && '.join(parts))
    return [ln + (' &&' if i + 1 < len(lines) else '') for i, ln in enumerate(lines)]


# ---- in-process actions --------------------------------------------------------------------------------------------------------
def install_frames(workdir, src, seq):
    """The frames of `src` in natural order -> JPEGImages/<res>/<seq>/%05d.jpg, quality 95 (what auto_gen.py writes)."""
    from PIL import Image
    if not src:
        raise PipelineError('install: --frames is required to install a sequence')
    paths = list_images(src)
    if not paths:
        raise PipelineError('install: no frames under %s' % src)
    if len(paths) < 3:
        raise PipelineError('install: %d frames under %s, at least 3 are needed' % (len(paths), src))
    size = None
    for p in paths:                                    # refuse before anything is written
        with Image.open(p) as im:
            if size is not None and im.size != size:
                raise PipelineError('install: %s is %d x %d, %s is %d x %d' % ((p,) + im.size + (paths[0],) + size))
            size = im.size
    out = os.path.join(workdir, seq_dir('JPEGImages', seq))
    if os.path.isdir(out):
        shutil.rmtree(out)
    os.makedirs(out)
    for i, p in enumerate(paths):
        with Image.open(p) as im:
            im.convert('RGB').save(os.path.join(out, '%05d.jpg' % i), quality=95)
    return len(paths)


def install_masks(workdir, src, seq):
    """One image per frame, in natural order, any non-zero pixel = object -> Annotations/<res>/<seq>/%05d.png in the loader's
    encoding (128 in the red channel)."""
    import numpy as np
    from PIL import Image
    paths = list_images(src)
    frames = list_images(os.path.join(workdir, seq_dir('JPEGImages', seq)))
    if len(paths) != len(frames):
        raise PipelineError('masks: %d images under %s for %d frames' % (len(paths), src, len(frames)))
    out = os.path.join(workdir, seq_dir('Annotations', seq))
    if os.path.isdir(out):
        shutil.rmtree(out)
    os.makedirs(out)
    with Image.open(frames[0]) as im:
        size = im.size
    for i, p in enumerate(paths):
        with Image.open(p) as im:
            if im.size != size:
                raise PipelineError('masks: %s is %d x %d, the frames are %d x %d' % ((p,) + im.size + size))
            on = np.asarray(im.convert('RGB')).any(-1)
        if not on.any():
            raise PipelineError('masks: %s is empty' % p)
        enc = np.zeros(on.shape + (3,), np.uint8)
        enc[..., 0] = on * np.uint8(128)
        Image.fromarray(enc).save(os.path.join(out, '%05d.png' % i))
    return len(paths)


def copy_tree(workdir, src, dst):
    """cp -rf src/. dst/ (preprocess/auto_gen.sh), after emptying dst: a shorter pass leaves no file of a longer one behind."""
    s, d = os.path.join(workdir, src), os.path.join(workdir, dst)
    if not os.path.isdir(s):
        raise PipelineError('%s was not written' % src)
    if os.path.isdir(d):
        shutil.rmtree(d)
    shutil.copytree(s, d)


def remove_tree(workdir, rel):
    """rm -rf of a pass's own output folder, so that a shorter pass leaves no pair of a longer one behind."""
    full = os.path.join(workdir, rel)
    if os.path.isdir(full):
        shutil.rmtree(full)


def config_text(seq, dframe, init_frame, end_frame, can_frame):
    return ('[data]\ndatapath = %s/\ndframe = %d\ninit_frame = %d\nend_frame = %d\ncan_frame = %d\n'
            % (seq_dir('JPEGImages', seq), dframe, init_frame, end_frame, can_frame))


def write_configs(workdir, seq, dframe, init_frame, end_frame, can_frame):
    os.makedirs(os.path.join(workdir, 'configs'), exist_ok=True)
    for name in (seq, 'r' + seq):
        with open(os.path.join(workdir, 'configs', '%s.config' % name), 'w') as fh:
            fh.write(config_text(name, dframe, init_frame, end_frame, can_frame))


ACTIONS = dict(remove_tree=remove_tree, install_frames=install_frames, install_masks=install_masks, copy_tree=copy_tree, write_configs=write_configs)


# ---- the runner ----------------------------------------------------------------------------------------------------------------
def listing(workdir, paths):
    """[(path, size)] of the files named, a folder standing for the files under it; what is missing is listed with size -1."""
    out = []
    for rel in paths:
        full = os.path.join(workdir, rel)
        if os.path.isdir(full):
            for d, dirs, files in os.walk(full):
                dirs.sort()
                for f in sorted(files):
                    p = os.path.join(d, f)
                    out.append((os.path.relpath(p, workdir) if not os.path.isabs(rel) else p, os.path.getsize(p)))
        elif os.path.exists(full):
            out.append((rel, os.path.getsize(full)))
        else:
            out.append((rel, -1))
    return out


def step_hash(step, workdir, previous):
    doc = [list(step.argv) if step.argv else None, [list(a) for a in step.pre + step.post], listing(workdir, step.inputs), previous]
    return hashlib.sha256(json.dumps(doc, sort_keys=True).encode()).hexdigest()


def find_step(steps, name, last=False):
    """Index of the step called `name`; a name such as `scores` or `stage` stands for the steps `name-...`: the first of them, or
    with last=True the last."""
    hits = [i for i, s in enumerate(steps) if s.name == name] or [i for i, s in enumerate(steps) if s.name.startswith(name + '-')]
    if not hits:
        raise PipelineError('no step %r in the plan: %s' % (name, ' '.join(s.name for s in steps)))
    return hits[-1] if last else hits[0]


def _group_alive(pgid):
    try:
        os.killpg(pgid, 0)
        return True
    except OSError:
        return False


def _end_group(pgid, proc):
    """SIGTERM to the child's process group, SIGKILL after KILL_AFTER_S if any of it is left."""
    try:
        os.killpg(pgid, signal.SIGTERM)
    except OSError:
        pass
    deadline = time.monotonic() + KILL_AFTER_S
    while time.monotonic() < deadline:
        if proc.poll() is not None and not _group_alive(pgid):
            return
        time.sleep(0.05)
    try:
        os.killpg(pgid, signal.SIGKILL)
    except OSError:
        pass
    proc.wait()


def run_child(step, log_path):
    """One fresh process in its own process group, the driver's environment untouched, stdout and stderr into the log.
    -> (return code, timed out)."""
    with open(log_path, 'ab') as log:
        proc = subprocess.Popen(list(step.argv), cwd=step.cwd, stdin=subprocess.DEVNULL, stdout=log, stderr=subprocess.STDOUT,
                                start_new_session=True)
        try:
            try:
                return proc.wait(step.timeout_s), False
            except subprocess.TimeoutExpired:
                _end_group(proc.pid, proc)
                return proc.returncode, True
        except BaseException:                          # the driver itself is being stopped: leave nothing running
            _end_group(proc.pid, proc)
            raise
        finally:
            if _group_alive(proc.pid):                 # a child that left something of its group behind
                _end_group(proc.pid, proc)


def tail(path, n=TAIL_LINES):
    try:
        with open(path, errors='replace') as fh:
            return fh.read().splitlines()[-n:]
    except OSError:
        return []


def run(steps, workdir, start=None, until=None, force=(), meta=None, out=None):
    """Runs the plan under the rules of the module docstring.  -> 0, EXIT_FAILED (a step exited non-zero or was refused) or
    EXIT_TIMED_OUT.  meta: written to reconstruct/run.json for report()."""
    out = out or sys.stdout
    say = lambda text: (out.write(text + '\n'), out.flush())                   # noqa: E731
    lo = find_step(steps, start) if start else 0
    hi = find_step(steps, until, last=True) if until else len(steps) - 1
    forced = set()
    for name in force:
        first, last = find_step(steps, name), find_step(steps, name, last=True)
        forced.update(range(first, last + 1) if steps[first].name != name else [first])
    sdir = os.path.join(workdir, OUT, 'steps')
    os.makedirs(sdir, exist_ok=True)
    if meta is not None:
        with open(os.path.join(workdir, OUT, 'run.json'), 'w') as fh:
            json.dump(meta, fh, indent=1)
    previous, dirty = '', False
    for i, st in enumerate(steps):
        base = os.path.join(sdir, '%02d-%s' % (i, st.name))
        stamp = None
        if os.path.exists(base + '.json') and i not in forced:
            try:
                with open(base + '.json') as fh:
                    stamp = json.load(fh)
            except ValueError:
                stamp = None
        if i < lo:
            previous = stamp['hash'] if stamp else ''
            continue
        if i > hi:
            break
        digest = step_hash(st, workdir, previous)
        if (not dirty and stamp and stamp.get('hash') == digest
                and all(os.path.exists(os.path.join(workdir, o)) for o in st.outputs)):
            say('%-14s up to date' % st.name)
            previous = digest
            continue
        dirty = True
        for ext in ('.json', '.log'):
            if os.path.exists(base + ext):
                os.remove(base + ext)
        say('%-14s %s' % (st.name, 'limit %d s' % st.timeout_s if st.argv else 'in process'))
        t0 = time.monotonic()
        rc, timed_out, refusal = 0, False, None
        try:
            with open(base + '.log', 'a') as log:
                for act in st.pre:
                    log.write('%s %s\n' % (act[0], ' '.join(str(a) for a in act[1:])))
                    ACTIONS[act[0]](workdir, *act[1:])
            if st.argv:
                rc, timed_out = run_child(st, base + '.log')
            if rc == 0 and not timed_out:
                with open(base + '.log', 'a') as log:
                    for act in st.post:
                        log.write('%s %s\n' % (act[0], ' '.join(str(a) for a in act[1:])))
                        ACTIONS[act[0]](workdir, *act[1:])
                missing = [o for o in st.outputs if not os.path.exists(os.path.join(workdir, o))]
                if missing:
                    raise PipelineError('the step ended without writing %s' % ', '.join(missing))
        except PipelineError as e:
            refusal = str(e)
            with open(base + '.log', 'a') as log:
                log.write(refusal + '\n')
        seconds = time.monotonic() - t0
        if timed_out or rc != 0 or refusal:
            what = 'timed out after %d s' % st.timeout_s if timed_out else 'failed'
            say('step %s %s: return code %s.  Nothing further is started.  Last lines of %s:' % (st.name, what, rc, base + '.log'))
            for line in tail(base + '.log'):
                say('  | ' + line)
            return EXIT_TIMED_OUT if timed_out else EXIT_FAILED
        with open(base + '.json', 'w') as fh:
            json.dump(dict(name=st.name, argv=list(st.argv) if st.argv else None, actions=[list(a) for a in st.pre + st.post],
                           hash=digest, returncode=rc, seconds=round(seconds, 3), timeout_s=st.timeout_s,
                           outputs=listing(workdir, st.outputs)), fh, indent=1)
        previous = digest
    return 0


# ---- the report ----------------------------------------------------------------------------------------------------------------
def _json(path):
    try:
        with open(path) as fh:
            return json.load(fh)
    except (OSError, ValueError):
        return None


def _last_total_loss(path):
    """The last total_loss of a monitor's scalars.csv (optimize.py --monitor), None when the stage wrote none."""
    try:
        with open(path) as fh:
            rows = [ln.strip().split(',') for ln in fh if ln.strip()]
    except OSError:
        return None
    if len(rows) < 2 or 'total_loss' not in rows[0]:
        return None
    try:
        return float(rows[-1][rows[0].index('total_loss')].split('=')[-1])
    except (ValueError, IndexError):
        return None


def _worst(doc, key, count, highest):
    per, ids = doc.get('per_frame', {}).get(key) or [], doc.get('frame_ids') or []
    have = [(v, i) for i, v in enumerate(per) if v is not None]
    have.sort(key=lambda x: (-x[0] if highest else x[0], x[1]))
    return [dict(frame=ids[i] if i < len(ids) else i, value=v) for v, i in have[:max(count, 0)]]


def report(workdir):
    """Writes reconstruct/report.json and report.md from what the steps left; what is absent is left out.  -> the document."""
    odir = os.path.join(workdir, OUT)
    meta = _json(os.path.join(odir, 'run.json')) or {}
    seq = meta.get('seqname', '')
    count = lambda kind, name: len(list_images(os.path.join(workdir, seq_dir(kind, name)))) \
        if os.path.isdir(os.path.join(workdir, seq_dir(kind, name))) else None      # noqa: E731
    stamps = {}
    sdir = os.path.join(odir, 'steps')
    for f in sorted(os.listdir(sdir)) if os.path.isdir(sdir) else []:
        doc = _json(os.path.join(sdir, f)) if f.endswith('.json') else None
        if doc and 'name' in doc:
            stamps[doc['name']] = doc
    doc = collections.OrderedDict()
    doc['sequence'] = dict(name=seq, frames=count('JPEGImages', seq) if seq else None, size=meta.get('size'),
                           frames_kept_in_r=count('JPEGImages', 'r' + seq) if seq else None)
    masks = dict(route=meta.get('mask_route'))
    prop = _json(os.path.join(workdir, seq_dir('Annotations', seq), 'maskprop.json')) if seq else None
    if prop:
        masks['keys'] = prop.get('keys')
        if prop.get('motion'):
            masks['motion_scores'] = prop['motion'].get('scores')
        if prop.get('roundtrip_iou') is not None:
            masks['roundtrip_iou'] = prop['roundtrip_iou']
    doc['masks'] = masks
    doc['flow_method'] = meta.get('flow_method')
    doc['schedule'] = meta.get('schedule')
    doc['stages'] = []
    for k, flags in enumerate(meta.get('stages', [])):
        st = stamps.get('stage-%d' % k)
        doc['stages'].append(dict(name='stage-%d' % k, flags=flags, seconds=st['seconds'] if st else None,
                                  total_loss=_last_total_loss(os.path.join(workdir, 'log', '%s-%d' % (seq, k), 'monitor', 'scalars.csv'))))
    worst = meta.get('worst', 5)
    doc['scores'] = {}
    for name, key, highest in (('reproj', 'JF', False), ('shape', 'ratio', True)):
        s = _json(os.path.join(odir, name + '.json'))
        if s:
            doc['scores'][name] = dict(means=s.get('means'), worst_by=key, worst=_worst(s, key, worst, highest))
    exports = [name for name in sorted(os.listdir(odir)) if name.endswith(('.gif', '.glb', '.obj', '.mtl', '.png', '.npz'))] \
        if os.path.isdir(odir) else []
    doc['exports'] = [OUT + '/' + name for name in exports]
    doc['seconds'] = {name: st['seconds'] for name, st in stamps.items()}
    doc['caveats'] = [CAVEATS[p] for p in meta.get('pieces', []) if p in CAVEATS]
    os.makedirs(odir, exist_ok=True)
    with open(os.path.join(odir, 'report.json'), 'w') as fh:
        json.dump(doc, fh, indent=1)
    with open(os.path.join(odir, 'report.md'), 'w') as fh:
        fh.write(markdown(doc))
    return doc


def markdown(doc):
    fmt = lambda v: 'n/a' if v is None else ('%.4g' % v if isinstance(v, float) else str(v))     # noqa: E731
    s = doc['sequence']
    lines = ['# Reconstruction of `%s`' % s['name'], '',
             '* frames: %s, size %s, kept in `r%s` after frame selection: %s' % (fmt(s['frames']), fmt(s['size']), s['name'], fmt(s['frames_kept_in_r'])),
             '* silhouettes: %s%s' % (fmt(doc['masks'].get('route')), ''.join(', %s %s' % (k, doc['masks'][k]) for k in
                                                                          ('keys', 'motion_scores', 'roundtrip_iou') if k in doc['masks'])),
             '* flow: %s; schedule: %s' % (fmt(doc['flow_method']), fmt(doc['schedule'])), '', '## Stages', '',
             '| stage | seconds | last total loss | flags |', '|---|---|---|---|']
    for st in doc['stages']:
        lines.append('| %s | %s | %s | `%s` |' % (st['name'], fmt(st['seconds']), fmt(st['total_loss']), ' '.join(flag_tokens(st['flags']))))
    lines += ['', '## Scores (no ground truth)', '']
    for name, sc in doc['scores'].items():
        lines.append('* %s: %s' % (name, ', '.join('%s %s' % (k, fmt(v)) for k, v in (sc['means'] or {}).items())))
        lines.append('  worst by %s: %s' % (sc['worst_by'], ', '.join('frame %s (%s)' % (w['frame'], fmt(w['value'])) for w in sc['worst']) or 'n/a'))
    lines += ['', '## Exports', ''] + (['* `%s`' % e for e in doc['exports']] or ['none'])
    lines += ['', '## Unverified', ''] + ['* ' + c for c in doc['caveats']]
    return '\n'.join(lines) + '\n'


# ---- the command ---------------------------------------------------------------------------------------------------------------
def main(argv=None, out=None):
    """scripts/reconstruct.py: arguments, plan, run, report.  -> the exit status."""
    out = out or sys.stdout
    argv = list(sys.argv[1:] if argv is None else argv)
    args = parse_args(argv)
    try:
        probe(args)
        steps = plan(args)
        if args.dry_run:
            sys.stderr.write('# the lines below run in the work directory: mkdir -p %s && cd %s\n' % ((shlex.quote(args.workdir),) * 2))
            for line in shell_lines(steps, args):
                out.write(line + '\n')
            return 0
        rc = run(steps, args.workdir, start=args.start, until=args.until, force=args.force, meta=describe(args), out=out)
    except PipelineError as e:
        out.write('reconstruct.py: %s\n' % e)
        return EXIT_FAILED
    if rc == 0:
        report(args.workdir)
        out.write('report: %s\n' % os.path.join(args.workdir, OUT, 'report.md'))
    return rc
