#!/usr/bin/env python3
"""Silhouettes for a video from motion alone: no painted frame (lasr_amd/nnutils/motionseg.py).

    python preprocess/auto_mask.py --datapath database/DAVIS/JPEGImages/Full-Resolution/mine/ --flow_method variational \\
           [--n_keys 2] [--ms_gap 3] [--ms_model affine] [--keys_only] [--roundtrip] [--min_area 1000] [--force]

preprocess/propagate_mask.py needs the object painted in one frame.  This script finds that frame and paints it: it fits the
dominant (camera-induced) motion of every flow field robustly, takes what does not follow it as the object, picks the frames where
that evidence is cleanest, writes them as key-%05d.png (the reference's mask encoding) into --keydir, prints the equivalent
propagate_mask.py command line, and, unless --keys_only is given, runs that propagation with the flows it has already computed.
maskprop.json then carries a `motion` block: the parameters, the per-frame scores, the chosen keys and theta, sigma of every pair.
auto_gen.py runs next, unchanged.

Quality on real footage is unverified.  It is meant for one object below half the frame, over a background that is far, planar or
seen by a rotating camera (parallax reads as motion), and the object has to move against the background in the chosen frames:
--ms_gap widens the frame distance for slow objects, --ms_model picks a simpler camera model.
"""
import argparse
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import auto_gen          # noqa: E402
import propagate_mask    # noqa: E402

# one --ms_<name> flag per entry of lasr_amd.nnutils.motionseg.DEFAULTS (tests/test_motionseg_cpu.py compares the two)
MOTION = (('tau', float, 1., 'forward-backward flow disagreement (px) at which a pixel loses 39 % of its weight'),
          ('model', str, 'quadratic', 'dominant-motion model: translation, affine or quadratic'),
          ('iters', int, 8, 'IRLS iterations of the motion fit'),
          ('k_sigma', float, 3., 'scale of the robust weight in medians of the residual'),
          ('sigma_min', float, 0.25, 'floor of that scale (px)'),
          ('ridge', float, 1e-9, 'diagonal load of the normal matrix, in units of its mean diagonal'),
          ('kappa', float, 4., 'squared residual, in units of the scale, above which a pixel counts for the object'),
          ('U', float, 6., 'clamp of a pair\'s evidence'),
          ('gap', int, 1, 'frame distance of the pairs the motion is read from; raise it for a slow object'),
          ('min_share', float, 0.01, 'a mask below this share of the frame scores 0'),
          ('max_share', float, 0.5, 'a mask above this share of the frame scores 0'),
          ('min_spacing', int, 10, 'least distance in frames between two keys'),
          ('min_score', float, 1., 'a frame below this score is no key'),
          ('n_keys', int, 1, 'number of key frames'))


def parse_args(argv=None):
    p = argparse.ArgumentParser(description='silhouettes from motion alone: key masks, then the propagation', allow_abbrev=False)
    p.add_argument('--datapath', required=True, help='folder of the frames (.../JPEGImages/.../<seq>/)')
    p.add_argument('--keydir', default=None, help='folder of the key masks (default: <Annotations folder>.autokeys)')
    p.add_argument('--keys_only', action='store_true', help='write the key masks and stop: no propagation')
    p.add_argument('--loadmodel', default=None, help='VCN checkpoint (vcn_rob.pth); none: dry run with random weights')
    p.add_argument('--testres', type=float, default=1, help='resolution of the flow network')
    p.add_argument('--maxdisp', type=int, default=256, help='maximum disparity of the flow network')
    p.add_argument('--fac', type=float, default=1, help='squeezes the coarsest search window along y')
    p.add_argument('--roundtrip', action='store_true', help='propagate from the first key to the last frame and back; print the IoU')
    p.add_argument('--min_area', type=int, default=1000, help='masks smaller than this many pixels are reported, not written')
    p.add_argument('--force', action='store_true', help='write into folders that already hold files')
    for name, kind, default, text in MOTION:
        flags = ('--n_keys', '--ms_n_keys') if name == 'n_keys' else ('--ms_' + name,)
        extra = dict(choices=('translation', 'affine', 'quadratic')) if name == 'model' else {}
        p.add_argument(*flags, dest='ms_' + name, type=kind, default=default, help='%s (default %s)' % (text, default), **extra)
    for name, kind, default, text in propagate_mask.TUNING:
        p.add_argument('--' + name, type=kind, default=default, help='propagation: %s (default %s)' % (text, default))
    auto_gen.add_flow_arguments(p)
    args = p.parse_args(argv)
    auto_gen.check_flow_arguments(p, args)
    return args


def motion_of(args):
    return {name: getattr(args, 'ms_' + name) for name, _, _, _ in MOTION}


def key_dir(args):
    return args.keydir or propagate_mask.annotations_dir(args.datapath) + '.autokeys'


def propagate_argv(args, key_paths):
    """The propagate_mask.py command line that repeats this run from the written keys."""
    argv = ['--datapath', args.datapath]
    for t, path in sorted(key_paths.items()):
        argv += ['--key', '%d:%s' % (t, path)]
    argv += ['--min_area', str(args.min_area), '--flow_method', args.flow_method]
    if args.loadmodel is not None:
        argv += ['--loadmodel', args.loadmodel]
    for name in ('testres', 'maxdisp', 'fac'):
        argv += ['--' + name, str(getattr(args, name))]
    for name, _, _, _ in propagate_mask.TUNING:
        argv += ['--' + name, str(getattr(args, name))]
    for name, _, _, _ in auto_gen.FLOW_TUNING:
        argv += ['--vf_' + name, str(getattr(args, 'vf_' + name))]
    for name, _, default, _ in auto_gen.FLOW_ROBUST:                               # (a default run prints the line it always printed)
        if getattr(args, 'vf_' + name) != default:
            argv += ['--vf_' + name, str(getattr(args, 'vf_' + name))]
    for _, suffix, _, default, _, _ in auto_gen.FLOW_MATCH:
        if getattr(args, 'vf_match' + suffix) != default:
            argv += ['--vf_match' + suffix, str(getattr(args, 'vf_match' + suffix))]
    for flag in ('roundtrip', 'force'):
        if getattr(args, flag):
            argv.append('--' + flag)
    return argv


def write_keys(out, keys, force):
    from PIL import Image
    if os.path.isdir(out) and os.listdir(out) and not force:
        raise propagate_mask.AnnotationsExist('%s already holds %d files; pass --force to write into it' % (out, len(os.listdir(out))))
    os.makedirs(out, exist_ok=True)
    paths = {}
    for t, m in sorted(keys.items()):
        paths[t] = os.path.join(out, 'key-%05d.png' % t)
        Image.fromarray(propagate_mask.encode_mask(m)).save(paths[t])
    return paths


def run(args, flow_fn, segment=None, propagate=None, roundtrip=None):
    """The whole script with flow_fn(imgA, imgB) -> (flow [H,W,>=2], occ), as auto_gen.run takes it.  segment / propagate /
    roundtrip default to lasr_amd.nnutils.motionseg.segment and maskprop's (the device passes).  -> the `motion` block."""
    from lasr_amd.nnutils import motionseg
    segment = segment or motionseg.segment
    if not args.keys_only:
        propagate_mask.prepare_output(args.datapath, args.force)                    # refuse before the flows are computed
    paths = sorted(p for p in glob.glob('%s/*' % args.datapath))
    if not paths:
        raise FileNotFoundError('no frames under %s' % args.datapath)
    frames = [auto_gen.read_rgb(p) for p in paths]
    flow_fn = motionseg.caching_flow_fn(flow_fn)
    motion = motion_of(args)
    masks, _, scores, rep = segment(frames, flow_fn, **motion)
    keys = motionseg.select_keys([float(v) for v in scores], motionseg.params(**motion))
    key_paths = write_keys(key_dir(args), {t: masks[t] for t in keys}, args.force)
    block = dict(params=motion, scores=[float(v) for v in scores], keys=keys, key_paths=[key_paths[t] for t in keys],
                 pairs=rep.get('pairs', []))
    argv = propagate_argv(args, key_paths)
    print('auto_mask.py: key frame%s %s (score %s) written to %s' % ('s' if len(keys) > 1 else '', keys,
                                                                     ', '.join('%.2f' % scores[t] for t in keys), key_dir(args)))
    print('  the same propagation by hand: python preprocess/propagate_mask.py %s' % ' '.join(argv))
    if args.keys_only:
        return block
    pargs = propagate_mask.parse_args(argv)
    propagate_mask.run(pargs, flow_fn, propagate=propagate, roundtrip=roundtrip)
    block['flow_calls'] = flow_fn.calls
    report_path = os.path.join(propagate_mask.annotations_dir(args.datapath), 'maskprop.json')
    with open(report_path) as f:
        report = json.load(f)
    report['motion'] = block
    with open(report_path, 'w') as f:
        json.dump(report, f, indent=1)
    return block


def main(argv=None):
    args = parse_args(argv)
    if args.flow_method == 'variational':
        flow_fn = auto_gen.variational_flow_fn(args)
    else:
        model = auto_gen.build_model(args)
        flow_fn = lambda a, b: auto_gen.flow_inference(model, a, b, args.testres)   # noqa: E731
    from lasr_amd.nnutils.maskprop import EmptyPropagation
    from lasr_amd.nnutils.motionseg import NoMovingObject
    try:
        run(args, flow_fn)
    except NoMovingObject as e:
        sys.exit('auto_mask.py: %s.  Try a wider frame distance (--ms_gap 3), a simpler camera model (--ms_model affine), or paint '
                 'a key by hand and run propagate_mask.py --key' % e)
    except (EmptyPropagation, propagate_mask.AnnotationsExist, ValueError) as e:
        sys.exit('auto_mask.py: %s' % e)


if __name__ == '__main__':
    main()
