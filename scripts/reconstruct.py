#!/usr/bin/env python3
"""From a folder of frames to a reconstruction and a report, in one resumable command (lasr_amd/pipeline.py).

    python scripts/reconstruct.py --frames ~/cat/ --seqname cat --workdir runs/cat [--key 0:first.png | --masks DIR]
           [--schedule quick|template|FILE] [--glb] [--gif] [--atlas] [--tracks] [--neighbours] [--dry_run] [--from S] [--until S]
           [--force S] [--fold_wt W] [--pierce_wt W] [--isect_wt W]
           [--timeout_scale 1.0] [-- flags passed through to the preprocessing scripts]

Steps, each a fresh child process with the work directory as its current one, one at a time, each under its own time limit:
install (the frames into the DAVIS layout), masks (--masks: given; --key: preprocess/propagate_mask.py; neither:
preprocess/auto_mask.py), flow-r and flow (the two passes of preprocess/auto_gen.sh), config (configs/<seq>.config and
configs/r<seq>.config), stage-0 ... stage-N (optimize.py, one run per stage of the schedule, each warm-started from the one
before), extract (extract.py --rig), scores-reproj and scores-shape (scripts/eval_reproj.py, scripts/eval_shape.py) and the exports
asked for.  Without --loadmodel and --alexnet_weights nothing needs a download: the flow is --flow_method variational, the texture
term --ptex_method ssim; for footage whose lighting changes, `-- --vf_gamma 5` hands the gradient-constancy term of that flow to
the masks and both flow steps, and `-- --vf_match 24` its large-displacement matching stage, for small parts that move further than
their own size (the report names either among the unverified pieces).  The first step that fails or runs into its limit ends the run (exit status 2 or 3) and nothing is started
after it; the same command again resumes at the first step whose stamp under <workdir>/reconstruct/steps/ no longer matches.
--neighbours hands scripts/eval_shape.py its flag of that name: folds between neighbouring faces are scored too (n_pierced, n_creased,
min_dihedral in the report; the angle threshold is unmeasured on real footage, and the report says so).
--fold_wt W and --pierce_wt W hand every optimize.py stage the weights of the fold penalty on the posed meshes
(scripts/fold_penalty.py), which acts on what --neighbours reports; both are 0 by default (off) and unmeasured on real footage, and
the report says so.
--isect_wt W hands every optimize.py stage the weight of the intersection penalty between faces that share no vertex
(scripts/isect_penalty.py), which acts on the n_pairs of the shape report; 0 by default (off) and unmeasured on real footage, and the
report says so.
--dry_run prints the plan as shell lines and does nothing else.  The run ends in <workdir>/reconstruct/report.md and report.json.
"""
import os
import signal
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from lasr_amd import pipeline   # noqa: E402


def _stop(signum, frame):
    raise SystemExit(128 + signum)                     # unwinds through the runner, which ends the running child's process group


def main(argv=None):
    signal.signal(signal.SIGTERM, _stop)
    return pipeline.main(argv)


if __name__ == '__main__':
    sys.exit(main())
