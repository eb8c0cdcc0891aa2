#!/usr/bin/env python3
"""Writes tests/golden/flowvis.npz: float64 flow fields and what the reference's flowlib.flow_to_image makes of them.

    python tools/gen_flowvis_golden.py [--reference /root/reference]

Runs on the CPU.  The reference module imports `png`, `cv2` and matplotlib at its top, none of which flow_to_image uses: empty
stand-ins go into sys.modules for the ones that are not installed.  Inputs are float64 so that the reference's result does not
depend on the numpy version's scalar promotion.  Cases: in_<name> [H,W,C], optional mask_<name> [H,W] (applied the way the trainer
does before the call, nnutils/train_utils.py:307: u = v = 0 where it is 0), out_<name> uint8 [H,W,3].  No NaN case: the reference's
behaviour there is an accident."""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_reference(ref_root):
    for name in ('png', 'cv2', 'matplotlib', 'matplotlib.colors', 'matplotlib.pyplot'):
        try:
            importlib.import_module(name)
        except Exception:
            sys.modules[name] = types.ModuleType(name)
    path = os.path.join(ref_root, 'third_party', 'ext_utils', 'flowlib.py')
    spec = importlib.util.spec_from_file_location('reference_flowlib', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def cases():
    rng = np.random.default_rng(20)
    out = {}
    out['rand'] = (5. * rng.standard_normal((37, 53, 2)), None)
    f = rng.standard_normal((16, 16, 3))
    f[3, 5, 0] = 2e7                                        # unknown flow: black, not part of the maximum
    f[9, 2, 1] = -3e8
    out['unknown_c3'] = (f, None)
    out['zeros'] = (np.zeros((8, 8, 2)), None)
    out['one'] = (np.array([[[3., -4.]]]), None)
    f = 40. * rng.standard_normal((24, 24, 2))
    m = (rng.random((24, 24)) > 0.4).astype(np.float64)
    out['masked'] = (f, m)
    f = rng.standard_normal((32, 32, 2)) * np.array([300., 0.01])   # a wide, flat distribution of angles near the u axis
    out['flat'] = (f, None)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default='/root/reference')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'flowvis.npz'))
    args = ap.parse_args(argv)
    ref = load_reference(args.reference)
    blob = {}
    for name, (flow, mask) in cases().items():
        blob['in_' + name] = flow
        work = flow.copy()                                  # the reference writes into its argument
        if mask is not None:
            blob['mask_' + name] = mask
            work[mask == 0, :2] = 0.
        blob['out_' + name] = ref.flow_to_image(work)
        assert blob['out_' + name].dtype == np.uint8
    np.savez_compressed(args.out, **blob)
    print('wrote %s (%d bytes, %d cases)' % (args.out, os.path.getsize(args.out), len(cases())))


if __name__ == '__main__':
    main()
