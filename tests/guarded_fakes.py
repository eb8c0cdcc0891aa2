"""Deliberately wrong operators for the self-tests of tests/guarded.py: a wrapper module in the style of lasr_amd's (allocates
with torch.empty / torch.empty_like, launches through _lib.call) whose 'kernels' are a few torch lines.  A stray write goes at
most one element outside the tensor and only where the tensor's storage has room for it (inside a guarded buffer's band): in a
plain run, on a tensor that ends with its storage, the faulty kernel stays inside, so nothing is ever written out of bounds."""
import types

import torch

from guarded import Case

WRAPPER_SOURCE = '''
import torch


def clean(x):
    out = torch.empty_like(x)
    _lib.call('fake_copy', out, x)
    return out


def overrun(x):
    out = torch.empty(x.numel(), dtype=x.dtype, device=x.device)
    _lib.call('fake_copy_one_past_the_end', out, x)
    return out


def underrun(x):
    out = torch.empty(x.numel(), dtype=x.dtype, device=x.device)
    _lib.call('fake_copy_one_before_the_start', out, x)
    return out


def short(x):
    out = torch.empty_like(x)
    _lib.call('fake_copy_all_but_the_last', out, x)
    return out


def stale(x):
    n = x.numel()
    scratch = torch.empty(n + 1, dtype=x.dtype, device=x.device)
    out = torch.empty(n, dtype=x.dtype, device=x.device)
    _lib.call('fake_copy', scratch[:n], x)                 # slot n of the scratch is never written ...
    _lib.call('fake_copy', out, scratch[1:])               # ... and read here
    return out
'''


def _room(t, before):
    s = t.untyped_storage().nbytes()
    if before:
        return t.storage_offset() >= 1
    return (t.storage_offset() + t.numel() + 1) * t.element_size() <= s


def _copy(out, x):
    out.copy_(x.reshape(out.shape))


def _past_end(out, x):
    _copy(out, x)
    if _room(out, False):
        out.as_strided((1,), (1,), out.storage_offset() + out.numel()).fill_(1)


def _before_start(out, x):
    _copy(out, x)
    if _room(out, True):
        out.as_strided((1,), (1,), out.storage_offset() - 1).fill_(1)


def _all_but_last(out, x):
    out.reshape(-1)[:-1].copy_(x.reshape(-1)[:-1])


KERNELS = {'fake_copy': _copy, 'fake_copy_one_past_the_end': _past_end, 'fake_copy_one_before_the_start': _before_start,
           'fake_copy_all_but_the_last': _all_but_last}


def make():
    """(wrapper module, its _lib): fresh objects, so that a test can look at their globals afterwards."""
    lib = types.SimpleNamespace()
    lib.call = lambda name, *args: KERNELS[name](*args)
    mod = types.ModuleType('fake_wrappers')
    mod._lib = lib
    exec(WRAPPER_SOURCE, mod.__dict__)
    return mod, lib


def _input(device):
    g = torch.Generator().manual_seed(7)
    return torch.rand(33, generator=g).to(device)


def cases(mod):
    """name -> Case over the wrapper module `mod`; all but 'clean' (and 'wrong_natives', clean with a wrong declaration) are
    wrong in the way their name says."""
    def one(name, natives):
        return Case(name, lambda device: (getattr(mod, name.split('/')[0])(_input(device)),), natives)
    return {
        'clean': one('clean', ['fake_copy']),
        'overrun': one('overrun', ['fake_copy_one_past_the_end']),
        'underrun': one('underrun', ['fake_copy_one_before_the_start']),
        'short': one('short', ['fake_copy_all_but_the_last']),
        'stale': one('stale', ['fake_copy']),
        'wrong_natives': one('clean/declared wrongly', ['fake_copy', 'fake_other']),
    }


EXPECTED = {'overrun': "side': 'after'", 'underrun': "side': 'before'", 'short': 'bits differ', 'stale': 'bits differ',
            'wrong_natives': 'natives reached'}
