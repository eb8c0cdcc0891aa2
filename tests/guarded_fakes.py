"""Deliberately wrong operators for the self-tests of tests/guarded.py: a wrapper module in the style of lasr_amd's (allocates
with torch.empty / torch.empty_like, launches through _lib.call) whose 'kernels' are a few torch lines.  A stray write goes at
most one element outside the tensor and only where the tensor's storage has room for it (inside a guarded buffer's band): in a
plain run, on a tensor that ends with its storage, the faulty kernel stays inside, so nothing is ever written out of bounds.
The same rule holds for the stray READS of the operators that only the relocated mode catches (RELOCATED_MODE): one element,
and only where the storage has it -- the band of the relocated copy, or the parent of a view."""
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


def overread(x):
    out = torch.empty(2, dtype=x.dtype, device=x.device)     # (the sum, and the first element)
    _lib.call('fake_sum_one_past_the_end', out, x)
    return out


def overread_view(x):
    out = torch.empty(2, dtype=x.dtype, device=x.device)     # (the sum, and the first element)
    _lib.call('fake_sum_one_past_the_end', out, x[:x.numel() - 1])      # a view: element n of the parent is a neighbour's data
    return out


def underread(x):
    out = torch.empty(2, dtype=x.dtype, device=x.device)     # (the sum, and the first element)
    _lib.call('fake_sum_one_before_the_start', out, x[1:])
    return out


def scribble_input(x):
    out = torch.empty_like(x)
    _lib.call('fake_copy_and_write_past_the_input', out, x)
    return out


def inout(x, acc):
    out = torch.empty_like(x)
    _lib.call('fake_accumulate', out, acc, x)              # acc is the caller's: incremented in place
    return out


def alias(x, k):
    out = torch.empty(x.numel() - k, dtype=x.dtype, device=x.device)
    _lib.call('fake_add', out, x, x[k:])
    return out


def raw_pointer(x):
    out = torch.empty_like(x)
    _lib.call('fake_copy_from_address', out, x, x.data_ptr() + 4)
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


def _sum_past_end(out, x):
    n = x.numel() + (1 if _room(x, False) else 0)
    out.copy_(torch.stack([x.as_strided((n,), (1,), x.storage_offset()).sum(), x[0]]))


def _sum_before_start(out, x):
    k = 1 if _room(x, True) else 0
    out.copy_(torch.stack([x.as_strided((x.numel() + k,), (1,), x.storage_offset() - k).sum(), x[0]]))


def _scribble_input(out, x):
    _copy(out, x)
    if _room(x, False):
        x.as_strided((1,), (1,), x.storage_offset() + x.numel()).fill_(1)


def _accumulate(out, acc, x):
    acc.add_(x)
    _copy(out, acc)


def _add(out, a, b):
    n = out.numel()
    out.copy_(a[:n] + b[:n])


def _copy_from_address(out, x, address):                   # (the address is only carried: nothing dereferences it)
    _copy(out, x)


KERNELS = {'fake_copy': _copy, 'fake_copy_one_past_the_end': _past_end, 'fake_copy_one_before_the_start': _before_start,
           'fake_copy_all_but_the_last': _all_but_last, 'fake_sum_one_past_the_end': _sum_past_end,
           'fake_sum_one_before_the_start': _sum_before_start, 'fake_copy_and_write_past_the_input': _scribble_input,
           'fake_accumulate': _accumulate, 'fake_add': _add, 'fake_copy_from_address': _copy_from_address}


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
    """name -> Case over the wrapper module `mod`; all but CLEAN (and 'wrong_natives', clean with a wrong declaration) are
    wrong in the way their name says."""
    def one(name, natives):
        return Case(name, lambda device: (getattr(mod, name.split('/')[0])(_input(device)),), natives)
    def inout(device):
        acc = torch.full((33,), 0.5).to(device)
        out = mod.inout(_input(device), acc)
        return out, acc                                      # (acc: what the caller holds after the call)

    return {
        'overread': one('overread', ['fake_sum_one_past_the_end']),
        'overread_view': one('overread_view', ['fake_sum_one_past_the_end']),
        'underread': one('underread', ['fake_sum_one_before_the_start']),
        'scribble_input': one('scribble_input', ['fake_copy_and_write_past_the_input']),
        'inout': Case('inout', inout, ['fake_accumulate']),
        'alias': Case('alias', lambda device: (mod.alias(_input(device), 5),), ['fake_add']),
        'raw_pointer': one('raw_pointer', ['fake_copy_from_address']),
        'clean': one('clean', ['fake_copy']),
        'overrun': one('overrun', ['fake_copy_one_past_the_end']),
        'underrun': one('underrun', ['fake_copy_one_before_the_start']),
        'short': one('short', ['fake_copy_all_but_the_last']),
        'stale': one('stale', ['fake_copy']),
        'wrong_natives': one('clean/declared wrongly', ['fake_copy', 'fake_other']),
    }


EXPECTED = {'overrun': "side': 'after'", 'underrun': "side': 'before'", 'short': 'bits differ', 'stale': 'bits differ',
            'wrong_natives': 'natives reached',
            'overread': 'bits differ', 'overread_view': 'bits differ', 'underread': 'bits differ',
            'scribble_input': "'input': 'fake_copy_and_write_past_the_input', 'arg': 1, 'side': 'after'",
            'raw_pointer': 'fake_copy_from_address: argument 2 holds the integer'}
RELOCATED_MODE = ('overread', 'overread_view', 'underread', 'scribble_input', 'raw_pointer')   # wrong, and seen only by run_relocated
CLEAN = ('clean', 'inout', 'alias')
