"""Every operator of tests/guarded_cases.py with guard-banded, poisoned outputs and scratch (tests/guarded.py): nothing is written
outside an allocation, no result depends on what memory held before the call, and the natives reached are the declared ones.
The deliberately wrong operators of tests/guarded_fakes.py run on the device too; their stray writes stay inside the guarded
buffer's own bands."""
import pytest

import guarded
import guarded_cases
import guarded_fakes

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('case', guarded_cases.CASES, ids=[c.name for c in guarded_cases.CASES])
def test_operator_under_guard_bands_and_two_poisons(cuda, case):
    guarded.run_case(case, cuda)


def _fake(cuda, name):
    mod, lib = guarded_fakes.make()
    guarded.run_case(guarded_fakes.cases(mod)[name], cuda, modules=[mod], lib=lib)


def test_a_clean_fake_operator_passes_on_the_device(cuda):
    _fake(cuda, 'clean')


@pytest.mark.parametrize('name', sorted(guarded_fakes.EXPECTED))
def test_a_wrong_fake_operator_is_caught_on_the_device(cuda, name):
    with pytest.raises(AssertionError) as e:
        _fake(cuda, name)
    assert guarded_fakes.EXPECTED[name] in str(e.value), str(e.value)
