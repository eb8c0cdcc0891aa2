"""The raster kernel sources carry no switch between alternative implementations: the only LASR_* macros a preprocessor
conditional tests are the ablation macros, which cut a part out of the shipped kernel to time the rest (make variant, lasr_amd/csrc/
Makefile).  The switches that were settled and removed are listed in profiles/experiments/README.md, "Retired switches"."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ABLATION_MACROS = {'LASR_ABL', 'LASR_BWD_ABL', 'LASR_PW_ABL', 'LASR_OCC_LDS'}
CONDITIONAL = re.compile(r'^[ \t]*#[ \t]*(?:if|ifdef|ifndef|elif)\b(.*)$', re.M)


def conditional_macros(text):
    text = re.sub(r'\\\n', ' ', text)                 # a conditional continued over several lines
    found = set()
    for m in CONDITIONAL.finditer(text):
        found.update(re.findall(r'\bLASR_[A-Za-z0-9_]+', m.group(1).split('//')[0]))
    return found


def test_only_the_ablation_macros_switch_raster_code():
    import bench
    found = {}
    for name in bench.RASTER_SOURCES:
        if not name.endswith(('.hip', '.h')):         # the Makefile holds no code
            continue
        for macro in conditional_macros(open(os.path.join(ROOT, 'lasr_amd', 'csrc', name)).read()):
            found.setdefault(macro, []).append(name)
    assert set(found) == ABLATION_MACROS, (
        'LASR_* macros tested by #if / #ifdef / #ifndef / #elif in the raster sources: %s; expected exactly %s.  A new switch must be '
        'settled and removed in the pull request that measures it (keep the A/B under profiles/ and add a row to "Retired switches" '
        'in profiles/experiments/README.md)' % ({k: found[k] for k in sorted(found)}, sorted(ABLATION_MACROS)))


def test_the_scan_sees_every_form_of_conditional():
    text = '#ifndef LASR_A\n#define LASR_NOT_TESTED 1\n#endif\n  #  if defined(LASR_B) && \\\n   LASR_C == 2   // LASR_COMMENT\n#elif LASR_D\n#ifdef LASR_E\n'
    assert conditional_macros(text) == {'LASR_A', 'LASR_B', 'LASR_C', 'LASR_D', 'LASR_E'}
