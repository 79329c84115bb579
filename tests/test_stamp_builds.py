"""Every clock-stamp set (-DEGDST_STAMPS=<set>, egdst_device.h) still compiles: the compiler front end, host and device pass,
over egdst_kernels.hip for a model with several choices and for one with a single choice (k_env1 instead of the envelope
kernels), with each set and with none.  Nothing is run; the diagnostic builds have no other user in the suite."""
import os
import subprocess

import pytest

from egdst_amd import build, codegen, examples

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETS = [None, 'env', 'walk', 'seg', 'sort', 'wg', 'tpsort', 'tpwalk']
MODELS = {'retirement1': examples.retirement1, 'deaton1': examples.deaton1}


def test_the_sets_are_the_ones_the_device_header_names():
    hdr = open(os.path.join(build.CSRC, 'egdst_device.h')).read()
    line = next(ln for ln in hdr.splitlines() if ln.startswith('enum { EG_STAMPSET_'))
    named = [w.split('=')[0].strip()[len('EG_STAMPSET_'):] for w in line[line.index('{') + 1:line.index('}')].split(',')]
    assert named == SETS[1:]


@pytest.mark.parametrize('stamps', SETS, ids=[s or 'none' for s in SETS])
@pytest.mark.parametrize('name', sorted(MODELS))
def test_kernel_source_compiles_with_the_stamp_set(name, stamps, tmp_path):
    model = MODELS[name]()
    assert (model.nd > 1) == (name == 'retirement1')
    (tmp_path / 'modelspec.h').write_text(codegen.generate_modelspec(model))
    cmd = [build._hipcc()] + [f for f in build.HIPCC_FLAGS if f not in ('-shared', '-fPIC')] + ['-fsyntax-only']
    cmd += ['-DEGDST_STAMPS=' + stamps] if stamps else []
    cmd += ['-I', str(tmp_path), '-I', build.CSRC, '-I', os.path.join(ROOT, 'include'), os.path.join(build.CSRC, 'egdst_kernels.hip')]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_stamp_build_on_the_cpu_harness_computes_the_same_bits():
    """tests/cpu_emu/run_emu_stamps.py: the harness build with -DEGDST_STAMPS=wg against the plain harness build, no sanitizer"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tests', 'cpu_emu'))
    import estimation_emu as emu
    out = emu.run_runner('run_emu_stamps.py', '', 'stamp build problems: 0')
    assert "'wg.resident': " in out, out
