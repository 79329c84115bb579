"""Build the reference's own solver, simulator and accessor for one model (TEST INFRASTRUCTURE).

    python oracle/build_ref.py <name in egdst_amd.examples.REGISTRY>

Each of the reference's three gateway sources defines ``mexFunction``, so each becomes a library of its own under
``oracle/_ref/<tag>/``: ``ref_solver.so``, ``ref_simulator.so``, ``ref_call.so`` = gateway source + the reference's common
routines (both read in place from the reference directory) + the generated ``modelspec.c`` (oracle/ref_modelspec.py) + the
MEX host (oracle/mexhost/).  Nothing of this is committed; ``oracle/_ref/`` is ignored.

Flags are what ``mex`` hands its compiler on Linux, as far as arithmetic goes: ``-O2 -fPIC``, no ``-march``, no
``-ffast-math``, contraction off: plain IEEE double with the platform libm.  ``-Wl,-Bsymbolic`` makes each library bind its
own global names (one of them, ``error``, is also a glibc function).

One flag more is needed for the reference to have an answer at all.  Its solver reads three locals of its per-cell routine
before anything has been stored in them (``evf``, ``c1``, ``pr1pre``; ``-Wmaybe-uninitialized`` names them): the first
savings guess of every cell tests ``evf==-INFINITY`` on an indeterminate value.  Under gcc 11 -O2 that value happens to
be -inf, and every model stops in its first non-terminal period with "Failed to find any value of savings ...".  The C
standard leaves such a read undefined, so the build pins it: ``-ftrivial-auto-var-init=zero`` gives every automatic
variable the value zero at its declaration and changes nothing else.  gcc has that flag from version 12 on; where the
system gcc is older, the clang of the ROCm toolchain (which the project needs anyway) compiles these host libraries.

The reference directory is ``$EGDST_REFERENCE_DIR`` (default ``/root/reference``).  Where it is absent, nothing is built
and ``build()`` returns None; libraries built earlier stay usable (``find()``).
"""
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import ref_modelspec  # noqa: E402

GATEWAYS = {'ref_solver.so': 'egdst_solver.c', 'ref_simulator.so': 'egdst_simulator.c', 'ref_call.so': 'egdst_call.c'}
COMMON = 'egdst_lib.c'
SUBDIR = '@egdstmodel'
OUT = os.path.join(HERE, '_ref')
HOST = os.path.join(HERE, 'mexhost')
PIN = '-ftrivial-auto-var-init=zero'
SANITIZE = ['-fsanitize=address,undefined', '-fsanitize-recover=address', '-fno-omit-frame-pointer', '-O1', '-g']


def reference_dir():
    """Directory holding the reference's C sources, or None."""
    d = os.environ.get('EGDST_REFERENCE_DIR', '/root/reference')
    for cand in (os.path.join(d, SUBDIR), d):
        if all(os.path.exists(os.path.join(cand, f)) for f in list(GATEWAYS.values()) + [COMMON, 'egdst_lib.h']):
            return cand
    return None


_CC = []


def compiler():
    """A C compiler that knows the pinning flag: gcc >= 12, else clang (PATH, then the ROCm toolchain); None if there is none."""
    if _CC:
        return _CC[0]
    rocm = os.environ.get('ROCM_PATH', '/opt/rocm')
    for cc in ('gcc', 'clang', os.path.join(rocm, 'llvm', 'bin', 'clang'), os.path.join(rocm, 'lib', 'llvm', 'bin', 'clang')):
        exe = shutil.which(cc)
        if exe and subprocess.run([exe, PIN, '-x', 'c', '-fsyntax-only', os.devnull], capture_output=True).returncode == 0:
            _CC.append(exe)
            return exe
    _CC.append(None)
    return None


def model_dir(model, sanitize=False):
    return os.path.join(OUT, ref_modelspec.tag(model) + ('_san' if sanitize else ''))


def find(model, sanitize=False):
    """{library name: path} of a finished build for this model, or None."""
    d = model_dir(model, sanitize)
    libs = {k: os.path.join(d, k) for k in GATEWAYS}
    return libs if all(os.path.exists(p) for p in libs.values()) else None


def _write_if_changed(path, text):
    if not os.path.exists(path) or open(path).read() != text:
        with open(path, 'w') as f:
            f.write(text)


def build(model, sanitize=False, quiet=True):   # sanitize: see build_sanitized()
    """Write the modelspec and build the three libraries; returns {name: path}, or None without a reference directory."""
    ref = reference_dir()
    if ref is None:
        if not quiet:
            print('build_ref: no reference sources under %s; nothing built' % os.environ.get('EGDST_REFERENCE_DIR', '/root/reference'))
        return None
    cc = compiler()
    if cc is None:
        if not quiet:
            print('build_ref: no C compiler with %s (gcc >= 12 or clang); nothing built' % PIN)
        return None
    d = model_dir(model, sanitize)
    os.makedirs(d, exist_ok=True)
    hdr, src = ref_modelspec.generate(model)
    _write_if_changed(os.path.join(d, 'modelspec.h'), hdr)
    _write_if_changed(os.path.join(d, 'modelspec.c'), src)
    host = [os.path.join(HOST, f) for f in ('mexhost.c', 'mex.h', 'matrix.h')]
    libs = {}
    for lib, gate in GATEWAYS.items():
        out = os.path.join(d, lib)
        deps = [os.path.join(ref, gate), os.path.join(ref, COMMON), os.path.join(ref, 'egdst_lib.h'),
                os.path.join(d, 'modelspec.c'), os.path.join(d, 'modelspec.h')] + host
        libs[lib] = out
        if os.path.exists(out) and os.path.getmtime(out) >= max(os.path.getmtime(p) for p in deps):
            continue
        tmp = out + '.tmp.%d' % os.getpid()
        cmd = [cc] + (SANITIZE if sanitize else ['-O2']) + [PIN, '-ffp-contract=off', '-fPIC', '-shared', '-w', '-Wl,-Bsymbolic', '-I', d,
               '-I', HOST, '-I', ref] + ref_modelspec.defines(model) + [os.path.join(ref, gate), os.path.join(ref, COMMON),
               os.path.join(d, 'modelspec.c'), host[0], '-o', tmp, '-lm']
        subprocess.run(cmd, check=True)
        os.replace(tmp, out)
    return libs


def build_sanitized(model, quiet=True):
    """The three gateways as stand-alone programs under AddressSanitizer and UBSan (oracle/mexhost/ref_main.c); host code,
    CPU only.  Returns {library name: path of the program}, or None."""
    ref, cc = reference_dir(), compiler()
    if ref is None or cc is None:
        return None
    d = model_dir(model, sanitize=True)
    os.makedirs(d, exist_ok=True)
    hdr, src = ref_modelspec.generate(model)
    _write_if_changed(os.path.join(d, 'modelspec.h'), hdr)
    _write_if_changed(os.path.join(d, 'modelspec.c'), src)
    progs = {}
    for lib, gate in GATEWAYS.items():
        out = os.path.join(d, lib.replace('.so', '_san'))
        progs[lib] = out
        if os.path.exists(out) and os.path.getmtime(out) >= max(os.path.getmtime(os.path.join(HOST, f)) for f in os.listdir(HOST)):
            continue
        subprocess.run([cc] + SANITIZE + [PIN, '-ffp-contract=off', '-w', '-I', d, '-I', HOST, '-I', ref] + ref_modelspec.defines(model) +
                       [os.path.join(ref, gate), os.path.join(ref, COMMON), os.path.join(d, 'modelspec.c'),
                        os.path.join(HOST, 'mexhost.c'), os.path.join(HOST, 'ref_main.c'), '-o', out, '-lm'], check=True)
    return progs


if __name__ == '__main__':
    from egdst_amd import examples
    print(build(examples.REGISTRY[sys.argv[1]](), sanitize='--sanitize' in sys.argv, quiet=False))
