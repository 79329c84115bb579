"""Build and drive the real MEX shims (shims/*.c) on the runnable MEX host of oracle/mexhost/ (TEST INFRASTRUCTURE).

Build: next to a model library, ``shim_solver.so``, ``shim_simulator.so`` and ``shim_call.so`` = the shim source + the MEX
host, linked to that library (``libegdst.so`` on the GPU, a tests/cpu_emu build on the CPU) by name with an $ORIGIN rpath.

Run: a gateway call loads the model library and with it HIP, so it never runs in the test process nor in a fork of it:

    results = run(shims, props, calls)          # parent: one fresh child, one model, a list of gateway calls

starts ``python shim_harness.py request.npz result.npz``; that child imports numpy and ctypes only, builds the model object
(tests/mex_object.py) and calls ``ref_run`` like tests/ref_harness.py does for the reference's gateways.  One child at a
time; a child that ends by a signal or runs out of time raises ``ShimChildDied`` and no further child is started.

A call is a dict: ``gw`` 'solver' | 'simulator' | 'call'; ``nlhs``; ``cells`` 'props' (M and D of ``props``, default),
'solver' (the cell arrays the last solver call of this child returned, handed on as mxArrays: the MATLAB way) or 'none';
``drop`` names of properties to leave out; ``set`` {property: array} to replace; ``rhs`` the arguments after the model
(default: rndtype for the simulator, [sw, args] for the accessor); ``nrhs`` to cut the argument list short.
Device-memory probes for the GPU tests: {'op': 'meminfo'} and {'op': 'footprint'}.
"""
import ctypes as C
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GATEWAYS = ('solver', 'simulator', 'call')
HOST = os.path.join(ROOT, 'oracle', 'mexhost')
STREAM_PER_THREAD = 2     # include/egdst.h: EGDST_STREAM_PER_THREAD (tests/test_abi.py holds it to the header)


class ShimChildDied(Exception):
    pass


# ---------------------------------------------------------------------------------------------------------------- build
def compiler():
    """gcc, else clang, else the ROCm clang (the order of oracle/build_ref.py: compiler(), without its pinning flag)."""
    rocm = os.environ.get('ROCM_PATH', '/opt/rocm')
    for cc in ('gcc', 'clang', os.path.join(rocm, 'llvm', 'bin', 'clang'), os.path.join(rocm, 'lib', 'llvm', 'bin', 'clang')):
        exe = shutil.which(cc)
        if exe:
            return exe
    raise RuntimeError('no C compiler for the shims')


def build(library):
    """The three shim libraries next to ``library``; {gateway: path}.  Rebuilt only when a source is newer."""
    d, name = os.path.dirname(os.path.abspath(library)), os.path.basename(library)
    suffix = '' if name == 'libegdst.so' else '_' + name[len('libegdst_'):-len('.so')]
    host = [os.path.join(HOST, f) for f in ('mexhost.c', 'mex.h', 'matrix.h')]
    common = [os.path.join(ROOT, 'shims', 'egdst_shim_common.h'), os.path.join(ROOT, 'include', 'egdst.h')] + host
    out = {}
    for gw in GATEWAYS:
        src = os.path.join(ROOT, 'shims', 'egdst_%s_hip.c' % gw)
        so = out[gw] = os.path.join(d, 'shim_%s%s.so' % (gw, suffix))
        if os.path.exists(so) and os.path.getmtime(so) >= max(os.path.getmtime(p) for p in [src, library] + common):
            continue
        cc, inc = compiler(), ['-I', os.path.join(ROOT, 'include'), '-I', os.path.join(ROOT, 'shims'), '-I', HOST]
        flags = ['-O1', '-g', '-fPIC']
        objs = [so + '.%s.%d.o' % (k, os.getpid()) for k in ('shim', 'host')]
        tmp = so + '.tmp.%d' % os.getpid()
        try:
            subprocess.run([cc] + flags + ['-Wall', '-Wextra', '-Werror'] + inc + ['-c', src, '-o', objs[0]], check=True)
            subprocess.run([cc] + flags + inc + ['-c', host[0], '-o', objs[1]], check=True)
            subprocess.run([cc] + flags + ['-shared'] + objs + ['-L', d, '-l:' + name, '-Wl,-rpath,$ORIGIN', '-o', tmp, '-lm'], check=True)
            os.replace(tmp, so)
        finally:
            for o in objs:
                if os.path.exists(o):
                    os.remove(o)
    return out


def build_for_model(model):
    """The shims for the GPU library of ``model`` (egdst_amd/_models/<tag>/libegdst.so, built if absent)."""
    sys.path.insert(0, ROOT)
    from egdst_amd import build as b
    return build(b.build_model(model).path)


def find_for_model(model):
    """The shims built earlier for the GPU library of ``model``; compiles nothing."""
    sys.path.insert(0, ROOT)
    from egdst_amd import build as b, codegen
    d = os.path.join(b.MODELS_DIR, b.model_tag(model, codegen.generate_modelspec(model)))
    out = {gw: os.path.join(d, 'shim_%s.so' % gw) for gw in GATEWAYS}
    missing = [p for p in list(out.values()) + [os.path.join(d, 'libegdst.so')] if not os.path.exists(p)]
    if missing:
        raise RuntimeError('not built (run __graft_entry__.build()): %s' % missing)
    return out


def build_emu_for_model(model):
    """The shims over the CPU harness build of the model's device code (tests/cpu_emu)."""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(HERE, 'cpu_emu'))
    import build_emu
    from egdst_amd import build as b, codegen
    text = codegen.generate_modelspec(model)
    d = os.path.join(b.MODELS_DIR, b.model_tag(model, text))
    os.makedirs(d, exist_ok=True)
    spec = os.path.join(d, 'modelspec.h')
    if not os.path.exists(spec) or open(spec).read() != text:
        with open(spec, 'w') as f:
            f.write(text)
    return build(build_emu.build(d, False, 1, False, 1))


# --------------------------------------------------------------------------------------------------------------- parent
_dead = []


def _pack(props, calls):
    arrays, plain = {}, {}
    for k, v in props.items():
        if k in ('M', 'D'):
            arrays['p_%s_len' % k] = np.array([0 if a is None else np.shape(a)[0] for a in v], dtype=np.int64)
            arrays['p_%s_ncol' % k] = np.array([0 if a is None else np.shape(a)[1] for a in v], dtype=np.int64)
            arrays['p_%s_rows' % k] = np.concatenate([np.asarray(a, dtype=float).reshape(-1) for a in v if a is not None] + [np.zeros(0)])
        elif k == 's':
            plain['s'] = [bool(dv) for dv, _ in v]
            for i, (_, grid) in enumerate(v):
                arrays['p_s%d' % i] = np.asarray(grid, dtype=float)
        elif isinstance(v, np.ndarray):
            arrays['p_' + k] = v
        else:
            plain[k] = v
    cs = []
    for i, c in enumerate(calls):
        c = dict(c)
        for key in ('set', 'rhs'):
            if key in c:
                items = c[key].items() if key == 'set' else enumerate(c[key])
                names = []
                for name, a in items:
                    arrays['c%d_%s_%s' % (i, key, name)] = np.asarray(a, dtype=float)
                    names.append(str(name))
                c[key] = names
        cs.append(c)
    arrays['json'] = np.array(json.dumps({'plain': plain, 'calls': cs}))
    return arrays


def run(shims, props, calls, timeout=60):
    """One child for one model: ``calls`` in order; a list of result dicts (rc, err, warn, nwarn, secs and the outputs)."""
    if _dead:
        raise ShimChildDied('an earlier shim child %s; no further child is started' % _dead[0])
    with tempfile.TemporaryDirectory() as tmp:
        req, res = os.path.join(tmp, 'request.npz'), os.path.join(tmp, 'result.npz')
        arrays = _pack(props, calls)
        arrays['shims'] = np.array(json.dumps(shims))
        np.savez(req, **arrays)
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), req, res], timeout=timeout, capture_output=True,
                               text=True)
        except subprocess.TimeoutExpired:
            _dead.append('ran out of its %d s' % timeout)
            raise ShimChildDied('the shim child ran out of its %d s' % timeout)
        if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
            _dead.append('ended with status %d' % r.returncode)
            raise ShimChildDied('the shim child ended with status %d\n%s' % (r.returncode, r.stderr[-3000:]))
        assert r.returncode == 0, 'shim child: exit %d\n%s\n%s' % (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
        with np.load(res) as z:
            n = int(z['ncalls'])
            out = [{} for _ in range(n)]
            for k in z.files:
                if k.startswith('r'):
                    i, name = k[1:].split('_', 1)
                    a = z[k]
                    out[int(i)][name] = a.item() if a.ndim == 0 else a
        for o in out:
            o['stderr'] = r.stderr
        return out


# ---------------------------------------------------------------------------------------------------------------- child
class _Desc(C.Structure):     # include/egdst.h: egdst_desc
    _fields_ = [('t0', C.c_int), ('T', C.c_int), ('ngridm', C.c_int), ('ngridmax', C.c_int), ('nthrhmax', C.c_int),
                ('ny', C.c_int), ('mmax', C.c_double), ('a0', C.c_double), ('quadrature', C.POINTER(C.c_double))]


def _mem_in_use(libpath):
    """Device memory in use on the current device, bytes, from the HIP runtime this process has already loaded (found through
    the model library that depends on it)."""
    hip = C.CDLL(libpath)
    free, total = C.c_size_t(), C.c_size_t()
    rc = hip.hipMemGetInfo(C.byref(free), C.byref(total))
    assert rc == 0, 'hipMemGetInfo: %d' % rc
    return total.value - free.value


def _footprint(libpath, p):
    """In-use device memory with one live handle, made as shim_handle() of shims/egdst_shim_common.h makes it (one draw,
    history kept, EGDST_STREAM_PER_THREAD), minus without."""
    lib = C.CDLL(libpath)
    q = np.ascontiguousarray(np.asarray(p['quadrature'], dtype=float).T.reshape(-1))
    d = _Desc(int(p['t0']), int(p['T']), int(p['ngridm']), int(p['ngridmax']), int(p['nthrhmax']), int(p['ny']),
              float(p['mmax']), float(p['a0']), q.ctypes.data_as(C.POINTER(C.c_double)))
    h = C.c_void_p()
    before = _mem_in_use(libpath)
    rc = lib.egdst_create(C.byref(d), 1, 1, C.c_void_p(STREAM_PER_THREAD), C.byref(h))
    assert rc == 0, 'egdst_create: %d' % rc
    live = _mem_in_use(libpath)
    lib.egdst_destroy.argtypes = [C.c_void_p]
    lib.egdst_destroy(h)
    return live - before, _mem_in_use(libpath) - before


def _child(req, res):
    sys.path.insert(0, HERE)
    import mex_object
    z = np.load(req)
    meta = json.loads(str(z['json']))
    shims = json.loads(str(z['shims']))
    props = dict(meta['plain'])
    for k in z.files:
        if k.startswith('p_') and not re.match(r'p_([MD]_(len|ncol|rows)|s[0-9]+)$', k):
            props[k[2:]] = z[k]
    if 's' in props:
        props['s'] = [(dv, z['p_s%d' % i]) for i, dv in enumerate(props['s'])]
    for k in ('M', 'D'):
        if 'p_%s_len' % k in z.files:
            lens, ncol, rows = z['p_%s_len' % k], z['p_%s_ncol' % k], z['p_%s_rows' % k]
            offs = np.concatenate([[0], np.cumsum(lens * ncol)])
            props[k] = [rows[offs[i]:offs[i + 1]].reshape(lens[i], ncol[i]) if lens[i] else None for i in range(len(lens))]
    hosts, out, solved = {}, {'ncalls': np.int64(len(meta['calls']))}, None
    nt, nst = int(props['T']) - int(props['t0']) + 1, int(props['nst'])
    for i, c in enumerate(meta['calls']):
        put = lambda name, v: out.__setitem__('r%d_%s' % (i, name), np.asarray(v))   # noqa: E731
        libpath = os.path.join(os.path.dirname(shims['solver']), 'libegdst.so')
        if c.get('op') == 'meminfo':
            put('in_use', _mem_in_use(libpath))
            continue
        if c.get('op') == 'footprint':
            live, left = _footprint(libpath, props)
            put('footprint', live)
            put('left', left)
            continue
        gw = c['gw']
        h = hosts.get(gw) or hosts.setdefault(gw, mex_object.Host(shims[gw]))
        p = {k: v for k, v in props.items() if k not in c.get('drop', [])}
        for name in c.get('set', []):
            p[name] = z['c%d_set_%s' % (i, name)]
        cells = c.get('cells', 'props')
        M = D = None
        if cells == 'none':
            p.pop('M', None), p.pop('D', None)
        elif cells == 'solver':
            # the solver's outputs live in the solver library's host; every host has the same array layout, and the object
            # only holds pointers, so they are handed on as they are: what egdstmodel.solve stores and egdstmodel.sim reads
            M, D = solved
        obj = mex_object.build_object(h, p, M=M, D=D)
        rhs = [z['c%d_rhs_%s' % (i, name)] for name in c.get('rhs', [])]
        prhs = [obj] + [h.double(a) for a in rhs]
        if 'nrhs' in c:
            prhs = (prhs + [h.double(0.0)] * c['nrhs'])[:c['nrhs']]
        nlhs = int(c.get('nlhs', 3 if gw == 'solver' else 1))
        t = time.perf_counter()
        rc, lhs, msg, warn, nwarn = h.run(nlhs, prhs)
        put('secs', time.perf_counter() - t)
        put('rc', rc), put('err', msg), put('warn', warn), put('nwarn', nwarn)
        if rc != 0:
            continue
        if gw == 'solver' and nlhs == 3:
            solved = (lhs[0], lhs[1])
            ln, th, mrows, drows, ncols = np.zeros((nt, nst), np.int64), np.zeros((nt, nst), np.int64), [], [], []
            for it in range(nt):
                for ist in range(nst):
                    cm, cd = h.lib.mxGetCell(lhs[0], ist + it * nst), h.lib.mxGetCell(lhs[1], ist + it * nst)
                    if cm:
                        a = h.array(cm)
                        ln[it, ist] = a.shape[0]
                        ncols.append(a.shape[1])
                        mrows.append(a)
                    if cd:
                        a = h.array(cd)
                        th[it, ist] = a.shape[0]
                        drows.append(a)
            put('len', ln), put('thlen', th)
            put('ncells', h.lib.mxGetNumberOfElements(lhs[0]))
            put('mcav', np.concatenate(mrows) if mrows and set(ncols) == {4} else np.zeros((0, 4)))
            put('dth', np.concatenate(drows) if drows else np.zeros((0, 2)))
            put('dbgout', h.array(lhs[2]))
        elif gw == 'simulator' and lhs[0]:
            n = h.lib.mxGetNumberOfElements(lhs[0])
            flat = np.ctypeslib.as_array(h.lib.mxGetPr(lhs[0]), shape=(n,)).copy() if n else np.zeros(0)
            nsim = len(p['init']) if 'init' in p else 0
            put('sims', flat.reshape(nsim, nt, -1) if nsim else flat)   # column-major [nout x nt x nsim]
        elif gw == 'call' and lhs[0]:
            put('res', h.array(lhs[0]).reshape(-1))
    np.savez(res, **out)


if __name__ == '__main__':
    _child(sys.argv[1], sys.argv[2])
