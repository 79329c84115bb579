"""ctypes harness around a live build of the reference's own solver, simulator and accessor (oracle/build_ref.py).
Test infrastructure only; CPU only.  ``Reference(model)`` answers in the layout of ``oracle_harness`` so that the same
comparison code serves both.

The reference keeps its state in process globals and leaks on every error path, so each gateway call runs in a forked
child that sends its result back through a pipe and exits; a crash of the reference is reported, not suffered.
"""
import ctypes as C
import os
import pickle
import sys
import threading

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'oracle'))

import build_ref  # noqa: E402
from oracle_harness import OracleSolution  # noqa: E402

import mex_object  # noqa: E402
from mex_object import Host as _Host, P, SCALARS, PROPS, OPTIM  # noqa: E402,F401


class ReferenceUnavailable(Exception):
    pass


class ReferenceCrashed(Exception):
    pass


def available(model=None):
    """Is there a reference to run: its sources, or (for ``model``) libraries built earlier?"""
    if build_ref.reference_dir() is not None:
        return True
    return model is not None and build_ref.find(model) is not None


def _in_child(fn):
    """Run fn() in a forked child with its standard output discarded; return what it returns."""
    r, w = os.pipe()
    sys.stdout.flush()
    pid = os.fork()
    if pid == 0:
        code = 1
        try:
            os.close(r)
            if not os.environ.get('EGDST_REF_STDOUT'):   # the reference prints progress and diagnostics
                os.dup2(os.open(os.devnull, os.O_WRONLY), 1)
            # the gateway runs on a thread with a stack of its own: at the stress sizes the reference needs more than the
            # main thread of a test runner has left (C3 under pytest ended in SIGSEGV with 8 MB, runs with 64 MB)
            box = []
            threading.stack_size(512 << 20)
            th = threading.Thread(target=lambda: box.append(fn()))
            th.start()
            th.join()
            out = pickle.dumps(box[0], protocol=pickle.HIGHEST_PROTOCOL)
            with os.fdopen(w, 'wb') as f:
                f.write(out)
            code = 0
        except BaseException as e:   # noqa: BLE001  (the child must never return into the caller's stack)
            try:
                sys.stderr.write('ref_harness child: %r\n' % (e,))
            except Exception:
                pass
        finally:
            C.CDLL(None).fflush(None)    # the reference's printf output, when it is being kept
            os._exit(code)
    os.close(w)
    with os.fdopen(r, 'rb') as f:
        data = f.read()
    _, status = os.waitpid(pid, 0)
    if status != 0 or not data:
        raise ReferenceCrashed('the reference ended with wait status %d' % status)
    return pickle.loads(data)


class RefSim:
    """Result of a simulator call: sims [nsim x nt x nout] (None when the gateway raised), err, warnings."""

    def __init__(self, sims, err, warnings, nwarn):
        self.sims, self.err, self.warnings, self.nwarn = sims, err, warnings, nwarn


class RefCall:
    def __init__(self, res, err, warnings, nwarn):
        self.res, self.err, self.warnings, self.nwarn = res, err, warnings, nwarn


class Reference:
    def __init__(self, model, sanitize=False):
        self.model = model
        libs = build_ref.build(model, sanitize=sanitize) or build_ref.find(model, sanitize=sanitize)
        if libs is None:
            raise ReferenceUnavailable('no reference sources (EGDST_REFERENCE_DIR) and no libraries under oracle/_ref/')
        self.libs = libs
        self.sanitize = sanitize

    # ------------------------------------------------------------------ the Model object
    def _model(self, h, params=None, sol=None, init=None, randstream=None):
        """tests/mex_object.py: the same properties, built by the same code, as the shims get (tests/shim_harness.py)."""
        return mex_object.build_object(h, mex_object.properties(self.model, params, sol, init, randstream))

    # ------------------------------------------------------------------ gateways
    def solve(self, params=None, dbgout=False):
        """The solver gateway.  An ``OracleSolution`` with ``err`` (the gateway's error text or the solver's own ``err``),
        ``rc`` (0 clean), ``warnings``; with dbgout=True also ``dbgout`` [cap x 7] and ``dbgn``."""
        m = self.model
        d = m.descriptor()
        nt, nst = d['T'] - d['t0'] + 1, m.nst

        def work():
            h = _Host(self.libs['ref_solver.so'])
            rc, out, msg, warn, nwarn = h.run(3, [self._model(h, params)])
            res = {'gate': rc, 'msg': msg, 'warn': warn, 'nwarn': nwarn, 'M': {}, 'D': {}}
            if rc == 0:
                res['err'] = C.string_at(C.addressof((C.c_char * 300).in_dll(h.lib, 'err'))).decode(errors='replace')
                for i in range(nt * nst):
                    cm, cd = h.lib.mxGetCell(out[0], i), h.lib.mxGetCell(out[1], i)
                    if cm:
                        res['M'][i] = h.array(cm)
                    if cd:
                        res['D'][i] = h.array(cd)
                if dbgout:
                    res['dbgout'] = h.array(out[2])
                    res['dbgn'] = int(C.c_int.in_dll(h.lib, 'dbgouti').value)
            return res

        res = _in_child(work)
        sol = OracleSolution(nt, nst, d['ngridmax'], d['nthrhmax'])
        sol.warnings, sol.nwarn = res['warn'], res['nwarn']
        sol.err = res['msg'] if res['gate'] else res['err']
        sol.rc = 1 if sol.err else 0
        for i, a in res['M'].items():
            it, ist = divmod(i, nst)
            n = a.shape[0]
            sol.len[it, ist] = n
            sol.M[it, ist, :n], sol.C[it, ist, :n], sol.V[it, ist, :n] = a[:, 0], a[:, 1], a[:, 3]
            sol.__dict__.setdefault('A', {})[(it, ist)] = a[:, 2]
        for i, a in res['D'].items():
            it, ist = divmod(i, nst)
            n = a.shape[0]
            sol.thlen[it, ist] = n
            sol.D[it, ist, :n], sol.TH[it, ist, :n] = a[:, 0], a[:, 1]
        if dbgout and 'dbgout' in res:
            sol.dbgout, sol.dbgn = np.asfortranarray(res['dbgout']), res['dbgn']
        return sol

    def sim(self, sol, init, randstream, rndtype=0, params=None):
        d = self.model.descriptor()
        nt = d['T'] - d['t0'] + 1
        init = np.atleast_2d(np.asarray(init, dtype=np.float64))

        def work():
            h = _Host(self.libs['ref_simulator.so'])
            obj = self._model(h, params, sol=sol, init=init, randstream=randstream)
            rc, out, msg, warn, nwarn = h.run(1, [obj, h.lib.mxCreateDoubleScalar(float(rndtype))])
            sims = None
            if rc == 0:
                n = h.lib.mxGetNumberOfElements(out[0])
                flat = np.ctypeslib.as_array(h.lib.mxGetPr(out[0]), shape=(n,)).copy()
                sims = flat.reshape(init.shape[0], nt, -1)   # column-major [nout x nt x nsim]
            return sims, msg, warn, nwarn

        return RefSim(*_in_child(work))

    def call(self, sol, sw, args, params=None):
        a = np.atleast_2d(np.asarray(args, dtype=np.float64))

        def work():
            h = _Host(self.libs['ref_call.so'])
            obj = self._model(h, params, sol=sol)
            rc, out, msg, warn, nwarn = h.run(1, [obj, h.lib.mxCreateDoubleScalar(float(sw)), h.double(a)])
            res = h.array(out[0]).reshape(-1) if rc == 0 and out[0] else None
            return res, msg, warn, nwarn

        return RefCall(*_in_child(work))
