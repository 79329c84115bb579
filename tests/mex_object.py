"""The model object the reference's MATLAB host hands a gateway, for the runnable MEX host of oracle/mexhost/ (TEST
INFRASTRUCTURE).  Two steps, so that a process which must stay small can take the second alone:

    properties(model, ...)      plain numbers and arrays: what the object's properties hold      (needs the model)
    build_object(host, props)   the mxArray struct a gateway reads through mxGetProperty         (numpy and ctypes only)

tests/ref_harness.py (the reference's own gateways) and tests/shim_harness.py (the project's shims) both go through these
two functions: the reference and the shim receive the same properties from the same code.
"""
import ctypes as C

import numpy as np

P = C.c_void_p
SCALARS = ('t0', 'T', 'ngridm', 'ngridmax', 'nthrhmax', 'ny', 'nd', 'nnd', 'nst', 'nnst', 'mmax', 'a0')
PROPS = SCALARS + ('stm', 'states', 'decisions', 'optim', 'quadrature', 'param', 's', 'eq', 'init', 'randstream', 'M', 'D')
OPTIM = ('optim_UasD', 'optim_MUnoD', 'optim_UnoD', 'optim_TRPRnoSH')


class Host:
    """A library that holds a gateway and the MEX host, with the Matrix API typed for ctypes."""

    def __init__(self, path):
        lib = self.lib = C.CDLL(path)
        sz = C.c_size_t
        for name, res, args in (
                ('mxCreateDoubleMatrix', P, [sz, sz, C.c_int]), ('mxCreateDoubleScalar', P, [C.c_double]),
                ('mxCreateNumericArray', P, [sz, C.POINTER(sz), C.c_int, C.c_int]),
                ('mxCreateCellMatrix', P, [sz, sz]), ('mxCreateStructMatrix', P, [sz, sz, C.c_int, C.POINTER(C.c_char_p)]),
                ('mxCreateLogicalScalar', P, [C.c_bool]), ('mxGetPr', C.POINTER(C.c_double), [P]), ('mxGetM', sz, [P]),
                ('mxGetN', sz, [P]), ('mxGetNumberOfElements', sz, [P]), ('mxGetCell', P, [P, sz]),
                ('mxSetCell', None, [P, sz, P]), ('mxSetField', None, [P, sz, C.c_char_p, P]),
                ('ref_run', C.c_int, [C.c_int, C.POINTER(P), C.c_int, C.POINTER(P), C.c_char_p, sz]),
                ('ref_warnings', C.c_char_p, []), ('ref_warning_count', sz, []), ('ref_reset_warnings', None, [])):
            f = getattr(lib, name)
            f.restype, f.argtypes = res, args

    def double(self, a):
        a = np.asarray(a, dtype=np.float64)
        if a.ndim == 0:
            a = a.reshape(1, 1)
        elif a.ndim == 1:
            a = a.reshape(-1, 1)
        mx = self.lib.mxCreateDoubleMatrix(a.shape[0], a.shape[1], 0)
        if a.size:
            flat = np.asfortranarray(a).reshape(-1, order='F')
            C.memmove(self.lib.mxGetPr(mx), flat.ctypes.data, flat.nbytes)
        return mx

    def struct(self, n, fields):
        names = (C.c_char_p * len(fields))(*[f.encode() for f in fields])
        return self.lib.mxCreateStructMatrix(1, n, len(fields), names)

    def array(self, mx):
        """Copy of a real double matrix as [rows x cols]."""
        m, n = self.lib.mxGetM(mx), self.lib.mxGetN(mx)
        if m * n == 0:
            return np.zeros((m, n))
        return np.ctypeslib.as_array(self.lib.mxGetPr(mx), shape=(m * n,)).copy().reshape((m, n), order='F')

    def cells(self, arrays):
        mx = self.lib.mxCreateCellMatrix(len(arrays), 1)
        for i, a in enumerate(arrays):
            if a is not None:
                self.lib.mxSetCell(mx, i, self.double(a))
        return mx

    def run(self, nlhs, prhs):
        plhs = (P * max(nlhs, 1))()
        rhs = (P * max(len(prhs), 1))(*prhs)
        buf = C.create_string_buffer(2048)
        self.lib.ref_reset_warnings()
        rc = self.lib.ref_run(nlhs, plhs, len(prhs), rhs, buf, len(buf))
        warn = (self.lib.ref_warnings() or b'').decode(errors='replace')
        return rc, list(plhs), buf.value.decode(errors='replace'), warn, int(self.lib.ref_warning_count())


def properties(m, params=None, sol=None, init=None, randstream=None):
    """What the object's properties hold, as plain data.  ``sol``: anything with nt, nst, len[it, ist], cell_M(it, ist)
    -> [len x 4] and cell_D(it, ist) -> [thlen x 2]; its cells go in as 'M' and 'D' (lists in cell order ist + it*nst,
    None = empty cell)."""
    d = m.descriptor()
    optim = m.analyse_optim()
    p = {k: (float(d[k]) if k in d else float(getattr(m, k))) for k in SCALARS}
    p['stm'] = np.asarray(m.stm, dtype=float).reshape(1, -1)
    p['states'] = np.asarray(m.states, dtype=float)
    p['decisions'] = np.asarray(m.decisions, dtype=float)
    p['quadrature'] = np.asarray(d['quadrature'], dtype=float).reshape(2, -1).T
    p['optim'] = [bool(optim[k]) for k in OPTIM]
    p['param'] = np.asarray(m.param_vector() if params is None else params, dtype=np.float64).reshape(-1)
    p['s'] = [(v.type == 'discrete', np.asarray(v.values if v.type == 'continuous' else [], dtype=float)) for v in m.s]
    p['eq'] = len(m.eq)
    if init is not None:
        p['init'] = np.atleast_2d(np.asarray(init, dtype=float))
    if randstream is not None:
        p['randstream'] = np.asarray(randstream, dtype=float)
    if sol is not None:
        Mc, Dc = [], []
        for it in range(sol.nt):             # cell index ist + it*nst
            for ist in range(sol.nst):
                if sol.len[it, ist] > 0:
                    Mc.append(np.asarray(sol.cell_M(it, ist), dtype=float))
                    Dc.append(np.asarray(sol.cell_D(it, ist), dtype=float))
                else:
                    Mc.append(None)
                    Dc.append(None)
        p['M'], p['D'] = Mc, Dc
    return p


def build_object(h, p, M=None, D=None):
    """The model object from ``properties()``.  A property absent from ``p`` is absent from the object (mxGetProperty then
    gives NULL).  ``M`` / ``D``: ready mxArray cell arrays to use instead of p['M'] / p['D'] (a solver gateway's outputs)."""
    obj = h.struct(1, PROPS)
    put = lambda k, v: h.lib.mxSetField(obj, 0, k.encode(), v)   # noqa: E731
    for k in SCALARS + ('stm', 'states', 'decisions', 'quadrature', 'init', 'randstream'):
        if k in p:
            put(k, h.double(p[k]))
    if 'optim' in p:
        o = h.struct(1, OPTIM)
        for k, v in zip(OPTIM, p['optim']):
            h.lib.mxSetField(o, 0, k.encode(), h.lib.mxCreateLogicalScalar(bool(v)))
        put('optim', o)
    if 'param' in p and len(p['param']):
        ps = h.struct(len(p['param']), ('value',))
        for i, v in enumerate(p['param']):
            h.lib.mxSetField(ps, i, b'value', h.lib.mxCreateDoubleScalar(float(v)))
        put('param', ps)
    if 's' in p:
        ss = h.struct(len(p['s']), ('discrete', 'grid'))
        for i, (discrete, grid) in enumerate(p['s']):
            h.lib.mxSetField(ss, i, b'discrete', h.lib.mxCreateLogicalScalar(bool(discrete)))
            h.lib.mxSetField(ss, i, b'grid', h.double(grid))
        put('s', ss)
    if 'eq' in p:
        put('eq', h.struct(int(p['eq']), ('ref',)))
    if M is not None or 'M' in p:
        put('M', M if M is not None else h.cells(p['M']))
    if D is not None or 'D' in p:
        put('D', D if D is not None else h.cells(p['D']))
    return obj
