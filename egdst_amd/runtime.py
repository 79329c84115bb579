"""ctypes binding of the per-model C ABI (include/egdst.h) + the solve/sim plumbing of the class.

No torch types cross the boundary; torch is only used by callers that want device-resident
parameter batches (``Solver.set_params_torch``).  There is no CPU fallback: if the HIP library
cannot be loaded, or no GPU is visible, every entry point raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np


class EgdstDesc(C.Structure):
    _fields_ = [('t0', C.c_int), ('T', C.c_int), ('ngridm', C.c_int), ('ngridmax', C.c_int),
                ('nthrhmax', C.c_int), ('ny', C.c_int), ('mmax', C.c_double), ('a0', C.c_double),
                ('quadrature', C.POINTER(C.c_double))]


class EgdstModelInfo(C.Structure):
    _fields_ = [('nst', C.c_int), ('nd', C.c_int), ('nnst', C.c_int), ('nnd', C.c_int), ('nparam', C.c_int),
                ('neq', C.c_int), ('distrib', C.c_int), ('optim_MUnoD', C.c_int), ('optim_UnoD', C.c_int),
                ('optim_UasD', C.c_int), ('optim_TRPRnoSH', C.c_int), ('tolerance', C.c_double),
                ('zeroconsumption', C.c_double), ('doublepoint_delta', C.c_double), ('label', C.c_char_p)]


# every symbol include/egdst.h declares (checked by the CPU test-suite against the header)
ABI_SYMBOLS = ['egdst_get_model_info', 'egdst_strerror', 'egdst_last_error', 'egdst_create', 'egdst_destroy',
               'egdst_set_params', 'egdst_set_params_dev', 'egdst_solve_async', 'egdst_sync', 'egdst_solve',
               'egdst_get_status', 'egdst_get_evals', 'egdst_cell_dims', 'egdst_get_cell_M', 'egdst_get_cell_D',
               'egdst_get_solution', 'egdst_simulate', 'egdst_device_tables', 'egdst_get_debug', 'egdst_set_profile',
               'egdst_get_profile', 'egdst_objective_dev', 'egdst_get_objective', 'egdst_get_params',
               'egdst_create_compact', 'egdst_geometry', 'egdst_set_groups', 'egdst_set_adaptive', 'egdst_get_schedule', 'egdst_get_work', 'egdst_get_regenerations', 'egdst_call', 'egdst_simulate_moments',
               'egdst_get_checksums', 'egdst_math_eval', 'egdst_get_evals_credited', 'egdst_simulate_batch_moments',
               'egdst_uniform', 'egdst_set_dbgout', 'egdst_get_dbgout', 'egdst_get_walk_stats', 'egdst_get_sort_stats',
               'egdst_set_cell_M', 'egdst_set_cell_D', 'egdst_set_solution', 'egdst_get_tp_stats', 'egdst_get_tp_inplace', 'egdst_get_tp_tail_counts', 'egdst_get_group_profile',
               'egdst_simulate_batch_spec', 'egdst_quantile_eval', 'egdst_quantile_lds_keys', 'egdst_simulate_batch_spec_lag',
               'egdst_simulate_batch_spec_cov', 'egdst_cov_parts', 'egdst_stamp_names', 'egdst_get_stamps',
               'egdst_policy_batch', 'egdst_policy_parts', 'egdst_quantile_band_eval',
               'egdst_attach_panel', 'egdst_fit_dev', 'egdst_get_fit']


class EgdstRuntimeError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__('egdst error %d: %s' % (code, msg))
        self.code = code


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


class ModelLibrary:
    """One loaded per-model shared library."""

    def __init__(self, path, tag=''):
        if not os.path.exists(path):
            raise EgdstRuntimeError(3, 'HIP library %s is missing: run model.compile() (no CPU fallback exists)' % path)
        self.path, self.tag = path, tag
        self.lib = C.CDLL(path, mode=getattr(os, 'RTLD_LOCAL', 0) | getattr(os, 'RTLD_NOW', 2))
        L = self.lib
        for s in ABI_SYMBOLS:
            getattr(L, s)  # AttributeError if the library does not export what the header declares
        L.egdst_strerror.restype = C.c_char_p
        L.egdst_last_error.restype = C.c_char_p
        L.egdst_create.argtypes = [C.POINTER(EgdstDesc), C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]
        L.egdst_create_compact.argtypes = [C.POINTER(EgdstDesc), C.c_int, C.c_int, C.c_int, C.c_void_p,
                                           C.POINTER(C.c_void_p)]
        L.egdst_set_groups.argtypes = [C.c_void_p, C.c_int]
        L.egdst_set_adaptive.argtypes = [C.c_void_p, C.c_int]
        L.egdst_call.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.egdst_get_schedule.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.egdst_geometry.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.egdst_get_objective.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        L.egdst_get_params.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        L.egdst_destroy.argtypes = [C.c_void_p]
        L.egdst_set_params.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int]
        L.egdst_set_params_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.egdst_solve_async.argtypes = [C.c_void_p]
        L.egdst_sync.argtypes = [C.c_void_p]
        L.egdst_solve.argtypes = [C.c_void_p]
        L.egdst_get_status.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.egdst_get_evals.argtypes = [C.c_void_p, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
        L.egdst_get_evals_credited.argtypes = [C.c_void_p, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
        L.egdst_simulate_batch_moments.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int, C.c_void_p, C.c_longlong, C.c_ulonglong,
                                                   C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_void_p, C.c_void_p, C.c_void_p]
        L.egdst_simulate_batch_spec.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int, C.c_void_p, C.c_longlong, C.c_ulonglong,
                                                C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                                C.c_void_p, C.c_void_p, C.c_void_p]
        L.egdst_simulate_batch_spec_lag.argtypes = L.egdst_simulate_batch_spec.argtypes
        L.egdst_simulate_batch_spec_cov.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int, C.c_void_p, C.c_longlong, C.c_ulonglong,
                                                    C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.egdst_cov_parts.argtypes = []
        L.egdst_policy_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 5
        L.egdst_policy_parts.argtypes = []
        L.egdst_attach_panel.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        L.egdst_fit_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.egdst_get_fit.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int)]
        L.egdst_uniform.restype = C.c_double
        L.egdst_uniform.argtypes = [C.c_ulonglong, C.c_ulonglong]
        L.egdst_set_dbgout.argtypes = [C.c_void_p, C.c_int]
        L.egdst_get_dbgout.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int)]
        L.egdst_cell_dims.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.egdst_get_cell_M.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]
        L.egdst_get_cell_D.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]
        L.egdst_get_solution.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)] + \
            [C.POINTER(C.c_double)] * 5
        L.egdst_set_cell_M.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]
        L.egdst_set_cell_D.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]
        L.egdst_set_solution.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)] + \
            [C.POINTER(C.c_double)] * 5
        L.egdst_simulate.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double),
                                     C.c_longlong, C.c_int, C.POINTER(C.c_double)]
        L.egdst_simulate_moments.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double),
                                             C.c_longlong, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int)]
        L.egdst_get_debug.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        L.egdst_stamp_names.argtypes = [C.POINTER(C.c_char_p), C.c_int]
        L.egdst_get_stamps.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_ulonglong)]
        L.egdst_objective_dev.argtypes = [C.c_void_p, C.c_void_p]
        L.egdst_set_profile.argtypes = [C.c_void_p, C.c_int]
        L.egdst_get_profile.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_longlong)]
        L.egdst_get_checksums.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.egdst_math_eval.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.egdst_quantile_eval.argtypes = [C.c_int, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                          C.POINTER(C.c_int)]
        L.egdst_quantile_band_eval.argtypes = [C.c_int, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                               C.POINTER(C.c_double), C.POINTER(C.c_int)]
        L.egdst_quantile_lds_keys.argtypes = []
        L.egdst_device_tables.argtypes = [C.c_void_p, C.c_int] + [C.POINTER(C.c_void_p)] * 4
        info = EgdstModelInfo()
        L.egdst_get_model_info(C.byref(info))
        self.info = info

    @property
    def nout(self):
        """columns of a simulated path (egdst_simulate: nsimout)"""
        return 11 + self.info.nnst + self.info.nnd + self.info.neq

    def check(self, rc):
        if rc != 0:
            raise EgdstRuntimeError(rc, (self.lib.egdst_last_error() or b'').decode(errors='replace'))

    def lerp_eval(self, x, g0, g1, f0, f1, shared=True):
        """linter's interpolation on the device: the grid kernels' shared-reciprocal form or the plain one (egdst_math_eval 3 / 4)."""
        xs = np.ascontiguousarray(np.concatenate([np.asarray(a, dtype=np.float64).ravel() for a in (x, g0, g1)]))
        ys = np.ascontiguousarray(np.concatenate([np.asarray(a, dtype=np.float64).ravel() for a in (f0, f1)]))
        n = xs.size // 3
        out = np.zeros(n)
        self.check(self.lib.egdst_math_eval(3 if shared else 4, n, _dp(xs), _dp(ys), _dp(out)))
        return out

    def math_eval(self, fn, x, y=None):
        """The device's exp ('exp'), log ('log'), pow ('pow') on host arrays (egdst_math_eval)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.ascontiguousarray(x if y is None else y, dtype=np.float64)
        out = np.zeros_like(x)
        self.check(self.lib.egdst_math_eval({'exp': 0, 'log': 1, 'pow': 2}[fn], x.size, _dp(x), _dp(y), _dp(out)))
        return out

    @property
    def quantile_lds_keys(self):
        """candidates up to which k_quantiles selects in LDS (the library's QNT_LDS_KEYS, egdst_quantile_lds_keys)"""
        return int(self.lib.egdst_quantile_lds_keys())

    @property
    def cov_parts(self):
        """partial sums P of the covariance's summation order (the library's COV_P, egdst_cov_parts): what
        MomentSpec.covariance takes as `parts` to give the device's bits"""
        return int(self.lib.egdst_cov_parts())

    @property
    def policy_parts(self):
        """partial sums B of the fit's summation order (the library's POL_BS, egdst_policy_parts): what datafit.fit_mirror takes
        as `block` to give the device's bits"""
        return int(self.lib.egdst_policy_parts())

    def quantile_eval(self, x, p):
        """(quantiles p of the host array x by the device's selection, the number of non-NaN values): egdst_quantile_eval,
        the kernel of the kind-3 moments on caller-supplied values."""
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
        p = np.ascontiguousarray(np.atleast_1d(p), dtype=np.float64).reshape(-1)
        out = np.zeros(p.size)
        cnt = C.c_int(0)
        self.check(self.lib.egdst_quantile_eval(x.size, _dp(x), p.size, _dp(p), _dp(out), C.byref(cnt)))
        return out, cnt.value

    def quantile_band_eval(self, x, p, h):
        """(out [np, 3], the number of non-NaN values): per quantile p[i] with bandwidth h[i] of the host array x the order
        statistics a = Q(p - h), b = Q(p + h) and the sparsity s by the device's k_quantile_band (egdst_quantile_band_eval);
        moments.quantile_band is the same on the host."""
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
        p = np.ascontiguousarray(np.atleast_1d(p), dtype=np.float64).reshape(-1)
        h = np.ascontiguousarray(np.broadcast_to(np.atleast_1d(np.asarray(h, dtype=np.float64)), p.shape))
        out = np.zeros((p.size, 3))
        cnt = C.c_int(0)
        self.check(self.lib.egdst_quantile_band_eval(x.size, _dp(x), p.size, _dp(p), _dp(h), _dp(out), C.byref(cnt)))
        return out, cnt.value


class Solution:
    """Host copy of one draw's solution in the table layout shared with the oracle harness."""

    def __init__(self, nt, nst, ngridmax, nthrhmax):
        self.nt, self.nst = nt, nst
        self.M = np.zeros((nt, nst, ngridmax + 1))
        self.C = np.zeros((nt, nst, ngridmax + 1))
        self.V = np.zeros((nt, nst, ngridmax + 1))
        self.D = np.zeros((nt, nst, nthrhmax))
        self.TH = np.zeros((nt, nst, nthrhmax))
        self.len = np.zeros((nt, nst), dtype=np.int32)
        self.thlen = np.zeros((nt, nst), dtype=np.int32)
        self.nevals = 0
        self.status = 0
        self.where = (0, 0)
        self.err = ''

    def cell_M(self, it, ist):
        n = self.len[it, ist]
        m, c, v = self.M[it, ist, :n], self.C[it, ist, :n], self.V[it, ist, :n]
        return np.stack([m, c, m - c, v], axis=1)

    def cell_D(self, it, ist):
        n = self.thlen[it, ist]
        return np.stack([self.D[it, ist, :n], self.TH[it, ist, :n]], axis=1)

    def total_rows(self):
        return int(self.len.sum())

    def cells(self):
        """(M, D) as nst x nt nested lists of matrices: the MATLAB cell arrays of solve (empty = None)."""
        M = [[self.cell_M(it, ist) if self.len[it, ist] else None for it in range(self.nt)] for ist in range(self.nst)]
        D = [[self.cell_D(it, ist) if self.len[it, ist] else None for it in range(self.nt)] for ist in range(self.nst)]
        return M, D


class Solver:
    """A device-resident batch of `ndraw` independent solves of one compiled model.

    rows_cap > 0 makes the handle COMPACT (include/egdst.h: egdst_create_compact): device lists and tables hold
    rows_cap rows instead of ngridmax, which keeps thousands of resident draws dense in memory.  A draw that needs
    more rows stops with EGDST_E_CAPACITY on the device; `sync` then solves exactly those draws again on a second,
    exact handle and every accessor below answers for them from there, so callers see the reference's semantics.
    """
    E_CAPACITY = 28

    def __init__(self, lib: ModelLibrary, desc: dict, ndraw=1, keep_history=True, stream=None, rows_cap=0):
        self.lib, self.ndraw, self.keep_history = lib, int(ndraw), bool(keep_history)
        self._quad = np.ascontiguousarray(desc['quadrature'], dtype=np.float64)
        ngridmax = desc['ngridmax'] if desc['ngridmax'] > desc['ngridm'] else 2 * desc['ngridm']
        self.desc = dict(desc, ngridmax=ngridmax)
        d = EgdstDesc(desc['t0'], desc['T'], desc['ngridm'], ngridmax, desc['nthrhmax'], desc['ny'],
                      desc['mmax'], desc['a0'], _dp(self._quad))
        self.nt = desc['T'] - desc['t0'] + 1
        self.h = C.c_void_p()
        self.rows_cap = int(rows_cap) if 0 < int(rows_cap) < ngridmax else 0
        self._exact = None          # exact handle for the draws that overflowed the compact one
        self._redo = np.zeros(0, dtype=np.int64)   # their draw indices, in the order of self._exact
        self.capacity_retries = 0   # draws solved again since creation
        lib.check(lib.lib.egdst_create_compact(C.byref(d), self.ndraw, int(self.keep_history), self.rows_cap,
                                               C.c_void_p(stream) if stream else None, C.byref(self.h)))

    def close(self):
        if self._exact is not None:
            self._exact.close()
            self._exact = None
        if self.h:
            self.lib.lib.egdst_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_groups(self, ngroups):
        """Split the draws into `ngroups` ranges that run on their own streams (egdst_set_groups)."""
        self.lib.check(self.lib.lib.egdst_set_groups(self.h, int(ngroups)))

    def set_adaptive(self, on=True):
        """History-based scheduling of straggler draws on lanes of their own (egdst_set_adaptive)."""
        self.lib.check(self.lib.lib.egdst_set_adaptive(self.h, int(bool(on))))

    def schedule(self):
        """(regular groups, straggler lanes, straggler draws) of the next solve"""
        a, b, c = C.c_int(0), C.c_int(0), C.c_int(0)
        self.lib.check(self.lib.lib.egdst_get_schedule(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def walk_stats(self):
        """[ndraw, 2]: envelope walks cut into segments and merged / fallen back to one wave (egdst_get_walk_stats)"""
        out = np.zeros((self.ndraw, 2), dtype=np.uint32)
        self.lib.check(self.lib.lib.egdst_get_walk_stats(self.h, out.ctypes.data_as(C.c_void_p)))
        return out

    def sort_stats(self):
        """[ndraw, 4]: LDS sorts of the last solve's envelope jobs with the lists in order / through the network / by counting ranks, and those
        of them with two or more pairs out of order seen by different threads (egdst_get_sort_stats)"""
        out = np.zeros((self.ndraw, 4), dtype=np.uint32)
        self.lib.check(self.lib.lib.egdst_get_sort_stats(self.h, out.ctypes.data_as(C.c_void_p)))
        return out

    def tp_stats(self):
        """[ndraw, 2]: cells of the last solve completed by the throughput path of the envelope step / left to k_envelope"""
        out = np.zeros((self.ndraw, 2), dtype=np.uint32)
        self.lib.check(self.lib.lib.egdst_get_tp_stats(self.h, out.ctypes.data_as(C.c_void_p)))
        return out

    def tp_inplace(self):
        """[ndraw]: second-tier cells of the last solve that gave up and were done in place by the tail launch (egdst_get_tp_inplace)"""
        out = np.zeros(self.ndraw, dtype=np.uint32)
        self.lib.check(self.lib.lib.egdst_get_tp_inplace(self.h, out.ctypes.data_as(C.c_void_p)))
        return out

    MAX_GROUPS = 32   # EGDST_MAX_GROUPS of the library (egdst_set_groups: at most 32)

    def tp_tail_counts(self):
        """(rest[MAX_GROUPS, nt], big[MAX_GROUPS, nt]): per draw group and period of the last solve, the cells the throughput path left over and the
        cells of its second tier -- the two lists of the period's tail launch (egdst_get_tp_tail_counts)"""
        rest, big = np.zeros((self.MAX_GROUPS, self.nt), dtype=np.int32), np.zeros((self.MAX_GROUPS, self.nt), dtype=np.int32)
        self.lib.check(self.lib.lib.egdst_get_tp_tail_counts(self.h, self.MAX_GROUPS, rest.ctypes.data_as(C.c_void_p), big.ctypes.data_as(C.c_void_p)))
        return rest, big

    def work(self):
        """re-basing calls per draw in the last solve (egdst_get_work)"""
        out = np.zeros(self.ndraw, dtype=np.uint32)
        self.lib.check(self.lib.lib.egdst_get_work(self.h, out.ctypes.data_as(C.c_void_p)))
        return out

    def regenerations(self):
        """regenerated guess streams per draw in the last solve (egdst_get_regenerations)"""
        out = np.zeros(self.ndraw, dtype=np.uint32)
        self.lib.check(self.lib.lib.egdst_get_regenerations(self.h, out.ctypes.data_as(C.c_void_p)))
        return out

    def geometry(self):
        """(physical rows per list, row stride of the device tables)"""
        a, b = C.c_int(0), C.c_int(0)
        self.lib.check(self.lib.lib.egdst_geometry(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def device_tables(self, it):
        """(M, C, V, len, stride) of period `it` where the handle keeps it: device pointers (ints) of the M, C and V tables,
        [ndraw][nst][stride] doubles, and of the lengths, [ndraw][nst] ints (egdst_device_tables), with the row stride of
        egdst_geometry.  Without history a period lives in slot it & 1: after a solve the two slots hold periods 0 and 1."""
        p = [C.c_void_p() for _ in range(4)]
        self.lib.check(self.lib.lib.egdst_device_tables(self.h, int(it), *[C.byref(x) for x in p]))
        return tuple(int(x.value or 0) for x in p) + (self.geometry()[1],)

    def _route(self, draw):
        """(solver, local draw) that holds the results of `draw`"""
        if len(self._redo):
            j = np.nonzero(self._redo == draw)[0]
            if len(j):
                return self._exact, int(j[0])
        return self, draw

    def set_params(self, params):
        p = np.ascontiguousarray(np.asarray(params, dtype=np.float64).reshape(self.ndraw, -1))
        if p.shape[1] != self.lib.info.nparam:
            raise EgdstRuntimeError(1, 'expected %d parameters per draw, got %d' % (self.lib.info.nparam, p.shape[1]))
        self.lib.check(self.lib.lib.egdst_set_params(self.h, _dp(p), self.ndraw))

    def set_params_dev(self, dev_ptr):
        self.lib.check(self.lib.lib.egdst_set_params_dev(self.h, C.c_void_p(dev_ptr), self.ndraw))

    def solve_async(self):
        self.lib.check(self.lib.lib.egdst_solve_async(self.h))

    def sync(self, raise_on_error=True):
        rc = self.lib.lib.egdst_sync(self.h)
        self._redo = np.zeros(0, dtype=np.int64)
        if rc and self.rows_cap:
            rc = self._redo_overflowed()
        if rc and (raise_on_error or rc < 10):
            self.lib.check(rc)
        return rc

    def _redo_overflowed(self):
        """Solve the draws that stopped with EGDST_E_CAPACITY again with exact capacities; returns the first
        non-zero per-draw status of the batch after that (what egdst_sync would have returned)."""
        st, _ = self._status_raw()
        idx = np.nonzero(st == self.E_CAPACITY)[0]
        if len(idx):
            par = np.zeros((self.ndraw, max(self.lib.info.nparam, 1)))
            self.lib.check(self.lib.lib.egdst_get_params(self.h, _dp(par)))
            if self._exact is None or self._exact.ndraw != len(idx):
                if self._exact is not None:
                    self._exact.close()
                self._exact = Solver(self.lib, self.desc, ndraw=len(idx), keep_history=self.keep_history)
            self._exact.set_params(par[idx, :self.lib.info.nparam])
            self._exact.solve(raise_on_error=False)
            self._redo = idx.astype(np.int64)
            self.capacity_retries += len(idx)
        st, _ = self.status()
        bad = st[st != 0]
        return int(bad[0]) if len(bad) else 0

    def solve(self, raise_on_error=True):
        self.solve_async()
        return self.sync(raise_on_error)

    def _status_raw(self):
        st = np.zeros(self.ndraw, dtype=np.int32)
        wh = np.zeros(2 * self.ndraw, dtype=np.int32)
        self.lib.check(self.lib.lib.egdst_get_status(self.h, _ip(st), _ip(wh)))
        return st, wh.reshape(self.ndraw, 2)

    def status(self):
        st, wh = self._status_raw()
        if len(self._redo):
            st[self._redo], wh[self._redo] = self._exact.status()
        return st, wh

    def evals(self):
        tot = C.c_longlong(0)
        per = np.zeros(self.ndraw, dtype=np.int64)
        self.lib.check(self.lib.lib.egdst_get_evals(self.h, C.byref(tot), per.ctypes.data_as(C.POINTER(C.c_longlong))))
        if len(self._redo):
            per[self._redo] = self._exact.evals()[1]
            return int(per.sum()), per
        return int(tot.value), per

    def evals_credited(self):
        """per-draw evaluations that were accounted for without being executed (egdst_get_evals_credited)"""
        tot = C.c_longlong(0)
        per = np.zeros(self.ndraw, dtype=np.int64)
        self.lib.check(self.lib.lib.egdst_get_evals_credited(self.h, C.byref(tot), per.ctypes.data_as(C.POINTER(C.c_longlong))))
        if len(self._redo):
            per[self._redo] = self._exact.evals_credited()
        return per

    def objective(self):
        """[ndraw, 2] host array of the objective contributions (egdst_objective_dev), NaN for failed draws."""
        out = np.zeros((self.ndraw, 2))
        self.lib.check(self.lib.lib.egdst_get_objective(self.h, _dp(out)))
        if len(self._redo):
            out[self._redo] = self._exact.objective()
        return out

    def solution(self, draw=0):
        if len(self._redo):
            s_, j_ = self._route(draw)
            if s_ is not self:
                return s_.solution(j_)
        d = self.desc
        sol = Solution(self.nt, self.lib.info.nst, d['ngridmax'], d['nthrhmax'])
        self.lib.check(self.lib.lib.egdst_get_solution(self.h, draw, _ip(sol.len), _ip(sol.thlen), _dp(sol.M),
                                                       _dp(sol.C), _dp(sol.V), _dp(sol.D), _dp(sol.TH)))
        st, wh = self.status()
        sol.status, sol.where = int(st[draw]), tuple(int(x) for x in wh[draw])
        sol.err = self.lib.lib.egdst_strerror(sol.status).decode() if sol.status else ''
        sol.nevals = int(self.evals()[1][draw])
        return sol

    def set_solution(self, sol, draw=0):
        """Import a host solution (the arrays `solution()` returns) into `draw`: egdst_set_solution, the inverse of the
        export.  The handle then simulates / evaluates `call` from it without having solved (egdst_simulator.c:61-68)."""
        ln = np.ascontiguousarray(sol.len, dtype=np.int32)
        th = np.ascontiguousarray(sol.thlen, dtype=np.int32)
        arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (sol.M, sol.C, sol.V, sol.D, sol.TH)]
        d = self.desc
        if arrs[0].shape != (self.nt, self.lib.info.nst, d['ngridmax'] + 1) or arrs[3].shape != (self.nt, self.lib.info.nst, d['nthrhmax']):
            raise EgdstRuntimeError(1, 'set_solution: the arrays do not have the shapes of this handle')
        self.lib.check(self.lib.lib.egdst_set_solution(self.h, draw, _ip(ln), _ip(th), *[_dp(a) for a in arrs]))

    def set_cells(self, M, D, draw=0):
        """Import the MATLAB-style cell arrays (nst x nt nested lists of (len x 4) [M C A V] and (thlen x 2) [D TH]
        matrices, None / empty = unsolved cell) cell by cell: egdst_set_cell_M / egdst_set_cell_D, what a MEX shim of the
        simulator gateway does with mxGetCell (shims/egdst_simulator_hip.c)."""
        for ist in range(self.lib.info.nst):
            for it in range(self.nt):
                m = None if M[ist][it] is None else np.asfortranarray(np.asarray(M[ist][it], dtype=np.float64))
                dd = None if D[ist][it] is None else np.asfortranarray(np.asarray(D[ist][it], dtype=np.float64))
                nm = 0 if m is None or m.size == 0 else m.shape[0]
                nd_ = 0 if dd is None or dd.size == 0 else dd.shape[0]
                if nm and m.shape[1] != 4 or nd_ and dd.shape[1] != 2:
                    raise EgdstRuntimeError(1, 'set_cells: cell (%d, %d) is not (len x 4) / (thlen x 2)' % (ist, it))
                self.lib.check(self.lib.lib.egdst_set_cell_M(self.h, draw, it, ist, nm, _dp(m) if nm else None))
                self.lib.check(self.lib.lib.egdst_set_cell_D(self.h, draw, it, ist, nd_, _dp(dd) if nd_ else None))

    def set_dbgout(self, on=True):
        """keep the kink log of the next solves (third output of the solver gateway)"""
        self.lib.check(self.lib.lib.egdst_set_dbgout(self.h, int(bool(on))))

    def dbgout(self, draw=0):
        """(matrix [cap, 7] as the gateway returns it, number of recorded rows)"""
        info = self.lib.info
        cap = self.nt * info.nst * info.nd * 2 * self.nt
        out = np.zeros((cap, 7), order='F')
        n = C.c_int(0)
        self.lib.check(self.lib.lib.egdst_get_dbgout(self.h, draw, _dp(out), C.byref(n)))
        return out, n.value

    def checksums(self, draw=0):
        """[nt, nst, 5] uint64 checksums of the draw's cells (columns M, C, V, TH, D), computed on the device."""
        if len(self._redo) and self._route(draw)[0] is not self:
            s_, j_ = self._route(draw)
            return s_.checksums(j_)
        out = np.zeros((self.nt, self.lib.info.nst, 5), dtype=np.uint64)
        self.lib.check(self.lib.lib.egdst_get_checksums(self.h, draw, out.ctypes.data_as(C.c_void_p)))
        return out

    def dims(self, draw=0):
        """(len, thlen) [nt, nst] of the draw's cells without copying the tables."""
        ln = np.zeros((self.nt, self.lib.info.nst), dtype=np.int32)
        th = np.zeros((self.nt, self.lib.info.nst), dtype=np.int32)
        self.lib.check(self.lib.lib.egdst_get_solution(self.h, draw, _ip(ln), _ip(th), None, None, None, None, None))
        return ln, th

    def objective_dev(self, dev_ptr):
        """Device-side objective of THIS handle's draws (draws redone after a capacity overflow read NaN here;
        use objective() when rows_cap is set and capacity_retries may be non-zero)."""
        self.lib.check(self.lib.lib.egdst_objective_dev(self.h, C.c_void_p(dev_ptr)))

    def set_profile(self, on=True):
        self.lib.check(self.lib.lib.egdst_set_profile(self.h, int(on)))

    PROFILE_CLASSES = ['probe', 'grid', 'k_envelope', 'regeneration', 'tp_prep', 'tp_sort0', 'tp_sort1', 'tp_walk0', 'tp_walk1']

    def profile(self):
        """(ms[9], launches[9], algorithmic bytes) of the last solve by kernel class (PROFILE_CLASSES; include/egdst.h)."""
        ms = np.zeros(9)
        ln = np.zeros(9, dtype=np.int32)
        ab = C.c_longlong(0)
        self.lib.check(self.lib.lib.egdst_get_profile(self.h, _dp(ms), _ip(ln), C.byref(ab)))
        return ms, ln, int(ab.value)

    def group_profile(self):
        """(finish[g], class_ms[g, 9]) of the last solve with profiling on: ms from the first group's first kernel to the end of group
        g's last kernel, and the group's summed HIP-event time per kernel class (egdst_get_group_profile)"""
        fin = np.zeros(32)
        cls = np.zeros((32, 9))
        self.lib.lib.egdst_get_group_profile.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        n = self.lib.lib.egdst_get_group_profile(self.h, 32, _dp(fin), _dp(cls))
        return fin[:n], cls[:n]

    def debug(self, draw=0):
        out = np.zeros(16, dtype=np.int32)
        self.lib.check(self.lib.lib.egdst_get_debug(self.h, draw, _ip(out)))
        return out

    def stamps(self, draw=0):
        """{slot name: ticks of 10 ns, or a count} of one draw in the last solve; needs a library built with -DEGDST_STAMPS=<set>
        (the slots of the other sets are zero; egdst_stamp_names, egdst_get_stamps)"""
        L = self.lib.lib
        n = L.egdst_stamp_names(None, 0)
        names = (C.c_char_p * n)()
        L.egdst_stamp_names(names, n)
        out = np.zeros(n, dtype=np.uint64)
        self.lib.check(L.egdst_get_stamps(self.h, draw, out.ctypes.data_as(C.POINTER(C.c_ulonglong))))
        return {names[i].decode(): int(out[i]) for i in range(n)}

    def cell_M(self, draw, it, ist):
        if len(self._redo) and self._route(draw)[0] is not self:
            s_, j_ = self._route(draw)
            return s_.cell_M(j_, it, ist)
        n, nth = C.c_int(0), C.c_int(0)
        self.lib.check(self.lib.lib.egdst_cell_dims(self.h, draw, it, ist, C.byref(n), C.byref(nth)))
        out = np.zeros((4, n.value))
        if n.value:
            self.lib.check(self.lib.lib.egdst_get_cell_M(self.h, draw, it, ist, _dp(out)))
        return np.ascontiguousarray(out.T)  # column-major (len x 4) -> rows

    def cell_D(self, draw, it, ist):
        if len(self._redo) and self._route(draw)[0] is not self:
            s_, j_ = self._route(draw)
            return s_.cell_D(j_, it, ist)
        n, nth = C.c_int(0), C.c_int(0)
        self.lib.check(self.lib.lib.egdst_cell_dims(self.h, draw, it, ist, C.byref(n), C.byref(nth)))
        out = np.zeros((2, nth.value))
        if nth.value:
            self.lib.check(self.lib.lib.egdst_get_cell_D(self.h, draw, it, ist, _dp(out)))
        return np.ascontiguousarray(out.T)

    def simulate_moments(self, init, randstream, rndtype=0, draw=0):
        """(means [nt, nout], counts [nt, nout]) of the simulated paths over the agents that have a value in a period;
        the paths themselves stay on the device (egdst_simulate_moments)."""
        if len(self._redo) and self._route(draw)[0] is not self:
            s_, j_ = self._route(draw)
            return s_.simulate_moments(init, randstream, rndtype, j_)
        init = np.asfortranarray(np.atleast_2d(np.asarray(init, dtype=np.float64)))
        means = np.zeros((self.nt, self.lib.nout))
        counts = np.zeros((self.nt, self.lib.nout), dtype=np.int32)
        rs = np.ascontiguousarray(randstream, dtype=np.float64)
        self.lib.check(self.lib.lib.egdst_simulate_moments(self.h, draw, _dp(init), init.shape[0], _dp(rs), rs.size, int(rndtype),
                                                           _dp(means), _ip(counts)))
        return means, counts

    def _estimation_step(self, entry, init, seed, rndtype, randstream_dev, nrand, shape, args, third, means_dev, counts_dev,
                         third_dev):
        """The one call path of simulate_batch_moments, simulate_batch_spec and simulate_batch_cov: `entry` is the library's
        function, args what it takes between rndtype and the outputs (records, target, weights), shape the moments of a
        draw, third the shape per draw of the third output -- () the objective, (nmom, nmom) the covariance, None: there is
        none.  With no device pointers given the results go through torch tensors allocated here and are returned."""
        init = np.asfortranarray(np.atleast_2d(np.asarray(init, dtype=np.float64)))
        own = means_dev is None and counts_dev is None and third_dev is None
        if own:
            import torch
            tm = torch.zeros(self.ndraw, *shape, dtype=torch.float64, device='cuda')
            tc = torch.zeros(self.ndraw, *shape, dtype=torch.int32, device='cuda')
            t3 = torch.zeros(self.ndraw, *third, dtype=torch.float64, device='cuda') if third is not None else None
            # torch fills them on ITS stream; the library writes them on the handle's: without this the fill may land after the
            # results (seen once in a few hundred runs: all moments and objectives zero)
            torch.cuda.current_stream().synchronize()
            means_dev, counts_dev = tm.data_ptr(), tc.data_ptr()
            third_dev = t3.data_ptr() if t3 is not None else None
        self.lib.check(entry(
            self.h, _dp(init), init.shape[0], C.c_void_p(randstream_dev) if randstream_dev else None, int(nrand), int(seed),
            int(rndtype), *args, C.c_void_p(means_dev) if means_dev else None, C.c_void_p(counts_dev) if counts_dev else None,
            C.c_void_p(third_dev) if third_dev else None))
        if own:
            return tm.cpu().numpy(), tc.cpu().numpy(), t3.cpu().numpy() if t3 is not None else None
        return None

    def simulate_batch_moments(self, init, seed=0, rndtype=0, target=None, weight=None, randstream_dev=None, nrand=0,
                               means_dev=None, counts_dev=None, obj_dev=None):
        """egdst_simulate_batch_moments: all draws of the handle, common random numbers; the *_dev arguments are device
        pointers (ints).  With no device pointers given, returns (means [ndraw, nt, nout], counts, objective [ndraw]) through
        torch tensors allocated here."""
        ncell = self.lib.nout * self.nt
        t = np.ascontiguousarray(np.zeros(ncell) if target is None else target, dtype=np.float64).reshape(-1)
        w = np.ascontiguousarray(np.zeros(ncell) if weight is None else weight, dtype=np.float64).reshape(-1)
        return self._estimation_step(self.lib.lib.egdst_simulate_batch_moments, init, seed, rndtype, randstream_dev, nrand,
                                     (self.nt, self.lib.nout), (_dp(t), _dp(w)), (), means_dev, counts_dev, obj_dev)

    def simulate_batch_spec(self, init, spec, seed=0, rndtype=0, target=None, W=None, randstream_dev=None, nrand=0,
                            means_dev=None, counts_dev=None, obj_dev=None):
        """egdst_simulate_batch_spec: the estimation step of simulate_batch_moments with user-defined moments -- spec is a
        moments.MomentSpec (names resolved with this library's columns) or an array of moments.MOMENT_DTYPE -- and a full
        weighting matrix W ([nmom, nmom], or a vector: its diagonal).  The objective is computed when target and W are given.
        A MomentSpec with a lag (spec.lagged) or an array of moments.MOMENT_LAG_DTYPE goes to egdst_simulate_batch_spec_lag.
        The *_dev arguments are device pointers (ints); with none given, returns (means [ndraw, nmom], counts [ndraw, nmom],
        objective [ndraw] or None) through torch tensors allocated here."""
        from . import moments
        rec, lag = moments.lag_records(spec, self.nt, layout=self.lib.info)
        entry = self.lib.lib.egdst_simulate_batch_spec_lag
        if not lag:
            rec, entry = moments.convert_records(rec, moments.MOMENT_DTYPE), self.lib.lib.egdst_simulate_batch_spec
        nmom = len(rec)
        if (target is None) != (W is None):
            raise EgdstRuntimeError(1, 'simulate_batch_spec: the objective needs both target and W')
        t = w = None
        if W is not None:
            t = np.ascontiguousarray(target, dtype=np.float64).reshape(-1)
            if t.size != nmom:
                raise EgdstRuntimeError(1, 'simulate_batch_spec: target has %d entries for %d moments' % (t.size, nmom))
            try:
                w = moments.weight_matrix(W, nmom)
            except ValueError as e:
                raise EgdstRuntimeError(1, 'simulate_batch_spec: %s' % e) from None
        return self._estimation_step(entry, init, seed, rndtype, randstream_dev, nrand, (nmom,),
                                     (rec.ctypes.data_as(C.c_void_p), nmom, _dp(t) if t is not None else None,
                                      _dp(w) if w is not None else None), () if w is not None else None, means_dev, counts_dev, obj_dev)

    def simulate_batch_cov(self, init, spec, seed=0, rndtype=0, randstream_dev=None, nrand=0, means_dev=None, counts_dev=None,
                           cov_dev=None):
        """egdst_simulate_batch_spec_cov: the moments of simulate_batch_spec and, per draw, their covariance matrix Omega
        (agent-clustered, include/egdst.h) -- spec is a moments.MomentSpec or an array of moments.MOMENT_DTYPE or
        moments.MOMENT_LAG_DTYPE, promoted to lag records.  A quantile is taken with a bandwidth (moments.quantile(...,
        bandwidth=h), the record's hi: the spacing estimate of the density at the quantile, 0 < p - h and p + h < 1) and refused
        without one; its row and column of Omega are NaN in a draw where the two ranks of the band coincide or the record is
        empty, and 0.0 where the band lies inside a mass point.  The *_dev arguments are device pointers
        (ints); with none given, returns (means [ndraw, nmom], counts [ndraw, nmom], cov [ndraw, nmom, nmom]) through torch
        tensors allocated here.  moments.MomentSpec.covariance(panel, parts=self.lib.cov_parts) is the same on the host."""
        from . import moments
        rec, _ = moments.lag_records(spec, self.nt, layout=self.lib.info)
        nmom = len(rec)
        return self._estimation_step(self.lib.lib.egdst_simulate_batch_spec_cov, init, seed, rndtype, randstream_dev, nrand, (nmom,),
                                     (rec.ctypes.data_as(C.c_void_p), nmom), (nmom, nmom), means_dev, counts_dev, cov_dev)

    POLICY_OUTPUTS = ('cons', 'id', 'vf', 'ssr', 'hits')

    def policy_batch(self, obs, resid=0, want=POLICY_OUTPUTS, cons_dev=None, id_dev=None, vf_dev=None, ssr_dev=None, hits_dev=None):
        """egdst_policy_batch: the policy at the observations of a data panel for every draw of THIS handle (draws redone after a
        capacity overflow read as failed here), and the fit per draw.  obs is a datafit.Observations or an array of
        datafit.OBS_DTYPE; resid 0: cons - c, 1: log(cons) - log(c).  Cash above mmax is NOT refused: the tables are
        extrapolated over their last two rows, as the simulator does for an agent whose cash has grown past the grid, however far above
        the grid the data lie -- a caller who wants such observations out of the fit gives them w = 0 or leaves them out.  The *_dev arguments are device pointers (ints); with none
        given, the outputs named in `want` are torch device tensors allocated here and returned as a dict: cons, vf float64
        [ndraw, nobs], id int32 [ndraw, nobs], ssr float64 [ndraw], hits int32 [ndraw]."""
        from . import datafit
        rec = datafit.records(obs)
        ptr = dict(cons=cons_dev, id=id_dev, vf=vf_dev, ssr=ssr_dev, hits=hits_dev)
        out = None
        if all(v is None for v in ptr.values()) and len(want):   # (nothing wanted: the library refuses the call)
            import torch
            unknown = [k for k in want if k not in self.POLICY_OUTPUTS]
            if unknown:
                raise EgdstRuntimeError(1, 'policy_batch: unknown outputs %s' % unknown)
            shape = lambda k: (self.ndraw, len(rec)) if k in ('cons', 'id', 'vf') else (self.ndraw,)   # noqa: E731
            out = {k: torch.zeros(*shape(k), dtype=torch.int32 if k in ('id', 'hits') else torch.float64, device='cuda') for k in want}
            torch.cuda.current_stream().synchronize()   # (torch fills on ITS stream, the library writes on the handle's)
            ptr = {k: (out[k].data_ptr() if k in out else None) for k in self.POLICY_OUTPUTS}
        self.lib.check(self.lib.lib.egdst_policy_batch(self.h, rec.ctypes.data_as(C.c_void_p), len(rec), int(resid),
                                                       *[C.c_void_p(ptr[k]) if ptr[k] else None for k in self.POLICY_OUTPUTS]))
        return out

    def attach_panel(self, obs, resid=0):
        """egdst_attach_panel: keep a data panel (a datafit.Observations or an array of datafit.OBS_DTYPE) on the handle; every
        solve from now on evaluates it period by period, with or without history, and fit_dev / fit hand back what
        policy_batch(want=('ssr', 'hits')) gives on a kept-history handle, bit for bit.  Checked as policy_batch checks;
        attaching again replaces the panel.  No fit until the next solve."""
        from . import datafit
        rec = datafit.records(obs)
        if len(rec) == 0:   # (an empty panel is refused, as policy_batch refuses it: detaching is detach_panel's)
            raise EgdstRuntimeError(1, 'attach_panel: no observations')
        self.lib.check(self.lib.lib.egdst_attach_panel(self.h, rec.ctypes.data_as(C.c_void_p), len(rec), int(resid)))

    def detach_panel(self):
        """free the attached panel: the solves enqueue what they did before it"""
        self.lib.check(self.lib.lib.egdst_attach_panel(self.h, None, 0, 0))

    def fit_dev(self, ssr_ptr, hits_ptr):
        """egdst_fit_dev: ssr (float64 [ndraw]) and hits (int32 [ndraw]) of the attached panel into device buffers (ints, either
        may be None), enqueued behind the solve on the handle's stream without a host synchronisation.  Of THIS handle's draws:
        a draw redone after a capacity overflow reads as failed (NaN, -1), as in policy_batch."""
        self.lib.check(self.lib.lib.egdst_fit_dev(self.h, C.c_void_p(ssr_ptr) if ssr_ptr else None, C.c_void_p(hits_ptr) if hits_ptr else None))

    def fit(self):
        """(ssr [ndraw] float64, hits [ndraw] int32) host arrays of the attached panel's fit (egdst_get_fit; synchronises)"""
        ssr, hits = np.zeros(self.ndraw), np.zeros(self.ndraw, dtype=np.int32)
        self.lib.check(self.lib.lib.egdst_get_fit(self.h, _dp(ssr), _ip(hits)))
        return ssr, hits

    def call(self, sw, args, draw=0):
        """egdst_call gateway (egdst_call.c:17-164): sw 1 utility, 2 marginal utility, 3 discount, 4 budget, 5 marginal
        budget, 6 value function; args [narg x ncol] with 1-based it/ist/id as in MATLAB.  Returns [narg]."""
        if len(self._redo) and self._route(draw)[0] is not self:
            s_, j_ = self._route(draw)
            return s_.call(sw, args, j_)
        a = np.asfortranarray(np.atleast_2d(np.asarray(args, dtype=np.float64)))
        res = np.zeros(a.shape[0])
        self.lib.check(self.lib.lib.egdst_call(self.h, draw, int(sw), a.shape[0], a.shape[1], _dp(a), _dp(res)))
        return res

    def simulate(self, init, randstream, rndtype=0, draw=0):
        if len(self._redo) and self._route(draw)[0] is not self:
            s_, j_ = self._route(draw)
            return s_.simulate(init, randstream, rndtype, j_)
        init = np.asfortranarray(np.atleast_2d(np.asarray(init, dtype=np.float64)))
        nsim = init.shape[0]
        sims = np.zeros((nsim, self.nt, self.lib.nout))  # C order == column-major [nout x nt x nsim]
        rs = np.ascontiguousarray(randstream, dtype=np.float64)
        self.lib.check(self.lib.lib.egdst_simulate(self.h, draw, _dp(init), nsim, _dp(rs), rs.size, int(rndtype),
                                                   _dp(sims)))
        return sims


def solve_model(model, dbgout=False):
    """model.solve(): one draw with the model's current parameters, history kept for sim/export."""
    desc = model.descriptor()
    if model.__dict__.get('_solver') is not None:
        model._solver.close()
    s = Solver(model._lib, desc, ndraw=1, keep_history=True)
    model.__dict__['_solver'] = s
    s.set_params(model.param_vector())
    if dbgout:
        s.set_dbgout(True)
    rc = s.solve(raise_on_error=False)
    sol = s.solution(0)
    if dbgout:
        sol.dbgout, sol.dbgn = s.dbgout(0)
    if rc:
        # the reference warns and returns the partially filled cells (egdst_solver.c:237)
        import warnings
        warnings.warn(sol.err)
    return sol


def _cells_stamp(M, D):
    """A cheap fingerprint of the cell arrays (shape and the bytes of the first, middle and last entry of every cell), so that a cell
    REPLACED inside model.M / model.D -- which keeps the outer objects -- is noticed and the cells are uploaded again: the reference
    reads them from the model object on every call.  (Bytes, not floats: a NaN entry must compare equal to itself.)"""
    out = []
    for cells in (M, D):
        for row in cells:
            for c in row:
                if c is None:
                    out.append(None)
                    continue
                a = np.asarray(c)
                n = a.size
                out.append((a.shape, a.flat[[0, n // 2, n - 1]].tobytes() if n else b''))
    return tuple(out)


def _solver_with_solution(model):
    """The handle that serves `sim` and `call`.  The reference's gateways take the solution from the model object on every
    call (egdst_simulator.c:61-68, egdst_call.c:28-34), not from the solve that produced it: when the handle of the last
    `solve` still holds exactly model.M / model.D it is reused (nothing to upload), otherwise -- the cells were assigned,
    e.g. restored from a saved model -- a fresh handle imports them (egdst_set_cell_M / egdst_set_cell_D)."""
    if model.M is None or model.D is None:
        raise EgdstRuntimeError(40, 'Error: the model has not yet been solved!')
    s = model.__dict__.get('_solver')
    held = model.__dict__.get('_solver_cells')   # the very objects the live handle holds (strong references: an id can be reused)
    if s is not None and held is not None and held[0] is model.M and held[1] is model.D and held[2] == _cells_stamp(model.M, model.D):
        s.set_params(model.param_vector())   # loadparameters() of the gateways: the CURRENT values (after a setparam too)
        return s
    if s is not None:
        s.close()
    s = Solver(model._lib, model.descriptor(), ndraw=1, keep_history=True)
    s.set_params(model.param_vector())   # (loadparameters() of the gateways: the CURRENT parameter values)
    s.set_cells(model.M, model.D, draw=0)
    model.__dict__['_solver'] = s
    model.__dict__['_solver_cells'] = (model.M, model.D, _cells_stamp(model.M, model.D))
    return s


def call_model(model, sw, args):
    return _solver_with_solution(model).call(sw, args, draw=0)


def policy_model(model, it, ist, cash):
    """(c, id, vf) of the model's current solution at the points (it, ist, cash), it and ist 0-based: one draw through
    egdst_policy_batch"""
    from . import datafit
    s = _solver_with_solution(model)
    obs = datafit.Observations(it, ist, cash)
    out = s.policy_batch(obs, want=('cons', 'id', 'vf'))
    return out['cons'][0].cpu().numpy(), out['id'][0].cpu().numpy(), out['vf'][0].cpu().numpy()


def simulate_model(model, rndtype):
    return _solver_with_solution(model).simulate(model.init, model.randstream, rndtype, draw=0)
