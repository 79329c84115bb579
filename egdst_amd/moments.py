"""User-defined simulated moments for the estimation step (egdst_simulate_batch_spec, include/egdst.h).

    from egdst_amd import moments as mo
    spec = mo.MomentSpec([mo.share('id', k, periods=it) for it in range(nt) for k in range(3)]
                         + [mo.mean('C', periods=(0, 9), where=('id', 2, 2)), mo.cross('M', 'C')], layout=solver.lib.info)
    spec += [mo.median('M', periods=it) for it in range(nt)] + [mo.quantile('A', 0.9, where=('id', 1, 1))]
    means, counts, obj = solver.simulate_batch_spec(init, spec, target=t, W=W)
    data_means, data_counts = spec.evaluate(data_panel)      # the same definitions, summed in the same order, on the host
    # the covariance of the moments: per draw on the device, and of the data panel on the host, which is the Omega a user
    # inverts into W.  A quantile needs a bandwidth for it (the spacing estimate of the density at the quantile)
    h = mo.quantile_bandwidth(0.5, nsim)
    banded = mo.MomentSpec(spec[:-nt - 1] + [mo.median('M', periods=it, bandwidth=h) for it in range(nt)], layout=solver.lib.info)
    means, counts, cov = solver.simulate_batch_cov(init, banded)          # cov [ndraw, nmom, nmom]
    data_means, data_counts, data_cov = banded.covariance(data_panel, parts=solver.lib.cov_parts)

Columns are 0-based indices of the simulated panel (egdst_simulate, model.sims) or the tokens of the model strings:
M C A V id ist mu sigma shock u df, then st1.. (nnst states), dc1.. (nnd decisions), eq1.. (neq equations).  `periods` is
a 0-based model period or an inclusive (first, last) pair; None pools every period.  `where=(col, lo, hi)` keeps the
(agent, period) pairs with lo <= sims[col] <= hi.

Moments across two periods (egdst_moment_lag, egdst_simulate_batch_spec_lag): a lag counts periods back (> 0) or ahead (< 0).
`where=(col, lo, hi, lag)` reads the condition in period it - lag, `cross(col, col2, lag=k)` multiplies sims[col] in period it
by sims[col2] in period it - k, and `transition(col, frm, to)` is the share moving to `to` among those who were at `frm` a
period earlier:

    spec = mo.MomentSpec([mo.transition('id', 1, 0, periods=it) for it in range(1, nt)]       # a hazard by age
                         + [mo.cross('C', 'C', lag=1), mo.mean('C', where=('id', 0, 0, -1))], layout=solver.lib.info)

A pair counts only if every value it reads is present in its own period (NaN never qualifies), so an agent that is dead or
not yet valued in the other period drops out.  With a lag, `periods=None` pools every period for which the other periods
exist, first = max(0, lags in use) to last = nt - 1 + min(0, lags in use); an explicit range that reaches outside raises
ValueError: nothing is clipped.  A spec with a lag packs with pack_lag (MOMENT_LAG_DTYPE, 64 bytes); pack() refuses it.

A quantile (kind 3) is an order statistic, not an interpolation: of the n qualifying values the k-th smallest,
k = ceil(p * n) clamped to [1, n], in the total order of the keys of `quantile_keys` (-0.0 before +0.0); the median of an even
n is the lower middle value.  The device selects it exactly, so `evaluate` returns the same bits for every block size.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

# egdst_moment: 6 ints, then 4 doubles (56 bytes, no padding)
MOMENT_DTYPE = np.dtype([('kind', '<i4'), ('col', '<i4'), ('col2', '<i4'), ('it_first', '<i4'), ('it_last', '<i4'),
                         ('cond_col', '<i4'), ('lo', '<f8'), ('hi', '<f8'), ('cond_lo', '<f8'), ('cond_hi', '<f8')])

# egdst_moment_lag: the fields of egdst_moment, then the two lags (64 bytes, no padding)
MOMENT_LAG_DTYPE = np.dtype(MOMENT_DTYPE.descr + [('lag2', '<i4'), ('cond_lag', '<i4')])

BASE_COLUMNS = ['M', 'C', 'A', 'V', 'id', 'ist', 'mu', 'sigma', 'shock', 'u', 'df']
MEAN, CROSS, SHARE, QUANTILE = 0, 1, 2, 3


def columns(nnst, nnd, neq):
    """the names of the simulated columns, in order"""
    return BASE_COLUMNS + ['st%d' % (k + 1) for k in range(nnst)] + ['dc%d' % (k + 1) for k in range(nnd)] + \
        ['eq%d' % (k + 1) for k in range(neq)]


def _layout(layout):
    """(nnst, nnd, neq) of a library's model info, a Solver / ModelLibrary, a model, or a tuple"""
    if layout is None:
        return None
    for attr in ('lib', 'info'):   # Solver -> ModelLibrary -> EgdstModelInfo
        if not hasattr(layout, 'nnst') and hasattr(layout, attr):
            layout = getattr(layout, attr)
    if hasattr(layout, 'nnst'):   # (a model object counts its equations in _eq)
        neq = layout.neq if hasattr(layout, 'neq') else len(layout._eq)
        return int(layout.nnst), int(layout.nnd), int(neq)
    nnst, nnd, neq = (int(x) for x in layout)
    return nnst, nnd, neq


@dataclass(frozen=True)
class Moment:
    kind: int
    col: object
    col2: object = None
    periods: object = None
    where: object = None
    lo: float = 0.0
    hi: float = 0.0
    lag: int = 0   # (of col2, kind 1 only; a condition's lag is the fourth entry of `where`)


def mean(col, periods=None, where=None):
    """mean of sims[col]"""
    return Moment(MEAN, col, periods=periods, where=where)


def cross(col, col2, periods=None, where=None, lag=0):
    """mean of sims[col] * sims[col2] over the pairs where both are present (E[x^2] with col2 = col); col2 is read `lag`
    periods before col (after it with lag < 0): cross('C', 'C', lag=1) is E[C_t * C_t-1]"""
    return Moment(CROSS, col, col2, periods=periods, where=where, lag=lag)


def share(col, lo, hi=None, periods=None, where=None):
    """share of the present values of sims[col] in [lo, hi] (hi = lo when not given): share('id', k) is choice k's share"""
    return Moment(SHARE, col, periods=periods, where=where, lo=float(lo), hi=float(lo if hi is None else hi))


def transition(col, frm, to, periods=None, lag=1):
    """share of the present values of sims[col] equal to `to` among the pairs whose sims[col] was `frm` `lag` periods before:
    share(col, to, where=(col, frm, frm, lag)).  transition('id', 0, 1, periods=it) is the hazard of choice 1 in period it."""
    return share(col, to, periods=periods, where=(col, frm, frm, lag))


def quantile(col, p, periods=None, where=None, bandwidth=None):
    """quantile p (0 < p < 1) of the present values of sims[col]: the ceil(p n)-th smallest of the n, no interpolation.
    bandwidth: the h of the spacing estimate of the density at the quantile (0 < p - h, p + h < 1; quantile_bandwidth gives the
    usual choices), which the covariance needs and nothing else reads; None: the record carries none and has no covariance"""
    return Moment(QUANTILE, col, periods=periods, where=where, lo=float(p), hi=0.0 if bandwidth is None else float(bandwidth))


def median(col, periods=None, where=None, bandwidth=None):
    """quantile(col, 0.5): the lower middle value of an even number of values"""
    return quantile(col, 0.5, periods=periods, where=where, bandwidth=bandwidth)


def bandwidth_problem(p, h):
    """why the library refuses bandwidth h on a quantile p (the rules of egdst_simulate_batch_spec_cov, on the rounded fp64 sum and
    difference), or None; h == 0.0 is no bandwidth at all, which only the covariance refuses"""
    p, h = float(p), float(h)
    if h == 0.0:
        return None
    if not h > 0.0:   # (NaN fails too)
        return 'is NaN or not positive'
    if p - h <= 0.0:
        return 'reaches p - h <= 0'
    if p + h >= 1.0:
        return 'reaches p + h >= 1'
    return None


def quantile_bandwidth(p, n, rule='bofinger'):
    """the usual bandwidth h of the spacing estimate for quantile p of n values: 'bofinger',
    h = n^(-1/5) (4.5 phi(z)^4 / (2 z^2 + 1)^2)^(1/5), or 'hall-sheather',
    h = n^(-1/3) z_0.975^(2/3) (1.5 phi(z)^2 / (2 z^2 + 1))^(1/3), with z the normal quantile of p and phi the normal density;
    clipped to what a record accepts (p - h > 0 and p + h < 1 as rounded).  A convenience: no bit contract."""
    from statistics import NormalDist
    p, n = float(p), float(n)
    if not 0.0 < p < 1.0:
        raise ValueError('quantile_bandwidth: p = %r is outside (0, 1)' % p)
    if not n >= 1.0:
        raise ValueError('quantile_bandwidth: n = %r is not a number of values' % n)
    nd = NormalDist()
    z = nd.inv_cdf(p)
    f = nd.pdf(z)
    if rule == 'bofinger':
        h = n ** -0.2 * (4.5 * f ** 4 / (2.0 * z * z + 1.0) ** 2) ** 0.2
    elif rule == 'hall-sheather':
        h = n ** (-1.0 / 3.0) * nd.inv_cdf(0.975) ** (2.0 / 3.0) * (1.5 * f * f / (2.0 * z * z + 1.0)) ** (1.0 / 3.0)
    else:
        raise ValueError('quantile_bandwidth: rule %r is neither \'bofinger\' nor \'hall-sheather\'' % (rule,))
    h = min(h, 0.5 * min(p, 1.0 - p))   # (half the distance to the nearer end; then down until the rounded ends are inside)
    while h > 0.0 and bandwidth_problem(p, h):
        h = math.nextafter(h, 0.0)
    if not h > 0.0:
        raise ValueError('quantile_bandwidth: no bandwidth fits p = %r' % p)
    return h


def quantile_keys(x):
    """the uint64 keys whose unsigned order is the order of the quantiles (include/egdst.h): bits u -> ~u if the sign bit is
    set, else u | 1 << 63"""
    u = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    return np.where(u >> np.uint64(63) != 0, ~u, u | np.uint64(1 << 63))


def quantile_rank(p, n):
    """1-based rank of quantile p among n >= 1 values: ceil of the one fp64 product p * n, clamped to [1, n]"""
    return min(max(int(math.ceil(float(p) * float(n))), 1), int(n))


def _key_value(key):
    """the double whose quantile key is `key` (the inverse of quantile_keys on one key)"""
    key = np.uint64(key)
    u = key & np.uint64((1 << 63) - 1) if key >> np.uint64(63) else ~key
    return np.array([u], dtype=np.uint64).view(np.float64)[0]


def _sparsity(skeys, p, h):
    """(a, b, s) of the contract of egdst_simulate_batch_spec_cov from the sorted keys of the n qualifying values: the order
    statistics of ranks k_lo = quantile_rank(p - h, n) and k_hi = quantile_rank(p + h, n), and the sparsity
    s = (b - a) / ((double)(k_hi - k_lo) / (double)n), one difference and two quotients; n = 0: all NaN"""
    n = len(skeys)
    if n == 0:
        return np.nan, np.nan, np.nan
    p, h = np.float64(p), np.float64(h)
    k_lo, k_hi = quantile_rank(p - h, n), quantile_rank(p + h, n)
    a, b = _key_value(skeys[k_lo - 1]), _key_value(skeys[k_hi - 1])
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        s = (b - a) / (np.float64(k_hi - k_lo) / np.float64(n))
    return a, b, s


def quantile_band(x, p, h):
    """(a, b, s): the order statistics Q(p - h) and Q(p + h) of the non-NaN values of x and the sparsity
    s = (b - a) / ((k_hi - k_lo) / n), the spacing estimate of 1 / f at quantile p (Siddiqui; Bloch and Gastwirth), as
    k_quantile_band forms it: mask, sort the keys, index.  The mirror of ModelLibrary.quantile_band_eval, bit for bit; all NaN
    when no value qualifies, s NaN when the two ranks coincide.  ValueError on a p or a bandwidth the library refuses."""
    p, h = float(p), float(h)
    if not 0.0 < p < 1.0:
        raise ValueError('quantile_band: p = %r is outside (0, 1)' % p)
    why = 'is missing' if h == 0.0 else bandwidth_problem(p, h)
    if why:
        raise ValueError('quantile_band: the bandwidth %r of quantile %r %s' % (h, p, why))
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
    return _sparsity(np.sort(quantile_keys(x[~np.isnan(x)])), p, h)


def convert_records(rec, dtype):
    """rec, an array of MOMENT_DTYPE or MOMENT_LAG_DTYPE, as a contiguous [nmom] array of `dtype` (one of the two): an
    egdst_moment widens with zero lags, an egdst_moment_lag narrows once its lags are seen to be zero (ValueError if not)"""
    src = MOMENT_LAG_DTYPE if getattr(rec, 'dtype', None) == MOMENT_LAG_DTYPE else MOMENT_DTYPE
    rec = np.ascontiguousarray(rec, dtype=src).reshape(-1)
    if src == dtype:
        return rec
    if dtype == MOMENT_DTYPE and (rec['lag2'].any() or rec['cond_lag'].any()):
        raise ValueError('a moment has a lag, which egdst_moment cannot carry')
    out = np.zeros(len(rec), dtype=dtype)   # (zero lags)
    for f in MOMENT_DTYPE.names:
        out[f] = rec[f]
    return out


def lag_records(spec, nt, layout=None):
    """(rec, lag): what a caller may pass as moments -- a MomentSpec, an array of MOMENT_DTYPE or one of MOMENT_LAG_DTYPE -- as
    an [nmom] array of MOMENT_LAG_DTYPE, and whether it needs the entry that takes those (egdst_simulate_batch_spec_lag): a
    MomentSpec with a lag or an array of MOMENT_LAG_DTYPE does, and then rec goes as it is; otherwise
    convert_records(rec, MOMENT_DTYPE) is what egdst_simulate_batch_spec takes."""
    if isinstance(spec, MomentSpec):
        return spec.pack_lag(nt, layout), spec.lagged
    return convert_records(spec, MOMENT_LAG_DTYPE), getattr(spec, 'dtype', None) == MOMENT_LAG_DTYPE


def _moment_term(sims, q):
    """(ok, x), both [nsim, periods of q]: the host's eg_moment_term -- which (agent, period) pairs of the panel qualify for
    the packed MOMENT_LAG_DTYPE record q, and with which value: v, v * w, or the share's 1.0 / 0.0 (a quantile: v).  The
    condition is read cond_lag periods away, the second factor lag2 periods away, and each must be present there."""
    f, l_ = int(q['it_first']), int(q['it_last']) + 1
    v = sims[:, f:l_, q['col']]
    ok = ~np.isnan(v)
    with np.errstate(invalid='ignore'):
        if q['cond_col'] >= 0:
            c = sims[:, f - int(q['cond_lag']):l_ - int(q['cond_lag']), q['cond_col']]   # (pack_lag: inside the panel)
            ok &= (c >= q['cond_lo']) & (c <= q['cond_hi'])
        if q['kind'] == CROSS:
            w = sims[:, f - int(q['lag2']):l_ - int(q['lag2']), q['col2']]
            ok &= ~np.isnan(w)
            x = v * w
        elif q['kind'] == SHARE:
            x = ((v >= q['lo']) & (v <= q['hi'])).astype(np.float64)
        else:
            x = v
    return ok, x


class MomentSpec(list):
    """A list of Moment records, resolved against a model's column layout (`layout`: the library's model info, a Solver, a
    ModelLibrary, a model, or (nnst, nnd, neq)).  pack(nt) gives the egdst_moment array, pack_lag(nt) the egdst_moment_lag array (a
    spec with a lag has only that one); evaluate(sims) the moments of a host panel."""

    def __init__(self, items=(), layout=None):
        super().__init__(items)
        self.layout = _layout(layout)

    def names(self, layout=None):
        lay = _layout(layout) or self.layout
        if lay is None:
            raise ValueError('MomentSpec: no column layout (pass layout=(nnst, nnd, neq) or the library)')
        return columns(*lay)

    @staticmethod
    def _col(c, names, what):
        """index of column c; names None: no layout, so only the base tokens resolve and the upper bound is left to the
        library (or to evaluate, which knows the panel)"""
        if isinstance(c, str):
            if c in (names or BASE_COLUMNS):
                return (names or BASE_COLUMNS).index(c)
            if names is None and c[:2] in ('st', 'dc', 'eq'):
                raise ValueError('MomentSpec: column %r of %s needs a layout (layout=(nnst, nnd, neq) or the library)' % (c, what))
            raise ValueError('MomentSpec: unknown column %r of %s (columns: %s)' % (c, what, ' '.join(names or BASE_COLUMNS)))
        if isinstance(c, (bool, np.bool_)) or not isinstance(c, (int, np.integer)):
            raise ValueError('MomentSpec: column %r of %s is neither a name nor an index' % (c, what))
        if c < 0 or names is not None and c >= len(names):
            raise ValueError('MomentSpec: column %d of %s is outside [0, %s)' % (c, what, len(names) if names else 'nout'))
        return int(c)

    @staticmethod
    def _lag(x, what):
        if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, np.integer)):
            raise ValueError('MomentSpec: lag %r of %s is not an integer number of periods' % (x, what))
        return int(x)

    @property
    def lagged(self):
        """does a moment read a second period (a non-zero lag on col2 or on the condition)?"""
        return any(isinstance(q, Moment) and (q.lag != 0 or q.where is not None and len(q.where) == 4 and q.where[3] != 0)
                   for q in self)

    def pack(self, nt, layout=None):
        """[nmom] array of MOMENT_DTYPE; raises ValueError on a bad name, kind, column or period range, and on a spec with a
        lag: that one packs with pack_lag"""
        if self.lagged:
            raise ValueError('MomentSpec: a moment has a lag, which egdst_moment cannot carry: use pack_lag')
        return convert_records(self.pack_lag(nt, layout), MOMENT_DTYPE)

    def pack_lag(self, nt, layout=None):
        """[nmom] array of MOMENT_LAG_DTYPE, with or without lags; raises ValueError on a bad name, kind, column, lag or
        period range: on everything the library refuses"""
        if len(self) == 0:
            raise ValueError('MomentSpec: no moments')
        lay = _layout(layout) or self.layout
        nm = None if lay is None else columns(*lay)
        out = np.zeros(len(self), dtype=MOMENT_LAG_DTYPE)
        for j, q in enumerate(self):
            what = 'moment %d' % j
            if not isinstance(q, Moment) or q.kind not in (MEAN, CROSS, SHARE, QUANTILE):
                raise ValueError('MomentSpec: %s is not a mean, cross, share or quantile' % what)
            col = self._col(q.col, nm, what)
            col2 = self._col(q.col2, nm, what) if q.kind == CROSS else col
            lag2 = self._lag(q.lag, what)
            if lag2 != 0 and q.kind != CROSS:
                raise ValueError('MomentSpec: %s has a lag but is not a cross (a condition\'s lag goes into where)' % what)
            cc, clo, chi, clag = -1, 0.0, 0.0, 0
            if q.where is not None:
                if len(q.where) not in (3, 4):
                    raise ValueError('MomentSpec: where of %s is not (col, lo, hi) or (col, lo, hi, lag)' % what)
                cc = self._col(q.where[0], nm, what)
                clo, chi = float(q.where[1]), float(q.where[2])
                if not clo <= chi:
                    raise ValueError('MomentSpec: where of %s has lo > hi' % what)
                if len(q.where) == 4:
                    clag = self._lag(q.where[3], what)
            lags = [lag2, clag]   # (0 where not in use: a lag of 0 moves neither end)
            if q.periods is None:   # every period for which the other periods exist
                f, l_ = max(0, *lags), nt - 1 + min(0, *lags)
                if f > l_:
                    raise ValueError('MomentSpec: with lags (%d, %d) %s has no period inside [0, %d)' % (lag2, clag, what, nt))
            elif isinstance(q.periods, (int, np.integer)) and not isinstance(q.periods, bool):
                f = l_ = int(q.periods)
            else:
                try:
                    f, l_ = (int(x) for x in q.periods)
                except (TypeError, ValueError):
                    raise ValueError('MomentSpec: periods %r of %s is neither a period nor a (first, last) pair'
                                     % (q.periods, what)) from None
            if not 0 <= f <= l_ < nt:
                raise ValueError('MomentSpec: periods (%d, %d) of %s are empty or outside [0, %d)' % (f, l_, what, nt))
            for lag in lags:
                if f - lag < 0 or l_ - lag >= nt:
                    raise ValueError('MomentSpec: periods (%d, %d) of %s, read %d periods %s, leave [0, %d)'
                                     % (f, l_, what, abs(lag), 'back' if lag > 0 else 'ahead', nt))
            if q.kind == SHARE and not q.lo <= q.hi:
                raise ValueError('MomentSpec: share %s has lo > hi' % what)
            if q.kind == QUANTILE and not 0.0 < q.lo < 1.0:   # (NaN fails both)
                raise ValueError('MomentSpec: quantile %s has p = %r outside (0, 1)' % (what, q.lo))
            if q.kind == QUANTILE and bandwidth_problem(q.lo, q.hi):
                raise ValueError('MomentSpec: the bandwidth %r of quantile %s (p = %r) %s'
                                 % (q.hi, what, q.lo, bandwidth_problem(q.lo, q.hi)))
            out[j] = (q.kind, col, col2, f, l_, cc, q.lo, q.hi, clo, chi, lag2, clag)
        return out

    def evaluate(self, sims, block=256, layout=None):
        """(means [nmom], counts [nmom]) of a host panel sims [nsim, nt, nout] (NaN = missing) with the definitions and the
        summation order of the device (include/egdst.h): per partial t < block the agents i = t (mod block) in ascending i,
        periods ascending within an agent, then the fixed tree over the partials.  block=256 is the GPU's.  A quantile is
        the key of rank quantile_rank(p, n) among the sorted keys of the qualifying values, whatever the block.  A lagged
        condition or second factor is read in period it - lag and must be present there."""
        sims = np.asarray(sims, dtype=np.float64)
        if sims.ndim != 3:
            raise ValueError('MomentSpec.evaluate: sims must be [nsim, nt, nout]')
        if block < 1 or block & (block - 1):
            raise ValueError('MomentSpec.evaluate: block must be a power of two')
        nsim, nt, nout = sims.shape
        lay = _layout(layout) or self.layout
        if lay is not None and 11 + sum(lay) != nout:
            raise ValueError('MomentSpec.evaluate: the panel has %d columns, the layout %d' % (nout, 11 + sum(lay)))
        rec = self.pack_lag(nt, layout)
        if (rec['col'].max(initial=0) >= nout or rec['col2'].max(initial=0) >= nout or rec['cond_col'].max(initial=-1) >= nout):
            raise ValueError('MomentSpec.evaluate: a column is outside the panel\'s %d columns' % nout)
        nb = -(-nsim // block)
        means = np.empty(len(rec))
        counts = np.empty(len(rec), dtype=np.int64)
        for j, q in enumerate(rec):
            ok, x = _moment_term(sims, q)
            if q['kind'] == QUANTILE:
                n = int(ok.sum())
                counts[j] = n
                means[j] = np.nan
                if n:
                    key = np.sort(quantile_keys(x[ok]))[quantile_rank(q['lo'], n) - 1]
                    u = key & np.uint64((1 << 63) - 1) if key >> np.uint64(63) else ~key
                    means[j] = np.array([u], dtype=np.uint64).view(np.float64)[0]
                continue
            x = np.where(ok, x, 0.0)   # (adding +0.0 leaves a partial unchanged: it starts at +0.0 and never becomes -0.0)
            # partial t adds agents t, t+block, ... in order, each agent's periods in order: [block, nb * periods] rows
            xp = np.zeros((nb * block, x.shape[1]))
            xp[:nsim] = x
            rows = xp.reshape(nb, block, x.shape[1]).transpose(1, 0, 2).reshape(block, -1)
            p = np.cumsum(rows, axis=1)[:, -1].copy() if rows.shape[1] else np.zeros(block)
            n = ok.sum()
            o = block // 2
            while o > 0:
                p[:o] += p[o:2 * o]
                o //= 2
            counts[j] = n
            means[j] = p[0] / n if n else np.nan
        return means, counts

    def covariance(self, sims, block=256, parts=4, layout=None):
        """(means [nmom], counts [nmom], cov [nmom, nmom]) of a host panel sims [nsim, nt, nout]: the moments of
        evaluate(sims, block) and their agent-clustered covariance Omega with the definitions and the summation order of
        egdst_simulate_batch_spec_cov (include/egdst.h).  Agent i's score on record j is d_ij = (s_ij - m_j * c_ij) / N_j, with
        c_ij the agent's qualifying pairs and s_ij the sum of their values in period order; Omega_jk = sum over i of
        d_ij * d_ik: partial t < parts adds the rounded products of the agents i = t (mod parts) in ascending i, then the fixed
        tree over the partials.  parts = the library's cov_parts (4) gives the device's bits.  The row and column of an empty
        moment are NaN.  No degrees-of-freedom correction: nsim * cov estimates the asymptotic variance of the moment vector,
        and cov of a data panel is what a user inverts into W.  A quantile enters with the influence function of the sample
        quantile, (p - F(q)) / f(q), 1 / f estimated by the spacing of two order statistics (`scores`, quantile_band): it needs a
        bandwidth, and its row and column are NaN where the sparsity is.  Raises ValueError on a quantile without a bandwidth."""
        if parts < 1 or parts > 256 or parts & (parts - 1):
            raise ValueError('MomentSpec.covariance: parts must be a power of two in [1, 256]')
        means, counts, d = self.scores(sims, block=block, layout=layout)
        nsim, nmom = d.shape
        p = np.zeros((parts, nmom, nmom))
        with np.errstate(invalid='ignore'):
            for i0 in range(0, nsim, parts):   # one agent per partial and round: p_t = p_t + (d_ij * d_ik)
                r = d[i0:i0 + parts]
                p[:len(r)] += r[:, :, None] * r[:, None, :]
            o = parts // 2
            while o > 0:
                p[:o] += p[o:2 * o]
                o //= 2
        cov = p[0]
        upper = np.triu_indices(nmom, 1)
        cov.T[upper] = cov[upper]   # (Omega_kj carries the bits of Omega_jk)
        return means, counts, cov

    def scores(self, sims, block=256, layout=None):
        """(means [nmom], counts [nmom], d [nsim, nmom]): the moments of evaluate(sims, block) and every agent's score
        d_ij = (s_ij - m_j * c_ij) / N_j as covariance documents it -- the agent's contribution to moment j, whose cross
        products over the agents are Omega.  Elementwise IEEE operations: no summation order beyond an agent's own periods.
        A quantile with a bandwidth h has d_ij = (s_j * (p * c_ij - t_ij)) / N_j: t_ij the agent's qualifying pairs whose key is
        <= the key of the quantile q_j, s_j the sparsity of quantile_band on the record's qualifying values (a product, a
        difference, a product, a quotient); its column is NaN when s_j is (an empty record, or two ranks that coincide) and 0.0
        when the band lies inside a mass point.  Raises ValueError on a quantile without a bandwidth."""
        sims = np.asarray(sims, dtype=np.float64)
        if sims.ndim != 3:
            raise ValueError('MomentSpec.scores: sims must be [nsim, nt, nout]')
        rec = self.pack_lag(sims.shape[1], layout)
        for j, q in enumerate(rec):
            if q['kind'] == QUANTILE and q['hi'] == 0.0:
                raise ValueError('MomentSpec: moment %d is a quantile without a bandwidth, which has no covariance' % j)
        means, counts = self.evaluate(sims, block=block, layout=layout)
        nsim = sims.shape[0]
        d = np.empty((nsim, len(rec)))
        for j, q in enumerate(rec):
            ok, x = _moment_term(sims, q)
            if q['kind'] == QUANTILE:
                keys = quantile_keys(np.where(ok, x, 0.0))   # (the pairs that do not qualify are masked below)
                s = _sparsity(np.sort(keys[ok]), q['lo'], q['hi'])[2]
                c = ok.sum(axis=1).astype(np.float64)
                t = np.zeros(nsim)
                if counts[j]:
                    t = (ok & (keys <= quantile_keys(means[j:j + 1])[0])).sum(axis=1).astype(np.float64)
                with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
                    d[:, j] = (np.float64(s) * (q['lo'] * c - t)) / np.float64(counts[j])
                continue
            # s_ij: from 0.0, the qualifying values in period order (adding +0.0 for the others leaves the sum unchanged)
            s = np.cumsum(np.concatenate([np.zeros((nsim, 1)), np.where(ok, x, 0.0)], axis=1), axis=1)[:, -1]
            with np.errstate(invalid='ignore', divide='ignore'):
                d[:, j] = (s - means[j] * ok.sum(axis=1).astype(np.float64)) / np.float64(counts[j])
        return means, counts, d


def objective(means, counts, target, W):
    """e' W e in the device's order (k_moment_objective): e = means - target, r_j = sum over k ascending of the non-zero
    W_jk * e_k, obj = sum over j ascending of e_j * r_j over the rows with a non-zero entry; NaN if a moment W touches is
    empty.  means/counts [nmom] or [ndraw, nmom]; W [nmom, nmom] or a vector (its diagonal)."""
    means, counts = np.asarray(means, dtype=np.float64), np.asarray(counts)
    if means.ndim == 2:
        return np.array([objective(m, c, target, W) for m, c in zip(means, counts)])
    n = len(means)
    W = weight_matrix(W, n)
    e = means - np.asarray(target, dtype=np.float64).reshape(-1)
    nz = W != 0
    if np.any((counts == 0) & (nz.any(axis=0) | nz.any(axis=1))):
        return np.nan
    acc = 0.0
    for j in range(n):
        k = np.nonzero(nz[j])[0]
        if len(k):
            r = float(np.cumsum(W[j, k] * e[k])[-1])
            acc += float(e[j]) * r
    return acc


def weight_matrix(W, nmom):
    """W as a C-ordered [nmom, nmom] float64 matrix (a vector is its diagonal)"""
    W = np.asarray(W, dtype=np.float64)
    if W.ndim == 1:
        W = np.diag(W)
    if W.shape != (nmom, nmom):
        raise ValueError('W must be [%d, %d] or a vector of %d' % (nmom, nmom, nmom))
    return np.ascontiguousarray(W)
