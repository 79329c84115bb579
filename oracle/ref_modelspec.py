"""Writer of ``modelspec.c`` / ``modelspec.h`` for the REFERENCE's model interface (TEST INFRASTRUCTURE).

The reference solver, simulator and accessor are compiled against a per-model pair of C files that supplies the user's
model functions with process globals for the parameters.  This module writes that pair from the same executable strings
(``egdst_amd/examples.py``) the product's plugin is generated from, so that the reference's own C can be built and run
(``oracle/build_ref.py``).  It is a second, independent path from the user's strings to C: it shares only the tokenizer
with ``egdst_amd/codegen.py``; what a token becomes is decided here, by what the reference's four C files call and read:

  PeriodVars            fields it, ist, id, cash, savings, shock, st[], dc[]
  NREQ                  number of equations (the simulator sizes an array with it)
  globals               one ``double`` per parameter, ``stgrids[]`` (grids of continuous states)
  loadparameters()      parameters from Model.param(k).value
  loadcontinuousgrid()  grids from Model.s(k).grid
  feasible inchoiceset utility utility_marginal utility_marginal_inverse discount survival tr trinv
  cashinhand cashinhand_marginal mu_param sigma_param trpr(curr,next,all) trpr_cont eqs_sim(curr,next|NULL,out)

States and decisions are read by index from the tables, or by value from the period's own st[]/dc[] when the library's
``byval`` global is set (the simulator sets it for models with continuous states).  The output is written under
``oracle/_ref/<tag>/`` and never committed.
"""
import hashlib
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from egdst_amd.codegen import _TOK, _lines, CodegenError  # noqa: E402

_LIBM = {'log', 'exp', 'pow', 'sqrt', 'fabs', 'floor', 'ceil', 'fmin', 'fmax', 'log1p', 'expm1', 'tanh', 'sin', 'cos',
         'atan', 'erf', 'erfc', 'fmod', 'isfinite', 'isnan', 'INFINITY', 'NAN'}
_C_WORDS = {'return', 'if', 'else', 'for', 'while', 'int', 'double', 'float', 'const', 'static', 'switch', 'case',
            'break', 'default', 'do', 'long', 'unsigned', 'void', 'sizeof'}
_LIB_GLOBALS = {'t0', 'T', 'ngridm', 'ngridmax', 'nthrhmax', 'ny', 'nd', 'nnd', 'nst', 'nnst', 'mmax', 'a0'}
_LOCALS = {'consumption', 'mutility', 'x'}


class _Rewrite:
    def __init__(self, m):
        self.m = m
        self.params = {p.ref for p in m.param}
        self.coefs = {c.ref for c in m.coef}
        self.eqs = {e.ref: e for e in m.eq}

    def __call__(self, text, two_periods, where, banned=()):
        for b in banned:
            if re.search(r'\b' + b + r'\d*\b', text, flags=re.IGNORECASE):
                raise CodegenError('`%s` may not be used in %s' % (b, where))
        m = self.m

        def nxt(tok):
            if not two_periods:
                raise CodegenError('`%s` needs the next period, which %s does not have' % (tok, where))

        def sub(mo):
            if mo.group('num') or mo.group('str'):
                return mo.group(0)
            t = mo.group('id')
            simple = {'min': 'MIN', 'max': 'MAX', 'true': '1', 'false': '0', 'it': 'curr->it', 'age': '(curr->it+t0)',
                      'id': 'curr->id', 'ist': 'curr->ist', 'cash': 'curr->cash', 'discount': 'discount(curr)',
                      'survival': 'survival(curr)'}
            if t in simple:
                return simple[t]
            two = {'ist1': 'next->ist', 'savings': 'next->savings', 'shock': 'next->shock',
                   'sigma': 'sigma_param(curr,next)', 'mu': 'mu_param(curr,next)'}
            if t in two:
                nxt(t)
                return two[t]
            mm = re.fullmatch(r'dc(\d+)', t)
            if mm and 1 <= int(mm.group(1)) <= m.nnd:
                k = int(mm.group(1)) - 1
                return '(byval>0?curr->dc[%d]:decisions[curr->id+%d*nd])' % (k, k)
            mm = re.fullmatch(r'st(\d+)(n?)', t)
            if mm and 1 <= int(mm.group(1)) <= m.nnst:
                k = int(mm.group(1)) - 1
                who = 'next' if mm.group(2) else 'curr'
                if mm.group(2):
                    nxt(t)
                return '(byval>0?%s->st[%d]:states[%s->ist+%d*nst])' % (who, k, who, k)
            if t in self.eqs:
                if self.eqs[t].type == 'next':
                    nxt(t)
                    return '%s(curr,next)' % t
                return '%s(curr)' % t
            if t in self.params or t in self.coefs or t in _LIB_GLOBALS or t in _LIBM or t in _C_WORDS or t in _LOCALS:
                return t
            raise CodegenError('Unknown identifier `%s` in %s: %s' % (t, where, text))

        return _TOK.sub(sub, text)


def generate(model):
    """(text of modelspec.h, text of modelspec.c) for ``model``."""
    m = model
    rw = _Rewrite(m)
    H, S = [], []
    h, c = H.append, S.append
    sizes = [int(v) for v in m.stm[:m.nnst]]
    strides = [int(v) for v in m.stm[m.nnst:]]
    cont = [k for k, v in enumerate(m.s) if v.type == 'continuous']

    h('#ifndef REF_MODELSPEC_H')
    h('#define REF_MODELSPEC_H')
    h('typedef struct ref_period {int it; int ist; int id; double cash; double savings; double shock; '
      'double st[%d]; double dc[%d];} PeriodVars;' % (max(m.nnst, 1), max(m.nnd, 1)))
    h('#define NREQ %d' % len(m.eq))
    h('extern double *stgrids[%d];' % max(m.nnst, 1))
    for p in m.param:
        h('extern double %s;' % p.ref)
    c('#include "egdst_lib.h"')
    c('double *stgrids[%d];' % max(m.nnst, 1))
    for p in m.param:
        c('double %s;' % p.ref)
    for co in m.coef:
        r, cc = co.array.shape       # padded so that the user's base-1 indices work
        rows = ['{' + ','.join(['0.0'] * (cc + 1)) + '}']
        rows += ['{0.0,' + ','.join('%.15f' % v for v in co.array[i]) + '}' for i in range(r)]
        c('static const double %s[%d][%d] = {%s};' % (co.ref, r + 1, cc + 1, ','.join(rows)))

    def fn(sig, expr, two, where, banned=()):
        h(sig + ';')
        c(sig + ' {')
        if isinstance(expr, str):
            c('  return ' + rw(expr, two, where, banned) + ';')
        else:
            for ln in _lines(expr):
                c('  ' + rw(ln, two, where, banned))
        c('}')

    P1, P2 = 'PeriodVars *curr', 'PeriodVars *curr, PeriodVars *next'
    for e in m.eq:
        h('double %s(%s);' % (e.ref, P2 if e.type == 'next' else P1))
    h('void loadparameters(void);')
    c('void loadparameters(void) {')
    for k, p in enumerate(m.param):
        c('  %s = mxGetScalar(mxGetField(mxGetProperty(Model, 0, "param"), %d, "value"));' % (p.ref, k))
    c('}')
    h('void loadcontinuousgrid(void);')
    c('void loadcontinuousgrid(void) {')
    for k in cont:
        c('  stgrids[%d] = mxGetPr(mxGetField(mxGetProperty(Model, 0, "s"), %d, "grid"));' % (k, k))
    c('}')
    fn('double discount(%s)' % P1, m.discount, False, 'discount', ('id', 'dc', 'cash'))
    fn('double survival(%s)' % P1, m.survival, False, 'survival', ('id', 'dc', 'cash'))
    fn('double utility(%s, double consumption)' % P1, m.u['utility'], False, 'utility', ('cash',))
    fn('double utility_marginal(%s, double consumption)' % P1, m.u['marginal'], False, 'marginal utility', ('cash',))
    fn('double utility_marginal_inverse(%s, double mutility)' % P1, m.u['marginalinverse'], False,
       'inverse marginal utility', ('cash',))
    tb = ('id', 'dc', 'cash', 'savings', 'shock')
    fn('double tr(%s, double x)' % P1, m.transform['direct'], False, 'transform', tb)
    fn('double trinv(%s, double x)' % P1, m.transform['inverse'], False, 'inverse transform', tb)
    fn('double mu_param(%s)' % P2, m.shock['mu'], True, 'shock mu', ('shock',))
    fn('double sigma_param(%s)' % P2, m.shock['sigma'], True, 'shock sigma', ('shock',))
    for e in m.eq:
        fn('double %s(%s)' % (e.ref, P2 if e.type == 'next' else P1), e.expression, e.type == 'next', 'equation ' + e.ref)
    fn('double cashinhand(%s)' % P2, m.budget['cashinhand'], True, 'budget', ('cash',))
    fn('double cashinhand_marginal(%s)' % P2, m.budget['marginal'], True, 'marginal budget', ('cash',))

    def rules(sig, default, rule_list, where, banned):
        h(sig + ';')
        c(sig + ' {')
        c('  int r = %d;' % int(default))
        for r in rule_list:
            c('  if (%s) r = %d;' % (rw(r['condition'], False, where, banned), int(not default)))
        c('  return r;')
        c('}')

    rules('int inchoiceset(%s)' % P1, m.choiceset['defaultallow'], m.choiceset['rules'], 'choice set', ('cash',))
    rules('int feasible(%s)' % P1, m.feasible['defaultfeasible'], m.feasible['rules'], 'feasibility',
          ('id', 'dc', 'cash'))

    # transition probability of the state index; all != 0 adds the interpolation weights of the continuous states
    h('double trpr(%s, int all);' % P2)
    c('double trpr(%s, int all) {' % P2)
    c('  double p = 1.0, nv; int i0, i1; (void)nv; (void)all;')
    for tr in m.trpr:
        k = tr.varindex - 1
        n = sizes[k]
        c('  i0 = (curr->ist/%d)%%%d; i1 = (next->ist/%d)%%%d;' % (strides[k], n, strides[k], n))
        for j, case in enumerate(tr.cases):
            c('  %sif (%s) {' % ('else ' if j else '', rw(case.condition, True, 'transition condition')))
            if k not in cont:
                c('    switch (i0*%d+i1) {' % n)
                for a in range(n):
                    for b in range(n):
                        c('    case %d: p *= %s; break;' % (a * n + b, rw(case.prob[a][b], True, 'transition probability')))
                c('    default: mexErrMsgTxt("modelspec: state index outside the table of state variable %d"); break;' % (k + 1))
                c('    }')
            else:
                g = 'stgrids[%d]' % k
                c('    if (all) {')
                c('      nv = %s;' % rw(case.prob, True, 'motion rule', ('ist1',)))
                c('      i0 = bxsearch(nv, %s, %d);' % (g, n))
                c('      if (i0 == i1) p *= (%s[i0+1]-nv)/(%s[i0+1]-%s[i0]);' % (g, g, g))
                c('      else if (i0+1 == i1) p *= (nv-%s[i0])/(%s[i0+1]-%s[i0]);' % (g, g, g))
                c('      else return 0.0;')
                c('    }')
            c('  }')
        c('  else mexErrMsgTxt("modelspec: no transition case applies to state variable %d");' % (k + 1))
        c('  if (p == 0.0) return 0.0;')
    c('  return p;')
    c('}')
    h('void trpr_cont(%s);' % P2)
    c('void trpr_cont(%s) {' % P2)
    for tr in m.trpr:
        k = tr.varindex - 1
        if k not in cont:
            continue
        for j, case in enumerate(tr.cases):
            c('  %sif (%s) next->st[%d] = %s;' % ('else ' if j else '', rw(case.condition, True, 'transition condition'), k,
                                                rw(case.prob, True, 'motion rule')))
    c('}')
    h('void eqs_sim(%s, double *out);' % P2)
    c('void eqs_sim(%s, double *out) {' % P2)
    c('  int n = 0; (void)n; (void)out;')
    for e in m.eq:
        if e.type == 'next':
            c('  out[n++] = next ? %s(curr,next) : mxGetNaN();' % e.ref)
        else:
            c('  out[n++] = %s(curr);' % e.ref)
    c('}')
    h('#endif')
    return '\n'.join(H) + '\n', '\n'.join(S) + '\n'


def defines(model):
    """Preprocessor definitions of the build: the shock family and the model's own flags."""
    d = ['-DDISTRIB=%d' % (1 if model.shock['type'] == 'lognormal' else 2)]
    for k, v in model.cflags.items():
        d.append('-D%s=%s' % (k, v))
    return d


def tag(model):
    hdr, src = generate(model)
    key = hashlib.sha1((hdr + src + ' '.join(defines(model))).encode()).hexdigest()[:12]
    return ''.join(ch for ch in model.label if ch.isalnum())[:16] + '_' + key
