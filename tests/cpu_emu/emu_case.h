// The case file of the stand-alone drivers (emu_main, emu_estimation_main), read in two parts:
//   solver part:     t0 T ngridm ngridmax nthrhmax ny mmax a0 nparam, then 2*ny quadrature, then the parameters
//   estimation part: nsim seed, init [nsim x 2] column-major, nmom, per record kind col col2 it_first it_last cond_col lo hi
//                    cond_lo cond_hi lag2 cond_lag, and optionally n, x[n], np, p[np] (for egdst_quantile_eval)
#pragma once
#include <cstdio>
#include <vector>
#include "../../include/egdst.h"

struct emu_case {
    egdst_desc d;   // (d.quadrature points into q: a case is not copied)
    std::vector<double> q, par;
    int nsim = 0;
    unsigned long long seed = 0;
    std::vector<double> init, x, p;
    std::vector<egdst_moment_lag> spec;
    emu_case() = default;
    emu_case(const emu_case &) = delete;
};

static bool emu_read_doubles(FILE *f, std::vector<double> &v)
{
    for (auto &x : v) if (fscanf(f, "%lf", &x) != 1) return false;
    return true;
}

static bool emu_read_solver_case(FILE *f, emu_case &c)
{
    egdst_desc &d = c.d;
    int npar;
    if (fscanf(f, "%d %d %d %d %d %d %lf %lf %d", &d.t0, &d.T, &d.ngridm, &d.ngridmax, &d.nthrhmax, &d.ny, &d.mmax, &d.a0, &npar) != 9) return false;
    if (d.ny < 0 || npar < 0) return false;
    c.q.resize(2 * (size_t)d.ny);
    c.par.assign(npar > 0 ? npar : 1, 0.0);
    if (!emu_read_doubles(f, c.q)) return false;
    for (int i = 0; i < npar; i++) if (fscanf(f, "%lf", &c.par[i]) != 1) return false;
    d.quadrature = c.q.data();
    return true;
}

static bool emu_read_estimation_case(FILE *f, emu_case &c)
{
    int nmom, n, np;
    if (fscanf(f, "%d %llu", &c.nsim, &c.seed) != 2 || c.nsim < 1) return false;
    c.init.resize(2 * (size_t)c.nsim);
    if (!emu_read_doubles(f, c.init)) return false;
    if (fscanf(f, "%d", &nmom) != 1 || nmom < 1) return false;
    c.spec.resize(nmom);
    for (auto &r : c.spec)
        if (fscanf(f, "%d %d %d %d %d %d %lf %lf %lf %lf %d %d", &r.kind, &r.col, &r.col2, &r.it_first, &r.it_last, &r.cond_col, &r.lo,
                   &r.hi, &r.cond_lo, &r.cond_hi, &r.lag2, &r.cond_lag) != 12) return false;
    if (fscanf(f, "%d", &n) != 1) return true;   // (no quantile evaluation)
    if (n < 1) return false;
    c.x.resize(n);
    if (!emu_read_doubles(f, c.x) || fscanf(f, "%d", &np) != 1 || np < 1) return false;
    c.p.resize(np);
    return emu_read_doubles(f, c.p);
}
