// Stand-alone driver of the sanitizer build for the quantile moments (the sanitizer's runtime is linked in, nothing is preloaded):
//   emu_quantile_main <case file>
// case file: t0 T ngridm ngridmax nthrhmax ny mmax a0 nparam, 2*ny quadrature, the parameters (as emu_main), then
//   nsim seed, init [nsim x 2] column-major, nmom, per record kind col col2 it_first it_last cond_col lo hi cond_lo cond_hi,
//   n, x[n], np, p[np]
// Solves one draw, runs the estimation step with generated uniforms on the records and egdst_quantile_eval on x; prints
//   moment <j> <count> <bits of the mean, hex>      and      eval <i> <count> <bits, hex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../include/egdst.h"

static unsigned long long bits(double x)
{
    unsigned long long u;
    memcpy(&u, &x, sizeof u);
    return u;
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    egdst_desc d;
    int npar;
    if (fscanf(f, "%d %d %d %d %d %d %lf %lf %d", &d.t0, &d.T, &d.ngridm, &d.ngridmax, &d.nthrhmax, &d.ny, &d.mmax, &d.a0, &npar) != 9) return 2;
    std::vector<double> q(2 * d.ny), par(npar > 0 ? npar : 1);
    for (auto &x : q) if (fscanf(f, "%lf", &x) != 1) return 2;
    for (int i = 0; i < npar; i++) if (fscanf(f, "%lf", &par[i]) != 1) return 2;
    d.quadrature = q.data();
    int nsim, nmom, n, np;
    unsigned long long seed;
    if (fscanf(f, "%d %llu", &nsim, &seed) != 2 || nsim < 1) return 2;
    std::vector<double> init(2 * (size_t)nsim);
    for (auto &x : init) if (fscanf(f, "%lf", &x) != 1) return 2;
    if (fscanf(f, "%d", &nmom) != 1 || nmom < 1) return 2;
    std::vector<egdst_moment> spec(nmom);
    for (auto &r : spec)
        if (fscanf(f, "%d %d %d %d %d %d %lf %lf %lf %lf", &r.kind, &r.col, &r.col2, &r.it_first, &r.it_last, &r.cond_col, &r.lo, &r.hi,
                   &r.cond_lo, &r.cond_hi) != 10) return 2;
    if (fscanf(f, "%d", &n) != 1 || n < 1) return 2;
    std::vector<double> x(n);
    for (auto &v : x) if (fscanf(f, "%lf", &v) != 1) return 2;
    if (fscanf(f, "%d", &np) != 1 || np < 1) return 2;
    std::vector<double> p(np);
    for (auto &v : p) if (fscanf(f, "%lf", &v) != 1) return 2;
    fclose(f);

    egdst_handle *h = nullptr;
    int rc = egdst_create(&d, 1, 1, nullptr, &h);
    if (rc) { printf("create rc=%d %s\n", rc, egdst_last_error()); return 1; }
    egdst_set_params(h, par.data(), 1);
    rc = egdst_solve(h);
    printf("solve rc=%d\n", rc);
    if (rc) return 1;
    std::vector<double> means(nmom), out(np);
    std::vector<int> counts(nmom);
    // (the harness has no device: the "device" buffers are host arrays)
    rc = egdst_simulate_batch_spec(h, init.data(), nsim, nullptr, 0, seed, 0, spec.data(), nmom, nullptr, nullptr, means.data(),
                                   counts.data(), nullptr);
    if (rc) { printf("spec rc=%d %s\n", rc, egdst_last_error()); return 1; }
    for (int j = 0; j < nmom; j++) printf("moment %d %d %016llx\n", j, counts[j], bits(means[j]));
    spec[0].lo = 1.0;   // refused before anything runs
    printf("refused rc=%d\n", egdst_simulate_batch_spec(h, init.data(), nsim, nullptr, 0, seed, 0, spec.data(), nmom, nullptr, nullptr,
                                                        means.data(), counts.data(), nullptr));
    int count = -1;
    rc = egdst_quantile_eval(n, x.data(), np, p.data(), out.data(), &count);
    if (rc) { printf("eval rc=%d %s\n", rc, egdst_last_error()); return 1; }
    for (int i = 0; i < np; i++) printf("eval %d %d %016llx\n", i, count, bits(out[i]));
    egdst_destroy(h);
    return 0;
}
