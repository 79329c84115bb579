// Stand-alone driver of the sanitizer build for the covariance of the moments (the sanitizer's runtime is linked in, nothing is
// preloaded):
//   emu_cov_main <case file>
// case file: as emu_lag_main's -- t0 T ngridm ngridmax nthrhmax ny mmax a0 nparam, 2*ny quadrature, the parameters, then
//   nsim seed, init [nsim x 2] column-major, nmom, per record kind col col2 it_first it_last cond_col lo hi cond_lo cond_hi
//   lag2 cond_lag
// Solves one draw and runs egdst_simulate_batch_spec_cov with generated uniforms on the records; prints
//   parts <egdst_cov_parts()>
//   moment <j> <count> <bits of the mean, hex>
//   cov <j> <k> <bits of Omega_jk, hex>          for every j and k
// and then "refused rc=<code> <message>" for the two refusals the entry adds -- a kind-3 record in the last place, a null
// cov_dev -- and "same <0 or 1>": whether the handle then gives the bits of the first call.
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
    int nsim, nmom;
    unsigned long long seed;
    if (fscanf(f, "%d %llu", &nsim, &seed) != 2 || nsim < 1) return 2;
    std::vector<double> init(2 * (size_t)nsim);
    for (auto &x : init) if (fscanf(f, "%lf", &x) != 1) return 2;
    if (fscanf(f, "%d", &nmom) != 1 || nmom < 1) return 2;
    std::vector<egdst_moment_lag> spec(nmom);
    for (auto &r : spec)
        if (fscanf(f, "%d %d %d %d %d %d %lf %lf %lf %lf %d %d", &r.kind, &r.col, &r.col2, &r.it_first, &r.it_last, &r.cond_col, &r.lo,
                   &r.hi, &r.cond_lo, &r.cond_hi, &r.lag2, &r.cond_lag) != 12) return 2;
    fclose(f);

    egdst_handle *h = nullptr;
    int rc = egdst_create(&d, 1, 1, nullptr, &h);
    if (rc) { printf("create rc=%d %s\n", rc, egdst_last_error()); return 1; }
    egdst_set_params(h, par.data(), 1);
    rc = egdst_solve(h);
    printf("solve rc=%d\n", rc);
    if (rc) return 1;
    printf("parts %d\n", egdst_cov_parts());
    std::vector<double> means(nmom), cov((size_t)nmom * nmom), cov2((size_t)nmom * nmom);
    std::vector<int> counts(nmom);
    // (the harness has no device: the "device" buffers are host arrays)
    rc = egdst_simulate_batch_spec_cov(h, init.data(), nsim, nullptr, 0, seed, 0, spec.data(), nmom, means.data(), counts.data(), cov.data());
    if (rc) { printf("cov rc=%d %s\n", rc, egdst_last_error()); return 1; }
    for (int j = 0; j < nmom; j++) printf("moment %d %d %016llx\n", j, counts[j], bits(means[j]));
    for (int j = 0; j < nmom; j++)
        for (int k = 0; k < nmom; k++) printf("cov %d %d %016llx\n", j, k, bits(cov[(size_t)j * nmom + k]));
    // refused before anything runs: a quantile (valid for egdst_simulate_batch_spec_lag) in the last place, and no cov_dev
    std::vector<egdst_moment_lag> s2(spec);
    egdst_moment_lag &r = s2.back();
    memset(&r, 0, sizeof r);
    r.kind = 3, r.col = 1, r.col2 = 1, r.it_last = d.T - d.t0, r.cond_col = -1, r.lo = 0.5;
    rc = egdst_simulate_batch_spec_cov(h, init.data(), nsim, nullptr, 0, seed, 0, s2.data(), nmom, means.data(), counts.data(), cov2.data());
    printf("refused rc=%d %s\n", rc, egdst_last_error());
    rc = egdst_simulate_batch_spec_cov(h, init.data(), nsim, nullptr, 0, seed, 0, spec.data(), nmom, means.data(), counts.data(), nullptr);
    printf("refused rc=%d %s\n", rc, egdst_last_error());
    // the means and counts alone may be left out, and the handle gives the same bits after the refusals
    rc = egdst_simulate_batch_spec_cov(h, init.data(), nsim, nullptr, 0, seed, 0, spec.data(), nmom, nullptr, nullptr, cov2.data());
    printf("same %d\n", rc == 0 && memcmp(cov.data(), cov2.data(), sizeof(double) * cov.size()) == 0);
    egdst_destroy(h);
    return rc ? 1 : 0;
}
