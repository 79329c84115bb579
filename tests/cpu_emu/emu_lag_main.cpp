// Stand-alone driver of the sanitizer build for the moments across two periods (the sanitizer's runtime is linked in, nothing is
// preloaded):
//   emu_lag_main <case file>
// case file: t0 T ngridm ngridmax nthrhmax ny mmax a0 nparam, 2*ny quadrature, the parameters (as emu_main), then
//   nsim seed, init [nsim x 2] column-major, nmom, per record kind col col2 it_first it_last cond_col lo hi cond_lo cond_hi
//   lag2 cond_lag
// Solves one draw and runs egdst_simulate_batch_spec_lag with generated uniforms on the records; prints
//   moment <j> <count> <bits of the mean, hex>
// and then "refused rc=<code>" for each of the three refusals the lags add: lag2 on a kind other than 1, cond_lag without a
// condition, a lag that leaves the model's periods.
#include <climits>
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
    std::vector<double> means(nmom);
    std::vector<int> counts(nmom);
    // (the harness has no device: the "device" buffers are host arrays)
    rc = egdst_simulate_batch_spec_lag(h, init.data(), nsim, nullptr, 0, seed, 0, spec.data(), nmom, nullptr, nullptr, means.data(),
                                       counts.data(), nullptr);
    if (rc) { printf("spec rc=%d %s\n", rc, egdst_last_error()); return 1; }
    for (int j = 0; j < nmom; j++) printf("moment %d %d %016llx\n", j, counts[j], bits(means[j]));
    // refused before anything runs, each on a record of its own: a mean with lag2, a cond_lag without a condition, and a
    // lag no period range survives (INT_MIN: it_last - lag does not fit an int)
    const int nt = d.T - d.t0 + 1;
    egdst_moment_lag bad[3];
    for (auto &r : bad) {
        memset(&r, 0, sizeof r);
        r.col = 1, r.col2 = 1, r.it_first = 1, r.it_last = nt - 2, r.cond_col = -1;
    }
    bad[0].kind = 0, bad[0].lag2 = 1;
    bad[1].kind = 1, bad[1].cond_lag = -1;
    bad[2].kind = 1, bad[2].lag2 = INT_MIN;
    for (const auto &r : bad) {
        std::vector<egdst_moment_lag> s2(spec);
        s2.back() = r;
        printf("refused rc=%d\n", egdst_simulate_batch_spec_lag(h, init.data(), nsim, nullptr, 0, seed, 0, s2.data(), nmom, nullptr, nullptr,
                                                                means.data(), counts.data(), nullptr));
    }
    // the same record with lags the periods allow is taken
    bad[2].lag2 = 1;
    rc = egdst_simulate_batch_spec_lag(h, init.data(), nsim, nullptr, 0, seed, 0, &bad[2], 1, nullptr, nullptr, means.data(), counts.data(),
                                       nullptr);
    printf("accepted rc=%d\n", rc);
    egdst_destroy(h);
    return rc ? 1 : 0;
}
