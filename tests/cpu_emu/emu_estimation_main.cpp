// Stand-alone driver of the sanitizer build for the estimation step (the sanitizer's runtime is linked in, nothing is preloaded):
//   emu_estimation_main <spec|lag|cov> <case file>          (the case file: emu_case.h, both parts)
// Solves one draw and runs one entry of the estimation step with generated uniforms on the records; every mode prints
//   solve rc=<code>      and      moment <j> <count> <bits of the mean, hex>
// spec: egdst_simulate_batch_spec on the records narrowed to egdst_moment (exit status 2 if one has a lag); then
//   "refused rc=<code>" for a quantile with p = 1.0, and egdst_quantile_eval on x: eval <i> <count> <bits, hex>
// lag: egdst_simulate_batch_spec_lag; then "refused rc=<code>" for each of the three refusals the lags add -- lag2 on a kind other
//   than 1, cond_lag without a condition, a lag that leaves the model's periods -- and "accepted rc=<code>"
// cov: egdst_simulate_batch_spec_cov; "parts <egdst_cov_parts()>" first, cov <j> <k> <bits of Omega_jk, hex> for every j and k; then
//   "refused rc=<code> <message>" for the two refusals the entry adds -- a kind-3 record in the last place, a null cov_dev --
//   and "same <0 or 1>": whether the handle then gives the bits of the first call.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "emu_case.h"

static unsigned long long bits(double x)
{
    unsigned long long u;
    memcpy(&u, &x, sizeof u);
    return u;
}

static void print_moments(const std::vector<double> &means, const std::vector<int> &counts)
{
    for (size_t j = 0; j < means.size(); j++) printf("moment %d %d %016llx\n", (int)j, counts[j], bits(means[j]));
}

// (the harness has no device: the "device" buffers of every mode are host arrays)
static int run_spec(egdst_handle *h, const emu_case &c)
{
    const int nmom = (int)c.spec.size();
    std::vector<egdst_moment> spec(nmom);
    for (int j = 0; j < nmom; j++) {
        const egdst_moment_lag &r = c.spec[j];
        spec[j] = {r.kind, r.col, r.col2, r.it_first, r.it_last, r.cond_col, r.lo, r.hi, r.cond_lo, r.cond_hi};
    }
    std::vector<double> means(nmom);
    std::vector<int> counts(nmom);
    int rc = egdst_simulate_batch_spec(h, c.init.data(), c.nsim, nullptr, 0, c.seed, 0, spec.data(), nmom, nullptr, nullptr, means.data(),
                                       counts.data(), nullptr);
    if (rc) { printf("spec rc=%d %s\n", rc, egdst_last_error()); return 1; }
    print_moments(means, counts);
    spec[0].lo = 1.0;   // refused before anything runs
    printf("refused rc=%d\n", egdst_simulate_batch_spec(h, c.init.data(), c.nsim, nullptr, 0, c.seed, 0, spec.data(), nmom, nullptr, nullptr,
                                                        means.data(), counts.data(), nullptr));
    if (c.x.empty()) return 0;
    std::vector<double> out(c.p.size());
    int count = -1;
    rc = egdst_quantile_eval((int)c.x.size(), c.x.data(), (int)c.p.size(), c.p.data(), out.data(), &count);
    if (rc) { printf("eval rc=%d %s\n", rc, egdst_last_error()); return 1; }
    for (size_t i = 0; i < out.size(); i++) printf("eval %d %d %016llx\n", (int)i, count, bits(out[i]));
    return 0;
}

static int run_lag(egdst_handle *h, const emu_case &c)
{
    const int nmom = (int)c.spec.size();
    std::vector<double> means(nmom);
    std::vector<int> counts(nmom);
    int rc = egdst_simulate_batch_spec_lag(h, c.init.data(), c.nsim, nullptr, 0, c.seed, 0, c.spec.data(), nmom, nullptr, nullptr,
                                           means.data(), counts.data(), nullptr);
    if (rc) { printf("spec rc=%d %s\n", rc, egdst_last_error()); return 1; }
    print_moments(means, counts);
    // refused before anything runs, each on a record of its own: a mean with lag2, a cond_lag without a condition, and a
    // lag no period range survives (INT_MIN: it_last - lag does not fit an int)
    const int nt = c.d.T - c.d.t0 + 1;
    egdst_moment_lag bad[3];
    for (auto &r : bad) {
        memset(&r, 0, sizeof r);
        r.col = 1, r.col2 = 1, r.it_first = 1, r.it_last = nt - 2, r.cond_col = -1;
    }
    bad[0].kind = 0, bad[0].lag2 = 1;
    bad[1].kind = 1, bad[1].cond_lag = -1;
    bad[2].kind = 1, bad[2].lag2 = INT_MIN;
    for (const auto &r : bad) {
        std::vector<egdst_moment_lag> s2(c.spec);
        s2.back() = r;
        printf("refused rc=%d\n", egdst_simulate_batch_spec_lag(h, c.init.data(), c.nsim, nullptr, 0, c.seed, 0, s2.data(), nmom, nullptr,
                                                                nullptr, means.data(), counts.data(), nullptr));
    }
    // the same record with lags the periods allow is taken
    bad[2].lag2 = 1;
    rc = egdst_simulate_batch_spec_lag(h, c.init.data(), c.nsim, nullptr, 0, c.seed, 0, &bad[2], 1, nullptr, nullptr, means.data(),
                                       counts.data(), nullptr);
    printf("accepted rc=%d\n", rc);
    return rc ? 1 : 0;
}

static int run_cov(egdst_handle *h, const emu_case &c)
{
    const int nmom = (int)c.spec.size();
    printf("parts %d\n", egdst_cov_parts());
    std::vector<double> means(nmom), cov((size_t)nmom * nmom), cov2((size_t)nmom * nmom);
    std::vector<int> counts(nmom);
    int rc = egdst_simulate_batch_spec_cov(h, c.init.data(), c.nsim, nullptr, 0, c.seed, 0, c.spec.data(), nmom, means.data(), counts.data(),
                                           cov.data());
    if (rc) { printf("cov rc=%d %s\n", rc, egdst_last_error()); return 1; }
    print_moments(means, counts);
    for (int j = 0; j < nmom; j++)
        for (int k = 0; k < nmom; k++) printf("cov %d %d %016llx\n", j, k, bits(cov[(size_t)j * nmom + k]));
    // refused before anything runs: a quantile (valid for egdst_simulate_batch_spec_lag) in the last place, and no cov_dev
    std::vector<egdst_moment_lag> s2(c.spec);
    egdst_moment_lag &r = s2.back();
    memset(&r, 0, sizeof r);
    r.kind = 3, r.col = 1, r.col2 = 1, r.it_last = c.d.T - c.d.t0, r.cond_col = -1, r.lo = 0.5;
    rc = egdst_simulate_batch_spec_cov(h, c.init.data(), c.nsim, nullptr, 0, c.seed, 0, s2.data(), nmom, means.data(), counts.data(),
                                       cov2.data());
    printf("refused rc=%d %s\n", rc, egdst_last_error());
    rc = egdst_simulate_batch_spec_cov(h, c.init.data(), c.nsim, nullptr, 0, c.seed, 0, c.spec.data(), nmom, means.data(), counts.data(),
                                       nullptr);
    printf("refused rc=%d %s\n", rc, egdst_last_error());
    // the means and counts alone may be left out, and the handle gives the same bits after the refusals
    rc = egdst_simulate_batch_spec_cov(h, c.init.data(), c.nsim, nullptr, 0, c.seed, 0, c.spec.data(), nmom, nullptr, nullptr, cov2.data());
    printf("same %d\n", rc == 0 && memcmp(cov.data(), cov2.data(), sizeof(double) * cov.size()) == 0);
    return rc ? 1 : 0;
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    int (*run)(egdst_handle *, const emu_case &) =
        !strcmp(argv[1], "spec") ? run_spec : !strcmp(argv[1], "lag") ? run_lag : !strcmp(argv[1], "cov") ? run_cov : nullptr;
    FILE *f = fopen(argv[2], "r");
    if (!run || !f) return 2;
    emu_case c;
    const bool read = emu_read_solver_case(f, c) && emu_read_estimation_case(f, c);
    fclose(f);
    if (!read) return 2;
    if (run == run_spec)
        for (const auto &r : c.spec) if (r.lag2 || r.cond_lag) return 2;   // (egdst_moment cannot carry a lag)

    egdst_handle *h = nullptr;
    int rc = egdst_create(&c.d, 1, 1, nullptr, &h);
    if (rc) { printf("create rc=%d %s\n", rc, egdst_last_error()); return 1; }
    egdst_set_params(h, c.par.data(), 1);
    rc = egdst_solve(h);
    printf("solve rc=%d\n", rc);
    rc = rc ? 1 : run(h, c);
    egdst_destroy(h);
    return rc;
}
