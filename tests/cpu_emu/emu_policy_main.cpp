// Stand-alone driver of the sanitizer build for the policy at a data panel's observations (the sanitizer's runtime is linked in,
// nothing is preloaded):
//   emu_policy_main <case file>
// The case file: the solver part of emu_case.h, then nobs and per observation  it ist id cash cons w  (cons may be nan).
// Solves one draw and calls egdst_policy_batch with every output for resid 0 and 1, then with the predictions alone.  Prints
//   solve rc=<code>      parts <egdst_policy_parts()>
//   obs <k> <id> <bits of c, hex> <bits of vf, hex>          (of the resid 0 call)
//   fit <resid> <bits of ssr, hex> <hits>
//   same <0 or 1>          whether the call without the fit gave the bits of the call with it
//   refused rc=<code> <message>   for a reserved field that is set, cash below a0, resid 2 and no output
// (the harness has no device: the "device" buffers are host arrays)
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

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    emu_case c;
    int nobs = 0;
    bool read = emu_read_solver_case(f, c) && fscanf(f, "%d", &nobs) == 1 && nobs >= 1;
    std::vector<egdst_obs> obs(read ? nobs : 0);
    for (auto &o : obs) {
        memset(&o, 0, sizeof o);
        read = read && fscanf(f, "%d %d %d %lf %lf %lf", &o.it, &o.ist, &o.id, &o.cash, &o.cons, &o.w) == 6;
    }
    fclose(f);
    if (!read) return 2;

    egdst_handle *h = nullptr;
    int rc = egdst_create(&c.d, 1, 1, nullptr, &h);
    if (rc) { printf("create rc=%d %s\n", rc, egdst_last_error()); return 1; }
    egdst_set_params(h, c.par.data(), 1);
    rc = egdst_solve(h);
    printf("solve rc=%d\nparts %d\n", rc, egdst_policy_parts());
    int status = rc ? 1 : 0;
    std::vector<double> cons(nobs), vf(nobs), cons2(nobs), vf2(nobs);
    std::vector<int> id(nobs), id2(nobs);
    for (int resid = 0; resid < 2 && !status; resid++) {
        double ssr = 0;
        int hits = 0;
        rc = egdst_policy_batch(h, obs.data(), nobs, resid, cons.data(), id.data(), vf.data(), &ssr, &hits);
        if (rc) { printf("policy rc=%d %s\n", rc, egdst_last_error()); status = 1; break; }
        if (resid == 0)
            for (int k = 0; k < nobs; k++) printf("obs %d %d %016llx %016llx\n", k, id[k], bits(cons[k]), bits(vf[k]));
        printf("fit %d %016llx %d\n", resid, bits(ssr), hits);
    }
    if (!status) {
        rc = egdst_policy_batch(h, obs.data(), nobs, 0, cons2.data(), id2.data(), vf2.data(), nullptr, nullptr);
        printf("same %d\n", rc == 0 && !memcmp(cons.data(), cons2.data(), sizeof(double) * nobs) && !memcmp(id.data(), id2.data(), sizeof(int) * nobs) &&
                                !memcmp(vf.data(), vf2.data(), sizeof(double) * nobs));
        std::vector<egdst_obs> bad(obs);
        bad[nobs - 1].reserved = 1;
        printf("refused rc=%d %s\n", egdst_policy_batch(h, bad.data(), nobs, 0, cons2.data(), nullptr, nullptr, nullptr, nullptr), egdst_last_error());
        bad = obs;
        bad[0].cash = c.d.a0 - 1.0;
        printf("refused rc=%d %s\n", egdst_policy_batch(h, bad.data(), nobs, 0, cons2.data(), nullptr, nullptr, nullptr, nullptr), egdst_last_error());
        printf("refused rc=%d %s\n", egdst_policy_batch(h, obs.data(), nobs, 2, cons2.data(), nullptr, nullptr, nullptr, nullptr), egdst_last_error());
        printf("refused rc=%d %s\n", egdst_policy_batch(h, obs.data(), nobs, 0, nullptr, nullptr, nullptr, nullptr, nullptr), egdst_last_error());
    }
    egdst_destroy(h);
    return status;
}
