// Stand-alone driver of the sanitizer build for the data panel attached to a handle (the sanitizer's runtime is linked in, nothing
// is preloaded):
//   emu_attached_main <case file>
// The case file is emu_policy_main's: the solver part of emu_case.h, then nobs and per observation  it ist id cash cons w  (cons
// may be nan).  A handle WITHOUT history holds two draws with the case's parameters in two draw groups.  Per residual the panel
// is attached (the second time over the first), two solves are enqueued back to back, each followed by egdst_fit_dev into
// buffers of its own, then one egdst_sync.  Prints
//   parts <egdst_policy_parts()>
//   early rc=<code>                           egdst_fit_dev without a panel, then with a panel and no solve yet
//   fit <resid> <solve> <draw> <bits of ssr, hex> <hits>
//   host <resid> <0 or 1>                     whether egdst_get_fit gave the bits of the last egdst_fit_dev
//   refused rc=<code> <message>               a reserved field that is set, cash below a0, resid 2
//   again <0 or 1>                            whether a solve after the refusals fits with the bits from before them
//   detached rc=<code>                        egdst_get_fit after the detach
// and leaves a panel attached for egdst_destroy to free.  (The harness has no device: the "device" buffers are host arrays.)
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

    const int nd = 2;
    egdst_handle *h = nullptr;
    int rc = egdst_create(&c.d, nd, 0, nullptr, &h);
    if (rc) { printf("create rc=%d %s\n", rc, egdst_last_error()); return 1; }
    std::vector<double> par;
    for (int d = 0; d < nd; d++) par.insert(par.end(), c.par.begin(), c.par.end());
    int status = egdst_set_groups(h, nd) || egdst_set_params(h, par.data(), nd) ? 1 : 0;
    printf("parts %d\n", egdst_policy_parts());
    double ssr[2][nd], last[nd];
    int hits[2][nd], lasth[nd];
    printf("early rc=%d\n", egdst_fit_dev(h, ssr[0], hits[0]));
    for (int resid = 0; resid < 2 && !status; resid++) {
        rc = egdst_attach_panel(h, obs.data(), nobs, resid);
        if (rc) { printf("attach rc=%d %s\n", rc, egdst_last_error()); status = 1; break; }
        if (resid == 0) printf("early rc=%d\n", egdst_fit_dev(h, ssr[0], hits[0]));
        for (int k = 0; k < 2 && !rc; k++) {
            rc = egdst_solve_async(h);
            if (!rc) rc = egdst_fit_dev(h, ssr[k], hits[k]);
        }
        if (!rc) rc = egdst_sync(h);
        if (rc) { printf("solve rc=%d %s\n", rc, egdst_last_error()); status = 1; break; }
        for (int k = 0; k < 2; k++)
            for (int d = 0; d < nd; d++) printf("fit %d %d %d %016llx %d\n", resid, k, d, bits(ssr[k][d]), hits[k][d]);
        rc = egdst_get_fit(h, last, lasth);
        printf("host %d %d\n", resid, rc == 0 && !memcmp(last, ssr[1], sizeof last) && !memcmp(lasth, hits[1], sizeof lasth));
    }
    if (!status) {
        std::vector<egdst_obs> bad(obs);
        bad[nobs - 1].reserved = 1;
        printf("refused rc=%d %s\n", egdst_attach_panel(h, bad.data(), nobs, 0), egdst_last_error());
        bad = obs;
        bad[0].cash = c.d.a0 - 1.0;
        printf("refused rc=%d %s\n", egdst_attach_panel(h, bad.data(), nobs, 0), egdst_last_error());
        printf("refused rc=%d %s\n", egdst_attach_panel(h, obs.data(), nobs, 2), egdst_last_error());
        double again[nd];
        int againh[nd];
        rc = egdst_solve(h);
        if (!rc) rc = egdst_get_fit(h, again, againh);
        printf("again %d\n", rc == 0 && !memcmp(again, last, sizeof last) && !memcmp(againh, lasth, sizeof lasth));
        rc = egdst_attach_panel(h, nullptr, 0, 0);
        if (rc) status = 1;
        printf("detached rc=%d\n", egdst_get_fit(h, again, againh));
        if (egdst_attach_panel(h, obs.data(), nobs, 0)) status = 1;   // (left for egdst_destroy)
    }
    egdst_destroy(h);
    return status;
}
