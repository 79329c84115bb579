// Stand-alone driver of the sanitizer build (TSan does not work preloaded into python):
//   emu_main <case file>     case file: t0 T ngridm ngridmax nthrhmax ny mmax a0 nparam  then 2*ny quadrature, then params
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "emu_case.h"
int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    emu_case c;
    const bool read = emu_read_solver_case(f, c);
    fclose(f);
    if (!read) return 2;
    egdst_handle *h = nullptr;
    int rc = egdst_create(&c.d, 1, 1, nullptr, &h);
    if (rc) { printf("create rc=%d %s\n", rc, egdst_last_error()); return 1; }
    egdst_set_params(h, c.par.data(), 1);
    rc = egdst_solve(h);
    long long ev = 0;
    egdst_get_evals(h, &ev, nullptr);
    int dbg[16];
    egdst_get_debug(h, 0, dbg);
    printf("solve rc=%d evals=%lld dbg0=%d\n", rc, ev, dbg[0]);
    egdst_destroy(h);
    return rc != 0;
}
