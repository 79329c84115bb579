/* Stand-alone driver for a hosted gateway (TEST INFRASTRUCTURE): the program to link when the gateway is to run under a
 * sanitizer, whose runtime then sits in the executable itself.
 *     ref_main <nlhs> <output prefix> <input 1> [<input 2> ...]      inputs: files written by ref_save()
 * Calls the gateway once, writes output k to <prefix>.<k>, prints the outcome. */
#include <stdio.h>
#include <stdlib.h>
#include "mex.h"

int main(int argc, char **argv) {
    mxArray *plhs[8] = {0};
    const mxArray *prhs[8];
    char err[1024], path[4096];
    int nlhs, nrhs = argc - 3, k, rc;
    if (argc < 4 || nrhs > 8) return 2;
    nlhs = atoi(argv[1]);
    if (nlhs > 8) return 2;
    for (k = 0; k < nrhs; k++)
        if (!(prhs[k] = ref_load(argv[3 + k]))) return 3;
    freopen("/dev/null", "w", stdout);      /* the hosted program prints diagnostics of its own */
    rc = ref_run(nlhs, plhs, nrhs, prhs, err, sizeof err);
    for (k = 0; k < nlhs && rc == 0; k++) {
        snprintf(path, sizeof path, "%s.%d", argv[2], k);
        if (ref_save(plhs[k], path)) return 4;
    }
    fprintf(stderr, "ref_main: rc=%d warnings=%lu err=%s\n", rc, (unsigned long)ref_warning_count(), err);
    return 0;
}
