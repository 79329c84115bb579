/*
 * The MEX-library half of the runnable host (TEST INFRASTRUCTURE, see matrix.h).  A gateway is entered through ref_run(),
 * which catches mexErrMsgTxt: the gateway call ends, the process goes on, and the caller gets the text.
 */
#ifndef EGDST_MEXHOST_MEX_H
#define EGDST_MEXHOST_MEX_H
#include <stdio.h>
#include "matrix.h"
#ifdef __cplusplus
extern "C" {
#endif

/* the gateway, defined by the program that is being hosted */
void mexFunction(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[]);

void mexErrMsgTxt(const char *error_msg);      /* ends the gateway call; never returns */
void mexWarnMsgTxt(const char *warn_msg);      /* appended to the warning log, one line each */
int mexPrintf(const char *fmt, ...);
int mexEvalString(const char *command);        /* no interpreter behind this host: does nothing, returns 0 */
int mexCallMATLAB(int nlhs, mxArray *plhs[], int nrhs, mxArray *prhs[], const char *name);  /* likewise; outputs are 0.0 scalars */

/* host entry points (not part of MathWorks' API) */
int ref_run(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[], char *errbuf, size_t errcap);  /* 0: returned, 1: mexErrMsgTxt */
const char *ref_warnings(void);                /* the log since the last ref_reset_warnings(), '\n'-separated */
size_t ref_warning_count(void);
void ref_reset_warnings(void);
int ref_save(const mxArray *pa, const char *path);       /* an array, with everything in it, to a file */
mxArray *ref_load(const char *path);

#ifdef __cplusplus
}
#endif
#endif
