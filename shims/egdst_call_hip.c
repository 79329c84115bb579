/*
 * egdst_call_hip.c -- MEX gateway  res = egdst_call(model, sw, args)  over the MI355X library.
 * Replaces @egdstmodel/egdst_call.c:17-125 (mexFunction) and :127-164 (vf); called by egdstmodel.call, egdstmodel.m:1190-1200.
 * sw: 1 utility, 2 marginal utility, 3 discount, 4 budget, 5 marginal budget, 6 value function; args is narg x ncol with
 * MATLAB's 1-based it / ist / id.  The solution comes from the model object (:32-34) and is uploaded; nothing is kept
 * between calls.  A wrong number of outputs only warns, as in the reference (:25); fewer than three inputs warn there and
 * then read past prhs: a gateway error here.  The reference's warnings about the rows of args (:51-116) are issued by
 * call_warnings() below, from the arguments and the descriptor alone.
 */
#include "egdst_shim_common.h"

/* The warnings of the reference's loop over the rows of args, in its order: index checks first (a bad index turns the
 * switch off for this row and every later one, :51-57), then the switch's own checks; a wrong column count ends the call
 * at the first row that reaches it (:66); an empty cell has no value function (:138); a cell of fewer than two rows raises
 * the interpolation's message (egdst_lib.c:171), which the reference never clears: it is repeated twice (:146,:161) for
 * that row and for every later row that reaches the value function. */
static void call_warnings(int sw, int narg, int ncol, const double *a, const egdst_desc *d, const egdst_model_info *info,
                          const mxArray *M)
{
    const int nt = d->T - d->t0 + 1;
    int i, interp = 0;
    for (i = 0; i < narg; i++) {
        const int it = (int)a[i] - d->t0, ist = (int)a[narg + i] - 1;
        if (it < 0 || it > nt - 1) { mexWarnMsgTxt("call(): it is outside of admissible range: must be in [t0,T]"); sw = -1; }
        if (ist < 0 || ist > info->nst) { mexWarnMsgTxt("call(): ist is outside of admissible range: must be in [1,nst]"); sw = -1; }
        if (ncol > 2 && sw != 6) {
            const int id = (int)a[2 * narg + i] - 1;
            if (id < 0 || id > info->nd) { mexWarnMsgTxt("call(): id is outside of admissible range: must be in [1,nd]"); sw = -1; }
        }
        switch (sw) {
        case 1:
        case 2:
            if (ncol != 4) {
                mexWarnMsgTxt(sw == 1 ? "call() Wrong number of arguments for utility!" : "call(): Wrong number of arguments for utility!");
                return;
            }
            if (a[3 * narg + i] > d->mmax - d->a0) mexWarnMsgTxt("call(): consumption is above mmax-a0");
            break;
        case 3:
            if (ncol != 2) { mexWarnMsgTxt("call(): Wrong number of arguments for discount!"); return; }
            break;
        case 4:
        case 5:
            if (ncol != 6) { mexWarnMsgTxt("call(): Wrong number of arguments for budget!"); return; }
            if (it + 1 < 0 || it + 1 > nt - 1) mexWarnMsgTxt("call(): it+1 is outside of admissible range: must be in [t0,T]");
            else if (a[3 * narg + i] < d->a0) mexWarnMsgTxt("call(): savings are below a0");
            else if ((int)a[4 * narg + i] - 1 < 0 || (int)a[4 * narg + i] - 1 > info->nst) {
                mexWarnMsgTxt("call(): ist1 is outside of admissible range: must be in [1,nst]");
                sw = -1;
            }
            break;
        case 6:
            if (ncol != 3) { mexWarnMsgTxt("call(): Wrong number of arguments for value function!"); return; }
            if (a[2 * narg + i] > d->mmax) mexWarnMsgTxt("call(): cash in hand is above");
            else if (it != nt - 1) {
                const mxArray *cm = mxGetCell(M, (mwIndex)(ist + it * info->nst));
                if (cm == NULL) { mexWarnMsgTxt("Solution missing for given it,ist.."); break; }
                if (mxGetM(cm) < 2) interp = 1;
                if (interp) {
                    mexWarnMsgTxt("Error:\nError: At least two points are required for interpolation!");
                    mexWarnMsgTxt("Error:\nError: At least two points are required for interpolation!");
                }
            }
            break;
        default:
            break;
        }
    }
}

void mexFunction(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[])
{
    const mxArray *model, *M, *D;
    egdst_model_info info;
    egdst_desc d;
    egdst_handle *h;
    int sw, narg, ncol, nt, rc;

    if (nrhs != 3) mexWarnMsgTxt("Error in call(): wrong number of inputs!");
    if (nlhs != 1) mexWarnMsgTxt("Error in call(): wrong number of outputs!");
    if (nrhs < 3) mexErrMsgTxt("Error in call(): the model, the switch and the arguments are needed!");
    model = prhs[0];
    egdst_get_model_info(&info);
    shim_descriptor(model, &d);
    nt = d.T - d.t0 + 1;
    M = mxGetProperty(model, 0, "M");
    D = mxGetProperty(model, 0, "D");
    if (M == NULL || D == NULL) mexErrMsgTxt("Error: the model has not yet been solved!"); /* :34 */
    sw = (int)mxGetScalar(prhs[1]);
    narg = (int)mxGetM(prhs[2]);
    ncol = (int)mxGetN(prhs[2]);
    if (narg > 0 && ncol < 2) mexErrMsgTxt("Error in call(): every row of arguments starts with it and ist!");
    plhs[0] = mxCreateDoubleMatrix((mwSize)narg, 1, mxREAL); /* zeros: what a wrong column count leaves behind */

    h = shim_handle(model, &d, &info);
    if (!h) mexErrMsgTxt(egdst_last_error());
    rc = shim_upload_solution(h, M, D, info.nst, nt);
    if (rc) {
        egdst_destroy(h);
        mexErrMsgTxt(rc == EGDST_E_ARG ? "Error: the cells of M and D do not have the layout of a solution!" : egdst_last_error());
    }
    rc = egdst_call(h, 0, sw, narg, ncol, mxGetPr(prhs[2]), mxGetPr(plhs[0]));
    egdst_destroy(h);
    if (rc) mexErrMsgTxt(egdst_last_error());
    call_warnings(sw, narg, ncol, mxGetPr(prhs[2]), &d, &info, M);
}
