/*
 * egdst_simulator_hip.c -- MEX gateway  sims = egdst_simulator(model, rndtype)  over the MI355X library.
 * Replaces @egdstmodel/egdst_simulator.c:47-117 (mexFunction); called by egdstmodel.sim, egdstmodel.m:1268.
 * As the reference does, it takes the solution from the model object (properties M and D, :66-68) -- the model may have
 * been solved in another session -- and uploads it (egdst_set_cell_M / egdst_set_cell_D); nothing is kept between calls.
 * Output: nsimout x nt x nsim, nsimout = 11 + nnst + nnd + numel(eq) (:95-101), NaN where an agent has no value.
 */
#include "egdst_shim_common.h"

void mexFunction(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[])
{
    const mxArray *model, *init, *rs, *M, *D;
    egdst_model_info info;
    egdst_desc d;
    egdst_handle *h;
    mwSize dims[3];
    const double *in, *out;
    int nsim, nt, nout, rndtype, rc, i;

    if (nrhs != 2) mexErrMsgTxt("Error: wrong number of inputs!");
    if (nlhs != 1) mexErrMsgTxt("Error: wrong number of outputs!");
    model = prhs[0];
    egdst_get_model_info(&info);
    shim_descriptor(model, &d);
    nt = d.T - d.t0 + 1;
    init = mxGetProperty(model, 0, "init");
    rs = mxGetProperty(model, 0, "randstream");
    if (init == NULL || rs == NULL) mexErrMsgTxt("Error: the model object has no init or no randstream!");
    nsim = (int)mxGetM(init);
    if (nsim > 0 && (mxGetN(init) < 2 || mxGetPr(init) == NULL))
        mexErrMsgTxt("Error: init must have two columns: state index and money-at-hand!");
    rndtype = (int)mxGetScalar(prhs[1]);
    M = mxGetProperty(model, 0, "M");
    D = mxGetProperty(model, 0, "D");
    if (M == NULL || D == NULL) mexErrMsgTxt("Error: the model has not yet been solved!"); /* :68 */

    h = shim_handle(model, &d, &info);
    if (!h) mexErrMsgTxt(egdst_last_error());
    rc = shim_upload_solution(h, M, D, info.nst, nt);
    if (rc) {
        egdst_destroy(h);
        mexErrMsgTxt(rc == EGDST_E_ARG ? "Error: the cells of M and D do not have the layout of a solution!" : egdst_last_error());
    }
    nout = 11 + info.nnst + info.nnd + info.neq;
    dims[0] = (mwSize)nout;
    dims[1] = (mwSize)nt;
    dims[2] = (mwSize)nsim;
    plhs[0] = mxCreateNumericArray(3, dims, mxDOUBLE_CLASS, mxREAL);
    rc = egdst_simulate(h, 0, mxGetPr(init), nsim, mxGetPr(rs), (long long)mxGetNumberOfElements(rs), rndtype, mxGetPr(plhs[0]));
    egdst_destroy(h);
    if (rc == EGDST_E_NOT_SOLVED) mexErrMsgTxt("Solution not found in model.M"); /* an empty cell on an agent's path, :171 */
    if (rc) mexErrMsgTxt(egdst_last_error()); /* short randstream: a hard error in the reference too, :70-75 */
    in = mxGetPr(init);
    out = mxGetPr(plhs[0]);
    for (i = 0; i < nsim; i++) {
        const int ist0 = (int)in[i] - 1;
        const double m0 = in[nsim + i], first = out[(size_t)i * (size_t)nout * (size_t)nt + 5]; /* state index in period 0 */
        if (ist0 < 0 || ist0 >= info.nst) mexWarnMsgTxt("Initial state index st(0) out of bounds! Moving to next simulation.");
        else if (m0 < d.a0 || m0 > d.mmax) mexWarnMsgTxt("Initial money-at-hand out of bounds! Moving to next simulation.");
        else if (first != first) mexWarnMsgTxt("Initial state not feasible! Moving to next simulation."); /* nothing was written */
    }
}
