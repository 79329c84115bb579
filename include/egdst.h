/*
 * egdst.h -- C ABI of the MI355X-native egdst hot path (one shared library PER MODEL).
 *
 * The reference builds three MEX files per model (compile.m:781,793,805) and calls them as
 *     [M,D,dbgout] = egdst_solver(model)        @egdstmodel/egdstmodel.m:1170  -> egdst_solver.c:143 mexFunction
 *     sims         = egdst_simulator(model,rnd) @egdstmodel/egdstmodel.m:1268  -> egdst_simulator.c:47 mexFunction
 * Every entry point below is what a MEX (or any FFI) shim for those two gateways binds; the model
 * plugin (utility, budget, trpr ... compile.m:183-655) is compiled INTO the library as gfx950
 * device code, exactly as the reference compiles modelspec.c into each MEX file.  Plain pointers
 * and sizes only; all buffers are caller-owned host memory unless a name ends in _dev.
 *
 * Error convention: the reference fills a global err[300] (egdst_lib.c:299-302), returns partial
 * results and warns (egdst_solver.c:237).  Here every call returns 0 or an EGDST_E_* code, solve
 * reports a per-draw status, unsolved cells have length 0, egdst_strerror() gives the reference's
 * message for a code and egdst_last_error() the text of the last failing call of this thread.
 */
#ifndef EGDST_H
#define EGDST_H

#ifdef __cplusplus
extern "C" {
#endif

/* Run-time scalars read by parseModel on every call (egdst_lib.c:34-62) plus the quadrature
 * array built by solve (egdstmodel.m:1157-1160): ny weights followed by ny Gauss-Legendre
 * abscissae on [0,1]; the library applies the inverse normal cdf itself (egdst_solver.c:164). */
typedef struct egdst_desc {
    int t0, T;          /* first and last period; nt = T-t0+1 */
    int ngridm;         /* standard number of endogenous grid points */
    int ngridmax;       /* capacity of a cell, rows (without the a0 row) */
    int nthrhmax;       /* capacity of a threshold list */
    int ny;             /* quadrature order */
    double mmax, a0;    /* largest cash-in-hand, credit constraint */
    const double *quadrature; /* host, [2*ny] */
} egdst_desc;

/* Constants baked into this model's library (compile-time in the reference too). */
typedef struct egdst_model_info {
    int nst, nd, nnst, nnd, nparam, neq, distrib;
    int optim_MUnoD, optim_UnoD, optim_UasD, optim_TRPRnoSH;
    double tolerance, zeroconsumption, doublepoint_delta; /* cflags, egdstmodel.m:420-424 */
    const char *label;
} egdst_model_info;

typedef struct egdst_handle egdst_handle; /* device-resident batch of independent solves */

enum {
    EGDST_OK = 0,
    EGDST_E_ARG = 1,            /* bad argument / descriptor */
    EGDST_E_HIP = 2,            /* HIP runtime failure (text in egdst_last_error) */
    EGDST_E_NOGPU = 3,          /* no gfx950 device visible: there is no CPU fallback */
    /* solver errors; same conditions and texts as the reference's error() calls */
    EGDST_E_INTERP2 = 10,       /* egdst_lib.c:172 */
    EGDST_E_TRPR_SUM = 11,      /* egdst_solver.c:580 */
    EGDST_E_NO_SAVINGS = 12,    /* egdst_solver.c:589 */
    EGDST_E_GRID_FULL = 13,     /* egdst_solver.c:662,1336,1378,1413,1456,1890,1912 */
    EGDST_E_EMPTY_CHOICESET = 14, /* egdst_solver.c:700 */
    EGDST_E_ALL_NEG_INF = 15,   /* egdst_solver.c:707 */
    EGDST_E_ENVELOPE = 16,      /* egdst_solver.c:726 */
    EGDST_E_ENV2_SPACE = 17,    /* egdst_solver.c:823,884 */
    EGDST_E_ENV2_SEGMENTS = 18, /* egdst_solver.c:832 */
    EGDST_E_ADRAW_INIT = 19,    /* egdst_solver.c:1018 */
    EGDST_E_THRH_FULL = 20,     /* egdst_solver.c:1327,1891 */
    EGDST_E_TWO_ANALYTIC = 21,  /* egdst_solver.c:1691 */
    EGDST_E_BRACKET_OUT = 22,   /* egdst_solver.c:1938 */
    EGDST_E_BRACKET_REV = 23,   /* egdst_solver.c:1943 */
    EGDST_E_BUDGET_INVERT = 24, /* egdst_lib.c:293 */
    EGDST_E_TRPR_CASES = 25,    /* compile.m:541-544 */
    EGDST_E_RESEND_IN_GRID = 26,/* internal guard: a c1<=0 resend inside the grid stage (egdst_solver.c:1080-1099)
                                   reached the envelope without having been redone sequentially by k_fixup */
    EGDST_E_INTERNAL = 27,      /* scratch exhausted (crossing stack) */
    EGDST_E_CAPACITY = 28,      /* compact handles only: the draw needs more rows than rows_cap (no reference
                                   counterpart; solve the draw again with exact capacities) */
    /* simulator gateway (egdst_simulator.c:54-75,155,165) */
    EGDST_E_NOT_SOLVED = 40,
    EGDST_E_RAND_SHORT = 41,
    EGDST_E_SIM_STATE = 42
};

int egdst_get_model_info(egdst_model_info *out);
const char *egdst_strerror(int code);
const char *egdst_last_error(void);

/* Create a batch of `ndraw` independent solves of this model.  keep_history=1 keeps every period's
 * tables resident (needed for cell export and simulation); 0 keeps two ping-pong periods only.
 * stream: a hipStream_t (NULL = the library creates its own non-blocking stream, and destroys it with the handle).
 * EGDST_STREAM_PER_THREAD is HIP's hipStreamPerThread for hosts that do not include the HIP headers: the calling thread's
 * own default stream, which lives as long as the process.  A host that creates and destroys a handle per call (the MEX
 * shims) should pass it: a stream of the handle's own is a new stream per call, the runtime may put it on another hardware
 * queue than the last one, and a queue on which the solver's kernels run first gets scratch memory of its own (56 MiB on
 * an MI355X, kept until the process ends). */
#define EGDST_STREAM_PER_THREAD ((void *)2)
int egdst_create(const egdst_desc *desc, int ndraw, int keep_history, void *stream, egdst_handle **out);
/* The same with PHYSICAL row capacity rows_cap < ngridmax for every device list and table (0 = exact).  The
 * reference sizes each cell for ngridmax rows (egdst_solver.c:198-217) although a solved cell holds about ngridm;
 * with thousands of draws resident that sparsity costs TLB reach and cache (measured).  All of the
 * reference's limits (ngridmax in the runaway guard :963, error :662 ...) keep their logical values; a draw that
 * would write row rows_cap stops with EGDST_E_CAPACITY instead and must be solved again on an exact handle
 * (egdst_amd.runtime.Solver does that transparently).  Results of the draws that fit are bit-identical. */
int egdst_create_compact(const egdst_desc *desc, int ndraw, int keep_history, int rows_cap, void *stream,
                         egdst_handle **out);
int egdst_destroy(egdst_handle *h);
/* Draw groups.  The draws of a handle are split into `ngroups` contiguous ranges whose per-period kernels are
 * enqueued on separate HIP streams, so that one draw with a long sequential stretch -- the reference's guess generator
 * re-bases point after point on some parameter draws -- holds up its own group only.  Group 0 is enqueued on the handle's own
 * stream, groups 1 .. ngroups-1 on streams forked from and joined to it: ngroups groups keep ngroups hardware queues busy.
 * Results do not depend on the grouping.  The library reads GPU_MAX_HW_QUEUES (unset: 4, the HIP runtime's default) and never
 * sets it.  Default with >= 10 queues: 4 groups from 64 (draw, state) cells, 8 from 512, and 16 from 1024 cells with >= 20
 * queues; with fewer queues: 4 groups from 1024 cells.  Two groups on one queue run one behind the other and the null stream
 * holds a queue, which costs a batch of mostly sparse launches dearly and a dense one little: while the count is the default
 * and history-based scheduling is on, a handle on the envelope step's throughput path whose last solve regenerated 0.5 % or more
 * of its guess streams continues with at most queues - 1 groups (3 on 4 queues), and returns to the default when a solve falls
 * below.  Environment EGDST_GROUPS and a call of this function override and end that.  At most 32, and at most ndraw. */
int egdst_set_groups(egdst_handle *h, int ngroups);
/* History-based scheduling (on by default with more than one group): after a solve, the draws whose guess streams
 * re-based more than 1000 times (degenerate parameter draws: one such stream is ~75 ms of strictly sequential work)
 * are scheduled on up to 8 extra streams of their own in the next solves, as far as hardware queues are left beside the groups',
 * so that they hold up each other instead of a whole group.  Results do not depend on it. */
int egdst_set_adaptive(egdst_handle *h, int on);
/* Current schedule: regular groups, extra straggler lanes, draws currently treated as stragglers. */
int egdst_get_schedule(egdst_handle *h, int *groups, int *lanes, int *stragglers);
/* Re-basing calls of every draw's guess streams in the last solve (the straggler measure). */
int egdst_get_work(egdst_handle *h, unsigned *out /* [ndraw] */);
/* Guess streams of every draw that had to be regenerated sequentially in the last solve (zero-consumption signal inside
 * the grid stage, egdst_solver.c:1080-1099): a diagnostic of where a batch spends sequential time. */
int egdst_get_regenerations(egdst_handle *h, unsigned *out /* [ndraw] */);
/* Physical geometry of the handle: rows per list and row stride of the device tables (egdst_device_tables). */
int egdst_geometry(egdst_handle *h, int *rows_cap, int *table_stride);

/* Parameter vectors, one row per draw: params[draw*nparam + k] (loadparameters, compile.m:469-475).
 * F8 of SURVEY.md: the batch-of-draws surface is new; ndraw==1 is the reference's setparam+solve. */
int egdst_set_params(egdst_handle *h, const double *params, int ndraw);
int egdst_set_params_dev(egdst_handle *h, const double *params_dev, int ndraw);
int egdst_get_params(egdst_handle *h, double *params /* host, [ndraw*nparam] */);

/* Backward induction for all draws (egdst_solver.c:258-339).  _async only enqueues on the handle's
 * stream; egdst_sync waits and returns the first non-zero per-draw status (or 0).  Solves may be enqueued back to
 * back without a host synchronisation in between (egdst_set_params_dev, egdst_solve_async, egdst_objective_dev, again):
 * each follows the one before on the handle's stream. */
int egdst_solve_async(egdst_handle *h);
int egdst_sync(egdst_handle *h);
int egdst_solve(egdst_handle *h);
int egdst_get_status(egdst_handle *h, int *status /* [ndraw] */, int *where /* [2*ndraw] (it,ist) or NULL */);

/* EGM evaluations the reference would have executed (body at egdst_solver.c:548-570), summed over draws. */
int egdst_get_evals(egdst_handle *h, long long *total, long long *per_draw /* [ndraw] or NULL */);
/* The part of those counts that was accounted for WITHOUT being executed: when the guess generator's first stage gets
 * M = +inf back for A = mmax it asks for mmax again until its runaway guard (egdst_solver.c:963-978); the expectation is a
 * pure function of the guess, so the device executes it once and credits the repeats.  Throughput figures subtract this. */
int egdst_get_evals_credited(egdst_handle *h, long long *total, long long *per_draw /* [ndraw] or NULL */);

/* Cell export in the reference's wire layout (saveoutput, egdst_solver.c:917-952):
 *   M cell: (len x 4) column-major [M C A V], row 0 = (a0, 0, a0, evf(a0));  D cell: (thlen x 2) [D TH].
 * Requires keep_history=1.  len==0: the cell was not solved (infeasible state or earlier error). */
int egdst_cell_dims(egdst_handle *h, int draw, int it, int ist, int *len, int *thlen);
int egdst_get_cell_M(egdst_handle *h, int draw, int it, int ist, double *out /* [len*4] */);
int egdst_get_cell_D(egdst_handle *h, int draw, int it, int ist, double *out /* [thlen*2] */);
/* Bulk export of one draw: lens/thlens [nt*nst], M/C/V [nt*nst*(ngridmax+1)], D/TH [nt*nst*nthrhmax];
 * slot = it*nst+ist.  Any pointer may be NULL. */
int egdst_get_solution(egdst_handle *h, int draw, int *lens, int *thlens, double *M, double *C, double *V,
                       double *D, double *TH);

/* Solution import, the inverse of the export calls.  The reference's simulator and accessor gateways read the cell arrays
 * M and D from the model object on every call (egdst_simulator.c:61-68, egdst_call.c:28-34; the class is ConstructOnLoad,
 * egdstmodel.m:1, so a saved model is simulated without solving again): a handle that never ran egdst_solve is given the
 * cells here and then serves egdst_simulate*, egdst_call, egdst_get_cell_* and egdst_get_checksums exactly as the handle
 * that solved them.  Same layouts as the export: M cell (len x 4) column-major [M C A V] (A is ignored, it is M - C),
 * D cell (thlen x 2) [D TH]; len == 0 marks the cell unsolved (the reference's empty cell).  Rows past len are zeroed.
 * Requires keep_history=1 and egdst_set_params for the draw (the model functions read the parameters).  The draw's
 * status becomes 0.  EGDST_E_ARG if a cell exceeds ngridmax+1 rows or nthrhmax thresholds. */
int egdst_set_cell_M(egdst_handle *h, int draw, int it, int ist, int len, const double *in /* [len*4] */);
int egdst_set_cell_D(egdst_handle *h, int draw, int it, int ist, int thlen, const double *in /* [thlen*2] */);
/* Bulk import of one draw, argument for argument the arrays egdst_get_solution fills (none may be NULL). */
int egdst_set_solution(egdst_handle *h, int draw, const int *lens, const int *thlens, const double *M, const double *C,
                       const double *V, const double *D, const double *TH);

/* Forward simulation of draw `draw` (egdst_simulator.c:47-117): init [nsim x 2] column-major (state index
 * base-1, cash-in-hand), randstream uniforms, rndtype 1 = every agent reuses the head of the stream.
 * sims: [nsimout x nt x nsim] column-major, nsimout = 11+nnst+nnd+neq, NaN where the agent is dead. */
int egdst_simulate(egdst_handle *h, int draw, const double *init, int nsim, const double *randstream,
                   long long nrand, int rndtype, double *sims);

/* Simulated moments (new surface): the same simulation, but only the per-period means of the
 * simulated columns leave the device -- means[col + nout*it] over the agents that have a value in period it, counts the
 * number of those agents (nout = 11+nnst+nnd+neq columns as in egdst_simulate).  Deterministic summation order. */
int egdst_simulate_moments(egdst_handle *h, int draw, const double *init, int nsim, const double *randstream,
                           long long nrand, int rndtype, double *means /* [nout*nt] */, int *counts /* [nout*nt] */);

/* The estimation step on the device: EVERY draw of the handle is simulated with the same nsim agents
 * (init as in egdst_simulate) and the same uniforms -- common random numbers -- and per draw only moments and an
 * objective leave the kernels:
 *   means_dev [ndraw][nout*nt], counts_dev [ndraw][nout*nt]   as egdst_simulate_moments, DEVICE buffers (may be NULL)
 *   obj_dev   [ndraw]   sum over the cells with weight != 0 of weight[k] * (mean[k] - target[k])^2, k = col + nout*it
 *                       (target, weight: host, [nout*nt]); NaN for a draw that failed to solve or has an empty weighted
 *                       cell.  DEVICE buffer (e.g. a torch tensor): it is what the cross-GPU reduce (RCCL) takes.
 * Uniforms: randstream_dev (device, layout and length rules of egdst_simulate) or NULL: generated on the device by the
 * counter-based generator egdst_uniform(seed, k) below, k the index a randstream would have.  Requires keep_history=1. */
int egdst_simulate_batch_moments(egdst_handle *h, const double *init, int nsim, const double *randstream_dev,
                                 long long nrand, unsigned long long seed, int rndtype, const double *target,
                                 const double *weight, double *means_dev, int *counts_dev, double *obj_dev);
/* One simulated moment of the estimation step.  Over the (agent, period) pairs with it_first <= it <= it_last whose
 * value is present (not NaN) and, if cond_col >= 0, with cond_lo <= sims[cond_col] <= cond_hi (NaN never qualifies):
 *   kind 0  mean of sims[col]
 *   kind 1  mean of sims[col] * sims[col2]                      (both present)
 *   kind 2  share with lo <= sims[col] <= hi among those pairs  (a choice share: col = 4, lo = hi = k)
 *   kind 3  quantile p of sims[col], p carried in lo with 0 < p < 1 (col2 is ignored; hi is the bandwidth of the record's
 *           covariance, which egdst_simulate_batch_spec_cov alone reads: every other entry ignores it): an order statistic, by exact
 *           selection on the device.  The qualifying values are those of kind 0 and count is n, their number (n = 0: NaN
 *           mean, count 0).  Rank: t = p * (double)n, one fp64 product; k = (long long)ceil(t), clamped to [1, n].  The k-th
 *           smallest qualifying value (1-based) is the "mean", its bit pattern untouched: no interpolation, so the median of
 *           an even n is the lower middle value.  "Smaller" is the total order of the keys u = bits(x),
 *           key = (u >> 63) ? ~u : u | 1<<63, compared as unsigned 64-bit: -0.0 comes before +0.0, -inf first, +inf last.
 *           No floating-point arithmetic beyond t, hence no summation order: the value is exact whatever the block size.
 * Columns are 0-based as in egdst_simulate (nout = 11+nnst+nnd+neq); periods are 0-based model periods. */
typedef struct {
    int kind, col, col2, it_first, it_last, cond_col;
    double lo, hi, cond_lo, cond_hi;
} egdst_moment;   /* 56 bytes */

/* The estimation step with user-defined moments and a full weighting matrix (new surface).  Simulation,
 * uniforms, rndtype, common random numbers, slicing and failed draws exactly as egdst_simulate_batch_moments; per draw:
 *   means_dev [ndraw][nmom], counts_dev [ndraw][nmom]   moment j of spec[j]; NaN mean / 0 count where no pair qualifies
 *   obj_dev   [ndraw]   e' W e, e_j = mean_j - target_j (target: host [nmom], W: host [nmom x nmom] row-major); NaN if a
 *                       moment with a non-zero entry in its row or column of W has count 0
 * All three are DEVICE buffers and may be NULL, but one of them must be given; obj_dev needs target and W.
 * Summation order (part of the contract; B = 256, the moment kernel's block size):
 *   partial t (0 <= t < B) starts at 0.0 and adds the qualifying values of the agents i = t (mod B) in ascending i, within
 *   an agent in ascending period (kind 2 adds 1.0 or 0.0); then for o = B/2 .. 1: p[t] += p[t+o] (t < o); mean = p[0] / count.
 *   A kind-0 moment over one period without condition is exactly the egdst_simulate_batch_moments cell.
 *   r_j = sum over k ascending of W_jk * e_k, skipping W_jk == 0; obj = sum over j ascending of e_j * r_j, skipping the j
 *   whose row of W is all zero (a diagonal W gives the bits of egdst_simulate_batch_moments' objective).
 * EGDST_E_ARG before anything is launched if a kind is not 0..3, the p (lo) of a kind-3 moment is NaN or outside the open
 * interval (0, 1), a column is outside [0, nout) (cond_col -1: no condition), a period range is empty or outside [0, nt),
 * nmom <= 0, nsim times the periods of a moment exceeds INT_MAX, obj_dev is given without target and W, or no output is
 * given. */
int egdst_simulate_batch_spec(egdst_handle *h, const double *init, int nsim, const double *randstream_dev,
                              long long nrand, unsigned long long seed, int rndtype,
                              const egdst_moment *spec, int nmom,
                              const double *target /* [nmom] */, const double *W /* [nmom x nmom] row-major */,
                              double *means_dev /* [ndraw][nmom] */, int *counts_dev /* [ndraw][nmom] */,
                              double *obj_dev /* [ndraw] */);
/* A moment across two periods: the 56 bytes of egdst_moment with the same meaning, then two lags in periods, back (> 0) or
 * ahead (< 0).  Pairs (agent, it) run over it_first <= it <= it_last, and the checks come in this order:
 *   1. v = sims[col][it] must be present;
 *   2. if cond_col >= 0, c = sims[cond_col][it - cond_lag] must satisfy cond_lo <= c <= cond_hi (NaN never qualifies: an
 *      agent that is dead or not yet valued in that other period drops out);
 *   3. kind 1 takes w = sims[col2][it - lag2], which must be present, and x = v * w;
 *   4. kinds 0, 2 and 3 use v as in egdst_moment.
 * A retirement hazard is kind 2 on the choice column with cond_col the same column, cond_lo = cond_hi = the origin and
 * cond_lag = 1; persistence E[x_t x_t-1] is kind 1 with lag2 = 1; "those about to retire" is a condition with cond_lag = -1. */
typedef struct {
    int kind, col, col2, it_first, it_last, cond_col;
    double lo, hi, cond_lo, cond_hi;
    int lag2, cond_lag;
} egdst_moment_lag;   /* 64 bytes, no padding */

/* egdst_simulate_batch_spec, argument for argument, on egdst_moment_lag records.  Count, the NaN mean with count 0, the
 * summation order, the quantile's rank and key order, failed draws, slicing and the objective are those of
 * egdst_simulate_batch_spec; a record with both lags zero gives the bits of that call on its first 56 bytes.
 * EGDST_E_ARG before anything is launched, with the moment's index in egdst_last_error: everything egdst_simulate_batch_spec
 * refuses; lag2 != 0 on a kind other than 1; cond_lag != 0 with cond_col == -1; a lag in use for which it_first - lag < 0 or
 * it_last - lag >= nt (any int lag; the period range is never clipped: the caller chooses it). */
int egdst_simulate_batch_spec_lag(egdst_handle *h, const double *init, int nsim, const double *randstream_dev,
                                  long long nrand, unsigned long long seed, int rndtype,
                                  const egdst_moment_lag *spec, int nmom,
                                  const double *target /* [nmom] */, const double *W /* [nmom x nmom] row-major */,
                                  double *means_dev /* [ndraw][nmom] */, int *counts_dev /* [ndraw][nmom] */,
                                  double *obj_dev /* [ndraw] */);
/* The covariance of the simulated moments (new surface): the step of egdst_simulate_batch_spec_lag without an
 * objective, and per draw the matrix Omega [nmom x nmom] of the moment vector.  Simulation, uniforms, rndtype, common random
 * numbers, slicing and failed draws are those of egdst_simulate_batch_spec_lag, and means_dev / counts_dev (DEVICE, may be NULL)
 * receive the bits that call writes.  cov_dev [ndraw][nmom][nmom] row-major is a DEVICE buffer and required.
 * Meaning: Omega is the agent-clustered delta-method variance of the vector of ratio estimators m_j (each a sum over an agent's
 * qualifying pairs divided by their number): the agents are the independent units, and all periods of an agent enter as one
 * cluster.  No degrees-of-freedom correction; nsim * Omega estimates the asymptotic variance.  For one period without a
 * condition Omega_jj is the population variance of the values divided by N_j; for a moment pooled over periods it is not
 * divided by the number of periods again.  It gives the efficient weighting matrix (its inverse, or a generalised inverse:
 * shares that sum to one make it singular), standard errors and the simulation-noise term of the sandwich formula, for specs
 * that hold quantiles too (below).
 * For one draw, records j and k (kinds 0, 1 and 2) and agent i, every operation a rounded fp64 operation, no FMA:
 *   c_ij   the number of the agent's qualifying pairs (those egdst_moment_lag's checks accept in the record's period range);
 *   s_ij   starts at 0.0 and adds the agent's qualifying values in ascending period (kind 2 adds 1.0 or 0.0);
 *   N_j    = sum over i of c_ij, the count of the moment; m_j its mean, the bits egdst_simulate_batch_spec_lag writes;
 *   d_ij   = (s_ij - m_j * (double)c_ij) / (double)N_j       the agent's score: one product, one difference, one quotient;
 *   Omega_jk = sum over i of d_ij * d_ik in this order, P = egdst_cov_parts() = 4 in this library:
 *            partial t (0 <= t < P) starts at 0.0 and, for the agents i = t (mod P) in ascending i, p_t = p_t + (d_ij * d_ik),
 *            the product rounded, then the sum; then for o = P/2 .. 1: p[t] += p[t+o] (t < o); Omega_jk = p[0].
 *   Omega_kj carries the bits of Omega_jk.
 * A kind-3 record j (a quantile) enters with p = lo and a bandwidth h = hi, 0 < p - h and p + h < 1 (the rounded fp64 difference
 * and sum).  Its score is the agent-clustered influence function of the sample quantile, (p - F^(q)) / f(q), with 1 / f estimated
 * by the spacing of two order statistics (Siddiqui; Bloch and Gastwirth); it is centred on p and not on F^, so a record's scores
 * sum to s_j (p N_j - T_j) / N_j, T_j the sum of the t_ij: not zero, but O(1 / N).  Every operation one rounded fp64 operation:
 *   N_j, q_j  the count and the value egdst_simulate_batch_spec_lag writes for the record (means_dev and counts_dev get these bits);
 *   a_j, b_j  the order statistics of the same qualifying values of ranks k_lo = rank(p - h, N_j) and k_hi = rank(p + h, N_j),
 *             rank and key order those of kind 3 above (ceil of the one product, clamped to [1, N_j]);
 *   s_j    = (b_j - a_j) / ((double)(k_hi - k_lo) / (double)N_j)   the sparsity: one difference, one quotient of the two
 *             conversions, one quotient.  k_hi == k_lo gives 0 / 0 = NaN, N_j = 0 gives NaN, a tie a_j == b_j with distinct ranks
 *             0.0 (a quantile inside a mass point has variance 0, the right limit); infinite ends flow through IEEE arithmetic;
 *   c_ij   as above;  t_ij  the number of those pairs whose key is <= the key of q_j (the integer comparison of the selection's
 *             keys: -0.0 comes before +0.0);
 *   d_ij   = (s_j * (p * (double)c_ij - (double)t_ij)) / (double)N_j    a product, a difference, a product and a quotient.
 * Omega is then formed as above.
 * An empty moment (N_j = 0) has m_j = NaN and d_ij = NaN: row and column j of Omega are NaN (the payload is not part of the
 * contract), and so are those of a quantile whose s_j is NaN.  A draw that failed to solve has counts 0, NaN means and an
 * all-NaN Omega.
 * EGDST_E_ARG before anything is launched, with the moment's index in egdst_last_error where a record is at fault: everything
 * egdst_simulate_batch_spec_lag refuses; a kind-3 record with hi == 0.0 (a quantile has no covariance without a bandwidth: its
 * influence function needs a density estimate), with hi NaN or hi <= 0, or with lo - hi <= 0 or lo + hi >= 1 (the message names
 * the quantile and its bandwidth); cov_dev == NULL. */
int egdst_simulate_batch_spec_cov(egdst_handle *h, const double *init, int nsim, const double *randstream_dev,
                                  long long nrand, unsigned long long seed, int rndtype,
                                  const egdst_moment_lag *spec, int nmom,
                                  double *means_dev /* [ndraw][nmom], may be NULL */,
                                  int *counts_dev   /* [ndraw][nmom], may be NULL */,
                                  double *cov_dev   /* [ndraw][nmom][nmom] row-major, required */);
/* The number P of partial sums of the covariance's summation order (build constant COV_P: one per wave of k_moment_cov's
 * 256-thread workgroup), a power of two in [1, 256]. */
int egdst_cov_parts(void);

/* One observation of a data panel, the other half of the estimation step (new surface): a household seen in
 * period it (0-based model period) in state ist (0-based, as column 5 of the simulated paths) with cash-in-hand `cash`, that
 * chose id (0-based as column 4; -1: the choice was not observed) and consumed cons (NaN: not observed), with weight w in the
 * fit.  reserved must be 0. */
typedef struct {
    int it, ist, id, reserved;
    double cash, cons, w;
} egdst_obs;   /* 40 bytes, no padding */

/* The model's policy at every observation, for EVERY draw of the handle, and per draw the fit to the observed consumption and
 * choices: non-linear least squares, or (resid = 1) the log residuals of a likelihood with measurement error in consumption.
 * obs is HOST memory [nobs]; the five outputs are DEVICE buffers, each may be NULL but one must be given:
 *   cons_dev [ndraw][nobs], id_dev [ndraw][nobs], vf_dev [ndraw][nobs]   the policy at observation k of draw d, at [d*nobs + k]
 *   ssr_dev [ndraw]    the weighted sum of squared residuals;   hits_dev [ndraw]   the correctly predicted choices
 * Requires keep_history=1.  Runs on the handle's stream, after the solve enqueued there; returns when the results are written.
 * Per (draw, observation) exactly what the simulator does for an agent standing at (it, ist) with `cash` (policy,
 * egdst_simulator.c:145-199; the kernels share one routine): on the table of (it, draw, ist), i the bracket of cash in the M
 * column (bxsearch), c the interpolation of C over rows i, i+1 (linter's expression, two divisions); id = D[max(j - 1, 0)], j the
 * number of leading thresholds TH <= cash; vf = u(c) + discount * V[0] when cash < M[1] and V[0] > -inf, else the interpolation of
 * V over the same rows.  (egdst_call's value function has a third branch, -inf; this is the simulator's form.)
 * A draw that failed to solve has NaN / -1 / NaN at every observation, ssr NaN and hits -1.  In a solved draw an observation
 * whose cell was not solved (fewer than 2 rows) has NaN / -1 / NaN and makes that draw's ssr NaN, whether or not it enters the
 * fit; hits counts the other observations.
 * The fit, every operation a rounded fp64 operation, no FMA: r_k = cons_k - c_k (resid 0) or log(cons_k) - log(c_k) (resid 1,
 * the log of include/egdst_math.h: glibc's bits; a c_k <= 0 flows through as -inf / NaN); term_k = w_k * (r_k * r_k), the square
 * rounded, then the product.  Observations with cons NaN or w == 0 are skipped.
 * Summation order (part of the contract; B = egdst_policy_parts() = 256 in this library): partial t (0 <= t < B) starts at 0.0
 * and adds the terms of the observations k = t (mod B) that are not skipped in ascending k; then for o = B/2 .. 1: p[t] += p[t+o]
 * (t < o); ssr = p[0].  hits is the exact number of observations with id_k >= 0 equal to the predicted decision.  The order is
 * over the caller's indices: the order in which the library's lanes take the observations and the slices it cuts the draws into
 * change no bit of any result.
 * EGDST_E_ARG before anything is launched, with the observation's index in egdst_last_error where one is at fault: nobs <= 0; it
 * outside [0, nt) or ist outside [0, nst); id outside [-1, nd); reserved != 0; cash NaN or below a0 (above mmax the tables are
 * extrapolated over their last two rows, as the simulator does for an agent whose cash has grown past mmax: more than half of the
 * pairs of a simulated occ3 panel stand there); w NaN or negative; resid not 0 or 1; resid = 1 with a cons <= 0; no output given; a model with continuous
 * states (there the simulator's policy is a blend over grid corners: not served). */
int egdst_policy_batch(egdst_handle *h, const egdst_obs *obs /* host, [nobs] */, int nobs, int resid,
                       double *cons_dev /* [ndraw][nobs] */, int *id_dev /* [ndraw][nobs] */, double *vf_dev /* [ndraw][nobs] */,
                       double *ssr_dev /* [ndraw] */, int *hits_dev /* [ndraw] */);
/* The number B of partial sums of the fit's summation order (build constant POL_BS: the threads of k_policy_fit's workgroup), a
 * power of two. */
int egdst_policy_parts(void);

/* The same fit with the panel RESIDENT on the handle and evaluated inside the solve, for an estimation loop that solves thousands
 * of times against one panel (egdst_set_params_dev, egdst_solve_async, egdst_fit_dev back to back, no host synchronisation).
 * egdst_attach_panel checks obs (HOST memory, [nobs]) and resid as egdst_policy_batch does -- every refusal of that door that
 * concerns the observations, resid or the model, with the same messages; nothing is kept when one fails -- and uploads once the
 * observations, their grouping by cell and period, and reserves the terms of every (draw, observation), 12 bytes each: if the
 * device cannot give them, EGDST_E_HIP with the bytes asked for in egdst_last_error and no panel attached.  Works with
 * keep_history 0 and 1 and before or after a solve; a one-time host call that waits for the handle's stream.  Attaching again
 * replaces the panel; obs == NULL with nobs == 0 detaches and frees it.  While a panel is attached, every solve evaluates the
 * observations of period it on the period's table right behind that period's envelope step, on the draw groups' own streams --
 * on a handle without history that is while the table is live -- one more launch per group and period with observations; without a
 * panel a solve enqueues what it always did.
 * egdst_fit_dev enqueues the reduction on the handle's stream behind the solve and returns without waiting (the contract of
 * egdst_objective_dev): ssr_dev and hits_dev are DEVICE buffers [ndraw], either may be NULL, not both.  The values are those of
 * egdst_policy_batch's ssr_dev and hits_dev on a kept-history handle with the same draws, bit for bit: its terms, its skips, its
 * summation order over the caller's indices with egdst_policy_parts() partials, hits an exact count, NaN and -1 for a draw that
 * failed (on a compact handle a draw stopped by EGDST_E_CAPACITY reads as failed), NaN ssr for a draw with an observation in a
 * cell of fewer than 2 rows.  The draw groups, their order and the grouping of the observations change no bit.
 * EGDST_E_ARG without an attached panel or with both outputs NULL; EGDST_E_NOT_SOLVED when no solve was enqueued since the
 * attach, or a solution was imported since (egdst_set_cell_M / _D, egdst_set_solution: the fit answers for solves alone).
 * egdst_get_fit is the host form (ssr, hits: HOST [ndraw], either may be NULL); it waits for the stream. */
int egdst_attach_panel(egdst_handle *h, const egdst_obs *obs /* host, [nobs]; NULL with nobs 0: detach */, int nobs, int resid);
int egdst_fit_dev(egdst_handle *h, double *ssr_dev /* [ndraw] */, int *hits_dev /* [ndraw] */);
int egdst_get_fit(egdst_handle *h, double *ssr /* host, [ndraw] */, int *hits /* host, [ndraw] */);

/* Uniform number k of stream `seed` (host replay of the device generator): with z = seed + (k+1)*0x9E3779B97F4A7C15,
 * z = (z ^ z>>30)*0xBF58476D1CE4E5B9, z = (z ^ z>>27)*0x94D049BB133111EB, z ^= z>>31 (splitmix64): (z >> 11) * 2^-53. */
double egdst_uniform(unsigned long long seed, unsigned long long k);

/* Model-function accessor behind egdstmodel.call (egdst_call.c:17-164; egdstmodel.m:1181-1207).  sw: 1 utility
 * (it, ist, id, consumption), 2 marginal utility (same), 3 discount (it, ist), 4 budget (it, ist, id, savings, ist1,
 * shock), 5 marginal budget (same), 6 value function from the solved tables (it, ist, cash).  args: host, [narg x ncol]
 * column-major with MATLAB's 1-based it/ist/id; res: host, [narg].  The gateway's conventions are kept: the first row
 * with an out-of-range index makes that row and every later one NaN, a wrong column count leaves zeros.  Requires
 * keep_history=1 (the value function reads the period's table). */
int egdst_call(egdst_handle *h, int draw, int sw, int narg, int ncol, const double *args, double *res);

/* Objective contributions of an estimation loop (new surface): out_dev[2*draw+{0,1}] =
 * value and consumption at the first endogenous grid point of (it=0, ist=0); NaN for failed draws.  The buffer
 * is device memory (e.g. a torch tensor) so that the cross-GPU reduce (RCCL) needs no host copy.  Enqueued on
 * the handle's stream. */
int egdst_objective_dev(egdst_handle *h, double *out_dev);
int egdst_get_objective(egdst_handle *h, double *out /* host, [2*ndraw] */);

/* Measurement: with profiling on, the launches of a solve are bracketed by HIP events on the stream they are
 * launched on (the draw groups' streams).  egdst_get_profile returns, for the nine classes
 *   0 k_probe / k_terminal      1 the grid kernel alone (k_grid_lds, k_grid_wide or k_grid)      2 k_envelope
 *   3 regeneration of guess streams (k_fixup_scan + k_fixup)
 *   4 k_tp_prep   5, 6 k_tp_sort stage 0, 1   7, 8 k_tp_walk stage 0, 1   (the envelope step's throughput path; with it on,
 *     class 2 is the period's tail launch, k_tp_tail: the cells the path left over and the second tier of its stage 1)
 * the summed device time in ms and the number of bracketed launches of the LAST solve (kernels of a class that was not
 * launched: 0), and the algorithmic table bytes of that solve summed over draws (24 B per table row read once per period,
 * 24 B per row written, 16 B per threshold). */
int egdst_set_profile(egdst_handle *h, int on);
int egdst_get_profile(egdst_handle *h, double *ms /* [9] */, int *launches /* [9] */, long long *algbytes);
/* The same events read per draw group (profiling on): for each of the groups of the last solve, ms from the start of the FIRST
 * group's first kernel to the end of this group's last kernel (out_ms[g]) -- how evenly the groups finish -- and the sum of this
 * group's bracketed kernel time per class (out_class_ms[g * 9 + k], may be NULL).  Returns the number of groups (<= max_groups). */
int egdst_get_group_profile(egdst_handle *h, int max_groups, double *out_ms, double *out_class_ms);

/* Diagnostics of a tripped internal guard (EGDST_E_INTERNAL and 27xx codes): 16 ints, meaning is internal. */
int egdst_get_debug(egdst_handle *h, int draw, int *out16);

/* Clock stamps of a diagnostic build, -DEGDST_STAMPS=<set>: where the kernels of the set spend their time.
 * egdst_stamp_names: the names of the slots, "<set>.<what>", into names[0 .. cap) (may be NULL); returns their number, the same
 * in every build.  egdst_get_stamps: the slots of one draw as the last solve left them, that many values -- ticks of 10 ns, or
 * counts; the slots of the sets that are not compiled in are zero.  A library built without stamps returns EGDST_E_ARG. */
int egdst_stamp_names(const char **names, int cap);
int egdst_get_stamps(egdst_handle *h, int draw, unsigned long long *out);

/* Third output of the solver gateway, [M,D,dbgout] = egdst_solver(model) (egdst_solver.c:178-181, filled in thresholds()
 * :1866-1879, DEBUGOUT is always on in the reference): one row per kink the secondary and primary envelopes record, in the
 * order they are recorded -- it, ist, the choice whose secondary envelope it is (-1: primary), the threshold, consumption
 * left and right of it (-.9999 where it is the zero-consumption marker), |right - left|.  egdst_set_dbgout(h, 1) before
 * the solve makes the kernels keep the log (device memory: nt*ndraw*nst*min((nd+1)*nthrhmax, cap)*32 B, so meant for the
 * single-draw handle of the gateway); egdst_get_dbgout copies one draw's rows into out [cap x 7] column-major with
 * cap = nt*nst*nd*2*nt, zero rows after the *nrows recorded ones, rows beyond cap dropped, as the reference does. */
int egdst_set_dbgout(egdst_handle *h, int on);
int egdst_get_dbgout(egdst_handle *h, int draw, double *out /* [nt*nst*nd*2*nt * 7] */, int *nrows);

/* Checksums of one draw's solution, computed on the device: out[(it*nst+ist)*5 + k] = wrapping 64-bit sum over the rows i of
 * bits(x_i) * (2 i + 1) for column k in {M, C, V} of the cell's rows and {TH, D} of its thresholds (the odd weight pins the
 * order of the rows).  Lets a caller (and the parity tests at BASELINE.json's full sizes) compare whole solutions without
 * exporting them.  Requires keep_history=1. */
int egdst_get_checksums(egdst_handle *h, int draw, unsigned long long *out /* [nt*nst*5] */);

/* Diagnostics: this library's device exp (fn 0), log (1), pow (2) on host arrays x, y (y only for pow), n values.
 * include/egdst_math.h restates glibc's algorithms so that these equal the host libm bit for bit.
 * fn 3, 4: the interpolation of linter (egdst_lib.c:186-189), f0 (g1 - x) / (g1 - g0) + f1 (x - g0) / (g1 - g0), in the form the grid
 * kernels use (3: one refined reciprocal serves both quotients) and as written (4); x = [x | g0 | g1] (3n values), y = [f0 | f1] (2n). */
int egdst_math_eval(int fn, int n, const double *x, const double *y, double *out);

/* Quantiles p[0..np) of the host array x[0..n) by the device's selection: x is laid out as column 0 of an [n][1][nout] panel
 * (the other columns NaN) and k_quantiles runs on np kind-3 records.  NaNs in x do not qualify.  out [np], count [1].
 * EGDST_E_ARG if n < 1, np < 1 or a p is not inside (0, 1). */
int egdst_quantile_eval(int n, const double *x, int np, const double *p, double *out, int *count);
/* The band of egdst_simulate_batch_spec_cov's quantile records on the host array x, laid out as egdst_quantile_eval lays it out:
 * k_quantile_band runs on np kind-3 records with p[i] and bandwidth h[i].  out [np][3]: the order statistics a = Q(p - h) and
 * b = Q(p + h) and the sparsity s (all NaN when nothing qualifies); count [1].  EGDST_E_ARG for what egdst_quantile_eval refuses,
 * for an h that is 0, NaN or negative, and for p - h <= 0 or p + h >= 1. */
int egdst_quantile_band_eval(int n, const double *x, int np, const double *p, const double *h,
                             double *out /* [np][3]: a, b, s */, int *count);
/* Candidates (agents times periods of a kind-3 moment) up to which this library's k_quantiles gathers the keys into LDS
 * once; a moment with more reads its column from memory in every pass of the selection (build constant QNT_LDS_KEYS). */
int egdst_quantile_lds_keys(void);

/* Envelope walks of the last solve per draw: out[2*draw] = walks that were cut into segments (one wave each) and merged,
 * out[2*draw+1] = walks whose segment predictions failed the check and were redone by one wave (results are the same
 * either way; environment EGDST_NOSEG=1 at create turns the cutting off). */
int egdst_get_walk_stats(egdst_handle *h, unsigned *out /* [2*ndraw] */);
/* LDS-resident sorts of the envelope jobs of the last solve per draw (general envelope kernel and the cells of the tail launch), by
 * kind: out[4*draw] = every list already in order (merge or ranks), out[4*draw+1] = a list out of order, bitonic network,
 * out[4*draw+2] = a list out of order and the padded stream beyond the LDS capacity, counting ranks; out[4*draw+3] = those of
 * the last two kinds in which two or more threads of the workgroup each saw a pair out of order.  Results are the same. */
int egdst_get_sort_stats(egdst_handle *h, unsigned *out /* [4*ndraw] */);

/* Envelope step of the last solve per draw: out[2*draw] = (state, period) cells completed by the throughput path (five lean
 * kernels with one wave per envelope walk, used for batches of >= 512 cells per period; environment EGDST_ENV_TP=0/1 at
 * solve overrides), out[2*draw+1] = cells it left to the general kernel (an error condition, more than 64 monotone pieces
 * in a choice list, a failed draw, an infeasible state).  Results are the same either way. */
int egdst_get_tp_stats(egdst_handle *h, unsigned *out /* [2*ndraw] */);
/* Of the cells the throughput path left over (out[2*draw+1] above): those of the second tier of stage 1 (lists beyond the regular
 * stream budget) that gave up and were done in place by the workgroup of the period's tail launch that held them. */
int egdst_get_tp_inplace(egdst_handle *h, unsigned *out /* [ndraw] */);
/* The two lists of every period's tail launch in the last solve, per draw group: entries of rest[g*nt + it] (cells left over) and
 * big[g*nt + it] (second-tier cells), for the first max_groups groups (the library has at most 32). */
int egdst_get_tp_tail_counts(egdst_handle *h, int max_groups, int *rest /* [max_groups*nt] */, int *big /* [max_groups*nt] */);

/* Raw device views for callers that keep data resident (bench, estimation loops). */
int egdst_device_tables(egdst_handle *h, int it, const double **M_dev, const double **C_dev, const double **V_dev,
                        const int **len_dev);

#ifdef __cplusplus
}
#endif
#endif
