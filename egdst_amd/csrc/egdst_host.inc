// egdst_host.inc -- host side of the C ABI (include/egdst.h): allocation, the period loop, export.
// Included at the end of egdst_kernels.hip so that the whole per-model library is one translation unit.

#define EGDST_MAX_GROUPS 32
#ifndef EG_STRAGGLER_CALLS   // (-DEG_STRAGGLER_CALLS=n: a checking build may lower it)
#define EG_STRAGGLER_CALLS 1000u
#endif
// -DEG_STRAGGLER_EVERY=n (checking builds): egdst_sync also takes every n-th draw (i % n == 1) for a straggler, so that a small
// case runs straggler lanes and a permuted draw order.  The counter alone cannot single draws out there: since the fixed points
// are fast-forwarded, Batch.work is 0 for every draw of the C2 cases, and with its floor lowered it is the same number for all.
#ifndef EG_STRAGGLER_EVERY
#define EG_STRAGGLER_EVERY 0
#endif
#define EG_ENV_WIDE_MAX_CELLS 128  // up to this many (draw, state) cells per solve k_envelope runs 512 threads wide
#define EG_GRID_WIDE_MAX_POINTS 131072  // grid points per period up to which k_grid_wide (16 lanes per point) is used
#if MS_ND == 1
#define EG_E1_NB(ngridm) ((size_t)(((ngridm) + E1_TILE - 1) / E1_TILE))  // tiles (workgroups) per cell of k_env1
#else
#define EG_E1_NB(ngridm) ((size_t)0)
struct Env1Tile { unsigned long long desc, evals; };
#endif
#ifndef EG_GRID_CV_DEFAULT
#define EG_GRID_CV_DEFAULT 0
#endif
#define EG_GRID_SAMPLED_ROWS 2048  // LDS rows of k_grid_lds' sampled index (tables too long to stage whole)
#define EG_NPROF 9      // kernel classes of egdst_get_profile
// The list-driven launches of a period (k_fixup, k_tp_tail): workgroups per EG_SPARSE_REF_CELLS cells of the
// group, never fewer than that many and never more than the cap (LaunchPlan, eg_sparse_grid).  The numbers per 256 cells are what
// was tuned with 16 groups of 256 draws of C2 (one cell per draw); a group of 1024 to 2048 draws has lists four to eight times as long.
#define EG_SPARSE_REF_CELLS 256
#define EG_FIX_GRID 32  // k_fixup; its workgroups take the streams k_fixup_scan listed by ticket
#define EG_FIX_GRID_MAX 512       // (two workgroups per CU, FIX_MINW)
#define EG_ENV_TP_MIN_CELLS 512   // (draw, state) cells per solve from which the throughput path of the envelope step is used
#define EG_ENV_TP_REST_GRID 32    // k_tp_tail: for the cells the throughput path left over ...
#define EG_ENV_TP_BIG_GRID 64     // ... and for the second tier of stage 1; the launch has the larger of the two,
#define EG_ENV_TP_GRID_MAX 256    // at most this many (a workgroup holds most of a CU's LDS: one per CU)
// -DEG_SPARSE_GRID_MAX=n (checking builds): at most n workgroups for each of them, so that a test's lists are many times
// longer than its launches are wide.  Default: no cap.
#define EG_ENV_TP_MAX_KEYS 5120   // points of a stream that the kernels of the throughput path keep in LDS (k_tp_walk: 24 B each)
#ifndef EG_TP_WALK_BS0
#define EG_TP_WALK_BS0 TP_WALK_BS  // threads of a stage-0 walk workgroup
#endif
#define EG_TP_WALK_LDS_PER_POINT 24  // k_tp_walk: M, V (8 B each), class word (4 B), function id and position list (2 B each)
#include <optional>
#include <vector>
// Environment switches of the library (INTEGRATION.md), read once when a handle is created: unset (nullopt) means the
// automatic choice, a set value is taken as atoi reads it.
struct Options {
    std::optional<int> noseg, lcap, groups, hwq, adaptive;   // EGDST_NOSEG, EGDST_LCAP, EGDST_GROUPS, GPU_MAX_HW_QUEUES, EGDST_ADAPTIVE
    std::optional<int> grid_wide, grid_lds, grid_cv;         // EGDST_GRID_WIDE, EGDST_GRID_LDS, EGDST_GRID_CV
    std::optional<int> env_tp, tp_lkcap, tp_sort_lkcap, tp_big, tp_bigcap;  // EGDST_ENV_TP, EGDST_TP_*
    std::optional<int> e1_defer_all;                         // EGDST_E1_DEFER_ALL
    bool no_env1, debug_sync, debug_poison;                  // set at all: EGDST_NO_ENV1, EGDST_DEBUG_SYNC, EGDST_DEBUG_POISON
};
// What the launches of a solve look like: fixed for a handle by its geometry, its options and the kernels' attributes.
struct LaunchPlan {
    bool grid_wide;      // a batch that leaves the GPU mostly idle spreads every grid point over 16 lanes (k_grid_wide)
    int grid_lrows;      // LDS rows of M columns of k_grid_lds (0: the general k_grid)
    bool grid_sampled;   // those rows are a sampled index of tables too long to stage whole
    bool sortcheck;      // k_sortcheck before the probe (the sampled index needs ordered M columns)
    bool grid_cv;        // k_grid_lds_cv: whole tables (M, C, V) in LDS
    bool e1_on;          // single-choice models: k_env1 compacts the regular cells
    int e1_defer_all;    // tests: k_env1 hands every cell to k_envelope (1: before its tiles write rows, 2: after)
    bool env_parts;      // several choices: per-choice workgroups of k_envelope (off while the kink log is on)
    bool env_tp;         // several choices: the throughput path of the envelope step (off while the kink log is on)
    int tp_lkcap, tp_lkcap0, tp_scap0, tp_scap1, tp_bigcap;  // stream budgets of the throughput path's kernels
    bool tp_big;         // second tier of stage 1 (k_tp_tail's second list)
    int tp_walk_bs0;     // threads of a stage-0 walk workgroup
    int fix_wg, tp_big_wg, tp_rest_wg;              // workgroups per EG_SPARSE_REF_CELLS cells of a group: k_fixup, and k_tp_tail's for its second tier and for its leftover cells
    int fix_wg_max, tp_big_wg_max, tp_rest_wg_max;  // and the most of each (eg_sparse_grid)
};
struct egdst_handle {
    Batch b;
    egdst_desc desc;
    hipStream_t stream;
    int own_stream;
    int keep_history;
    int params_set;
    int solved;
    int call_slot_ok;  // the device copy of `b` for launches outside a solve is current (batch_for_call)
    unsigned solve_seq;  // solves enqueued so far (base of the k_sortcheck stamps)
    unsigned char *imported;  // per draw: cells were imported since the last solve (import_begin)
    void *pool;        // one device allocation for everything
    Batch *b_dev;      // device copies of `b` the kernels read (constant address space): one per draw group with its draw0,
    Batch *b_host;     // and entry EGDST_MAX_GROUPS for the launches outside a solve; pinned staging of the same
    // simulator buffers, grown on demand and kept (egdst_simulate*, egdst_simulate_batch_moments, egdst_simulate_batch_spec)
    double *sim_init, *sim_rs, *sim_sims, *sim_means;
    int *sim_err, *sim_counts;
    size_t sim_init_bytes, sim_rs_bytes, sim_sims_bytes, sim_means_bytes, sim_err_bytes, sim_counts_bytes;
    egdst_moment_lag *sim_spec; // estimation_step: the moment records (egdst_simulate_batch_spec[_lag]), the target and the weighting
    double *sim_tgt, *sim_W;    // matrix, or its diagonal (egdst_simulate_batch_moments)
    size_t sim_spec_bytes, sim_tgt_bytes, sim_W_bytes;
    double *sim_scores;         // egdst_simulate_batch_spec_cov: the per-agent scores of a slice of draws, [nd][nsim][cov_padded(nmom)]
    size_t sim_scores_bytes;
    double *sim_band;           // the same entry on a spec with a banded quantile: the sparsities k_quantile_band writes, [ndraw][nmom]
    size_t sim_band_bytes;
    // egdst_policy_batch: the observations, their grouping by cell (permutation, workgroup items), and the terms of a slice of draws
    egdst_obs *pol_obs;
    int *pol_perm, *pol_flag;
    PolItem *pol_items;
    double *pol_term;
    size_t pol_obs_bytes, pol_perm_bytes, pol_flag_bytes, pol_items_bytes, pol_term_bytes;
    // egdst_attach_panel: a panel resident on the device (the same grouping), its items indexed by period, and the terms of ALL
    // draws, [ndraw][nobs], which every solve rewrites period by period (k_policy_period) and egdst_fit_dev reduces
    egdst_obs *pan_obs;
    int *pan_perm, *pan_flag;
    PolItem *pan_items;
    double *pan_term;
    int *pan_first;     // host, [nt + 1]: the items of period it are pan_items[pan_first[it] .. pan_first[it + 1])
    int pan_nobs, pan_resid;   // pan_nobs > 0: a panel is attached
    int pan_fit;        // a solve enqueued since the attach wrote the terms, and nothing was imported since
    size_t klog_bytes;  // kink log (egdst_set_dbgout), allocated apart from the pool
    void **emu_items;  // sanitizer harness only: one heap block per array instead of the pool
    int emu_nitems;
    size_t pool_bytes;
    double *h_par;     // pinned staging for parameters
    char *scratch_lo, *scratch_hi;  // work arrays that hold no state across periods (diagnostic poisoning)
    int profile;                    // record HIP events around every launch of each kernel
    int lcap;                       // sorted points that fit k_envelope's dynamic LDS
    size_t lds_bytes;
    size_t tail_lds, tail_soff;     // k_tp_tail: its dynamic LDS, and where in it the second tier's TpShared lives
    Options opt;                    // environment switches, read at create
    LaunchPlan plan;                // launch decisions of a solve, made at create
    hipEvent_t *ev;                 // [groups][EG_NPROF kernel classes][nt][2]
    int nev;
    // draw groups: contiguous ranges of draws whose per-period kernels run on their own streams, so that a
    // draw with a long sequential stretch (a re-basing guess stream, a long envelope walk) only holds up its group
    int ngroups;                    // regular groups (egdst_set_groups)
    // schedule: slot -> draw (order) and the slot ranges of the groups.  Regular groups first; after a solve in which
    // some draws spent long in re-basing guess streams (Batch.work), those draws get lanes of their own at the end
    int nlanes;                     // groups in use = regular groups + straggler lanes
    int gstart[EGDST_MAX_GROUPS + 1];
    int *order_h;
    unsigned *work_h;
    unsigned char *strag_h;         // [ndraw] 1 = currently scheduled as a straggler
    int nstrag, adaptive, hwq;
    int auto_groups;                // ngroups is the library's own choice, revisited after every solve (eg_history_groups)
    hipStream_t gstream[EGDST_MAX_GROUPS];   // of groups 1 ..; group 0 runs on `stream`
    hipEvent_t fork_ev, join_ev[EGDST_MAX_GROUPS];
};

static thread_local char g_err[512];

static int set_err(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

#define HIPCHK(call)                                                                                    \
    do {                                                                                                \
        hipError_t e_ = (call);                                                                         \
        if (e_ != hipSuccess) return set_err(EGDST_E_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); \
    } while (0)
// inside egdst_create_compact: a failure destroys the partially built handle `h` before returning
#define HIPCHK_H(call)                                                                       \
    do {                                                                                     \
        hipError_t e_ = (call);                                                              \
        if (e_ != hipSuccess) {                                                              \
            egdst_destroy(h);                                                                \
            return set_err(EGDST_E_HIP, "%s failed: %s", #call, hipGetErrorString(e_));      \
        }                                                                                    \
    } while (0)

extern "C" const char *egdst_last_error(void) { return g_err; }

extern "C" const char *egdst_strerror(int code)
{
    switch (code) {
    case EGDST_OK: return "ok";
    case EGDST_E_ARG: return "Error: bad argument";
    case EGDST_E_HIP: return "Error: HIP runtime failure";
    case EGDST_E_NOGPU: return "Error: no gfx950 device available (this library has no CPU fallback)";
    case EGDST_E_INTERP2: return "Error:\nError: At least two points are required for interpolation!";  // (error() puts its prefix before a text that has one, egdst_lib.c:172,183,299-302)
    case EGDST_E_TRPR_SUM: return "Error:\nTransition probabilities don't sum up! Check model specification!";
    case EGDST_E_NO_SAVINGS: return "Error:\nFailed to find any value of savings to result in positive consumption next period! Increase mmax.";
    case EGDST_E_GRID_FULL: return "Error:\nNot enough space for endogenous grid. Increase max number of grid points for M!";
    case EGDST_E_EMPTY_CHOICESET: return "Error:\nEmpty choiceset encountered! Check model specifications!";
    case EGDST_E_ALL_NEG_INF: return "Error:\nAll of the choices lead to -inf value functions for all values of money-at-hand!";
    case EGDST_E_ENVELOPE: return "Error:\nFailed to compute upper envelope, most likely individual grids don't overlap!";
    case EGDST_E_ENV2_SPACE: return "Error:\nNot enough space for endogenous grid in envelop2()";
    case EGDST_E_ENV2_SEGMENTS: return "Error:\n10000 is not enough in envelop2()";
    case EGDST_E_ADRAW_INIT: return "Error:\nCould not complete initial stage in adraw()..\nSeems like M(a0)>mmax! Increase mmax!";
    case EGDST_E_THRH_FULL: return "Error:\nNot enough space for thresholds. Increase max number of threshold points!";
    case EGDST_E_TWO_ANALYTIC: return "Error:\nFatal error in threshold module. Two analytical value functions seem to intersect. Utility is not additively separable in consumption and discrete choices.";
    case EGDST_E_BRACKET_OUT: return "Error:\nFatal error in braketing module! Solution is outside of brackets.";
    case EGDST_E_BRACKET_REV: return "Error:\nFatal error in braketing module! Bracket limits reversed.";
    case EGDST_E_BUDGET_INVERT: return "Error:\nDid not manage to invert the intertemporal budget (cashinhand) after performing many-many iterations!";
    case EGDST_E_TRPR_CASES: return "Error in trpr: unknown combination of current state and decision (the set of cases is not complete)!";
    case EGDST_E_RESEND_IN_GRID: return "Error: zero-consumption resend requested inside the parallel grid stage (not supported by this build)";
    case EGDST_E_INTERNAL: return "Error: internal scratch exhausted";
    case EGDST_E_CAPACITY: return "Compact capacity exceeded: this draw needs more rows than rows_cap; solve it with egdst_create (exact capacities)";
    case EGDST_E_NOT_SOLVED: return "Error: the model has not yet been solved!";
    case EGDST_E_RAND_SHORT: return "Error: randstream is too short to be used for all requested simulations!";
    case EGDST_E_SIM_STATE: return "Error: simulated transition left the state space";
    default: return "Error: unknown code";
    }
}

extern "C" int egdst_get_model_info(egdst_model_info *o)
{
    if (!o) return set_err(EGDST_E_ARG, "null info");
    o->nst = MS_NST;
    o->nd = MS_ND;
    o->nnst = MS_NNST;
    o->nnd = MS_NND;
    o->nparam = MS_NPARAM;
    o->neq = MS_NEQ;
    o->distrib = MS_DISTRIB;
    o->optim_MUnoD = MS_OPTIM_MUNOD;
    o->optim_UnoD = MS_OPTIM_UNOD;
    o->optim_UasD = MS_OPTIM_UASD;
    o->optim_TRPRnoSH = MS_OPTIM_TRPRNOSH;
    o->tolerance = MS_TOLERANCE;
    o->zeroconsumption = MS_ZEROCONSUMPTION;
    o->doublepoint_delta = MS_DOUBLEPOINT_DELTA;
    o->label = MS_LABEL;
    return 0;
}

static size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

#ifndef EGDST_EMU
// hipFuncAttributeMaxDynamicSharedMemorySize is a property of the kernel for the whole process, not of a handle: keep
// it at the largest size any handle of this library has asked for (a later handle with a smaller grid must not lower
// it below what an earlier, still live handle launches with).
// (the attribute is kept per DEVICE by the runtime: the cache is keyed by the current device and guarded by a mutex, so that
//  handles created on a second card, or from two threads at once, neither skip nor race the reservation)
#include <mutex>
static hipError_t eg_reserve_envelope_lds(size_t bytes)
{
    static std::mutex mu;
    static size_t reserved[64] = {0};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lock(mu);
    const bool cached = dev >= 0 && dev < 64;
    if (cached && bytes <= reserved[dev]) return hipSuccess;
    e = hipFuncSetAttribute((const void *)k_envelope, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess && cached) reserved[dev] = bytes;
    return e;
}
#endif

// The only place that reads the environment.
static Options read_options()
{
    auto num = [](const char *name) -> std::optional<int> {
        const char *v = getenv(name);
        if (!v) return std::nullopt;
        return atoi(v);
    };
    Options o;
    o.noseg = num("EGDST_NOSEG");
    o.lcap = num("EGDST_LCAP");             // tests: a small value sends every stream down the global path
    o.groups = num("EGDST_GROUPS");
    o.hwq = num("GPU_MAX_HW_QUEUES");       // what the HIP runtime was started with
    o.adaptive = num("EGDST_ADAPTIVE");
    o.grid_wide = num("EGDST_GRID_WIDE");
    o.grid_lds = num("EGDST_GRID_LDS");     // 0: the general k_grid
    o.grid_cv = num("EGDST_GRID_CV");
    o.env_tp = num("EGDST_ENV_TP");
    o.tp_lkcap = num("EGDST_TP_LKCAP");     // tests: a small value exercises the sampled key index
    o.tp_sort_lkcap = num("EGDST_TP_SORT_LKCAP");
    o.tp_big = num("EGDST_TP_BIG");
    o.tp_bigcap = num("EGDST_TP_BIGCAP");
    o.e1_defer_all = num("EGDST_E1_DEFER_ALL");
    o.no_env1 = getenv("EGDST_NO_ENV1") != nullptr;
    o.debug_sync = getenv("EGDST_DEBUG_SYNC") != nullptr;     // diagnostic: name the kernel a fault belongs to
    o.debug_poison = getenv("EGDST_DEBUG_POISON") != nullptr; // diagnostic: no kernel may rely on stale work arrays
    return o;
}

static LaunchPlan plan_launches(const Geom &g, const Options &o)
{
    LaunchPlan p = {};
    p.grid_wide = o.grid_wide ? *o.grid_wide != 0 : (long long)g.ndraw * MS_NST * MS_ND * g.ngridm <= EG_GRID_WIDE_MAX_POINTS;
    // rows of next-period M columns a k_grid_lds workgroup stages (dynamic LDS): room for the regular points of every
    // next state plus the kinks an envelope adds; a period whose tables need more falls back to the general path by itself
    const long long lrows_all = (long long)MS_NST * (g.ngridm + g.ngridm / 2 + 64);
    int grid_lrows = (int)(lrows_all < EG_GRID_LROWS_MAX ? lrows_all : EG_GRID_LROWS_MAX);
    if (o.grid_lds) grid_lrows = *o.grid_lds;
    if (MS_NST * 4 > grid_lrows) grid_lrows = 0;
    p.grid_sampled = lrows_all > (long long)grid_lrows;
    // A sampled index is staged with strided global reads by a workgroup that evaluates 256 points only: a coarser one is
    // cheaper to stage than its longer window search costs.  Measured (rows: C4 x 32 draws / C5 x 128 draws per step):
    // 16384: 168 ms / 14.0 s, 8192: 100 ms / 7.7 s, 4096: 73 ms / 4.82 s, 2048: 64 ms / 4.32 s, 1024: 65 ms / 4.45 s,
    // 512: 65 ms / 4.59 s.  (More points per workgroup instead: the loop costs 32 VGPRs and two waves of occupancy, 78 ms.)
    // (round 4, workgroups of 1024 points -- the C4 batch build -- share an index among four times the points: 3072 rows, 46.3 ms against
    //  47.1 for C4 x 32; 4096: 46.5, 1024: 47.7.  C5 x 128 at 256 points per workgroup: 2048 rows 3.31 s, 4096: 4.35 s, 1024: 3.39 s.)
    const int sampled_rows = (GRID_BS >= 1024) ? EG_GRID_SAMPLED_ROWS * 3 / 2 : EG_GRID_SAMPLED_ROWS;
    if (p.grid_sampled && !o.grid_lds && grid_lrows > sampled_rows) grid_lrows = sampled_rows;
#ifdef EGDST_EMU
    if (grid_lrows > 20480) grid_lrows = 20480;
#endif
    p.grid_lrows = grid_lrows;
    // tables that may not fit the LDS whole: the sampled form of k_grid_lds needs to know that their M columns are in order
    // (k_sortcheck), and with that knowledge the expectations of k_probe / k_fixup need one bracket search instead of two
    p.sortcheck = !p.grid_wide && grid_lrows > 0 && p.grid_sampled && g.nt < 4095;  // (the stamps hold the period in 12 bits)
    // whole tables (M, C, V) in LDS when they fit 48 KB (k_grid_lds_cv)
    p.grid_cv = !p.grid_sampled && grid_lrows > 0 && 24 * (long)grid_lrows <= 48 * 1024 &&
                (o.grid_cv ? *o.grid_cv != 0 : EG_GRID_CV_DEFAULT != 0);
#if MS_ND == 1
    // single-choice models: the regular cells are compacted by many workgroups (k_env1_*), k_envelope takes the rest
    p.e1_on = !o.no_env1;
    p.e1_defer_all = o.e1_defer_all ? (*o.e1_defer_all == 2 ? 2 : 1) : 0;
    // (the throughput path is for models with several choices: env_tp stays false)
#else
    // several choices: the choice lists and their secondary envelopes as workgroups of their own (part 1), then the primary
    // envelope per cell (part 2); one workgroup per cell (part 0) when the kink log is on (its rows are ordered) -- for
    // batches that leave CUs idle (measured: C3 single solve 42 -> 25 ms; C2 x 4096 274 -> 300 ms, where a workgroup
    // that only compacts a list still takes a CU's LDS)
    p.env_parts = g.ndraw * MS_NST <= EG_ENV_WIDE_MAX_CELLS;
    // Batches with many cells per period: the throughput path (k_tp_*: five lean kernels, one wave per walk, streams in global
    // memory) does the regular cells, k_envelope (pass 1) the cells it left flagged in b.defer.  Not for the terminal period
    // (one of nt), not with the kink log (its rows are ordered per cell), not for streams that a single wave should not walk
    // alone (C5: 65 536 points per stream and few cells -- there the segmented walk of k_envelope is the right tool).
    // points of a stream the kernels keep in LDS, per stage: a folded choice list with its extrapolation points (stage 0), the
    // lists of all choices (stage 1); the kinks of the envelopes add a few rows each.  Longer streams -- degenerate guess
    // streams -- are left to k_envelope.  (LDS per workgroup decides how many walks share a CU: measured on C2 x 4096,
    // 2100 entries 201.7 ms, 2314: 209.8 ms, 3000: 225 ms.)
    const long tp_keys = (long)MS_ND * g.ngridm + (long)g.ngridm / 10 + 64;
    const long tp_keys0 = (long)g.ngridm + (long)g.ngridm / 8 + 64;
    // (Measured slower and removed: the walks of streams too long for the walk's LDS (C5, C3) over global memory,
    //  k_tp_walk_g -- C5 x 128 3.89 s against 3.75 s, C3 x 64 51.5 against 37.7 ms, C5 x 16 720 against 763 ms.)
    p.env_tp = o.env_tp ? *o.env_tp != 0 : ((long)g.ndraw * MS_NST >= EG_ENV_TP_MIN_CELLS && tp_keys <= EG_ENV_TP_MAX_KEYS);
    int tp_lkcap = (int)(tp_keys < EG_ENV_TP_MAX_KEYS ? tp_keys : EG_ENV_TP_MAX_KEYS);
#ifndef EGDST_EMU
    {   // three walks per CU where a slightly smaller stream budget buys that (C2: 2164 -> ~2060 points, streams hold ~2010)
        hipFuncAttributes fa;
        if (hipFuncGetAttributes(&fa, (const void *)k_tp_walk) == hipSuccess) {
            const long cap3 = ((long)160 * 1024 / 3 - (long)fa.sharedSizeBytes - 512) / EG_TP_WALK_LDS_PER_POINT;
            if (tp_lkcap > cap3 && cap3 >= (long)MS_ND * g.ngridm + 24) tp_lkcap = (int)cap3;
        }
    }
#else
    if (tp_lkcap > 6500) tp_lkcap = 6500;  // (the harness' static stand-in for the dynamic LDS, with its poisoned gaps)
#endif
    if (o.tp_lkcap) tp_lkcap = *o.tp_lkcap;
    p.tp_lkcap = tp_lkcap;
    p.tp_lkcap0 = (int)(tp_keys0 < tp_lkcap ? tp_keys0 : tp_lkcap);
    // tests: so few keys that the sorts work on a sampled index of them and write the permutation through global memory
    const int tp_skcap = o.tp_sort_lkcap.value_or(0);
    p.tp_scap0 = tp_skcap ? tp_skcap : p.tp_lkcap0;
    p.tp_scap1 = tp_skcap ? tp_skcap : tp_lkcap;
    // second tier of stage 1: lists beyond the regular stream budget that still fit the largest one (EGDST_TP_BIG=0: off, such
    // cells are k_envelope's as in round 3)
    int tp_bigcap = (int)(tp_keys * 2 < EG_ENV_TP_MAX_KEYS ? tp_keys * 2 : EG_ENV_TP_MAX_KEYS);
#ifdef EGDST_EMU
    if (tp_bigcap > 6500) tp_bigcap = 6500;
#endif
    if (o.tp_bigcap) tp_bigcap = *o.tp_bigcap;
    if (tp_bigcap > EG_ENV_TP_MAX_KEYS) tp_bigcap = EG_ENV_TP_MAX_KEYS;  // (what the kernels' dynamic LDS is reserved for)
    p.tp_bigcap = tp_bigcap;
    p.tp_big = !tp_skcap && tp_bigcap > tp_lkcap && tp_bigcap < 65536 && (o.tp_big ? *o.tp_big != 0 : true);
    // threads of a stage-0 walk workgroup (all load the stream, its waves walk segments of it); stage 1 uses TP_WALK_BS
    p.tp_walk_bs0 = (EG_TP_WALK_BS0 < WAVE || EG_TP_WALK_BS0 > TP_WALK_BS || EG_TP_WALK_BS0 % WAVE) ? TP_WALK_BS : EG_TP_WALK_BS0;
#endif
    p.fix_wg = EG_FIX_GRID, p.fix_wg_max = EG_FIX_GRID_MAX;
    p.tp_big_wg = EG_ENV_TP_BIG_GRID, p.tp_rest_wg = EG_ENV_TP_REST_GRID;
    p.tp_big_wg_max = p.tp_rest_wg_max = EG_ENV_TP_GRID_MAX;
    return p;
}

// Workgroups of a list-driven launch of a group with `cells` cells whose list holds at most `entries`: `per_ref` per
// EG_SPARSE_REF_CELLS cells (at least that many: the small groups keep what they had), at most `most`.  A workgroup that finds
// the list exhausted leaves at once.
static unsigned eg_sparse_grid(unsigned cells, unsigned entries, int per_ref, int most)
{
    unsigned n = (unsigned)(((unsigned long long)cells * (unsigned)per_ref + EG_SPARSE_REF_CELLS - 1) / EG_SPARSE_REF_CELLS);
    if (n < (unsigned)per_ref) n = (unsigned)per_ref;
    if (n > (unsigned)most) n = (unsigned)most;
#ifdef EG_SPARSE_GRID_MAX
    if (n > (unsigned)(EG_SPARSE_GRID_MAX)) n = (unsigned)(EG_SPARSE_GRID_MAX);
#endif
    return n < entries ? n : entries;
}

#if MS_ND > 1
static size_t tp_sort_lds(int cap)  // keys, class words, and the permutation at the next power of two (k_tp_sort)
{
    int p2 = 1;
    while (p2 < cap) p2 <<= 1;
    return (size_t)12 * cap + (size_t)2 * p2 + 64;
}
#endif

// Regular groups of a handle.  Group 0 runs on the handle's stream and every other group on a stream of its own.  The runtime gives
// a stream a hardware queue of its own while it has made fewer than GPU_MAX_HW_QUEUES of them; a stream that comes after that shares
// a queue with an earlier one, which one is not ours to say, and the null stream has a queue in nearly every process (hipMemcpy uses
// it): the queues that can each run one chain of a solve are those beside the null stream's.
static int eg_chain_queues(int hwq) { return hwq > 1 ? hwq - 1 : 1; }
// At create.  Ten queues or more: the counts measured with 24 (DESIGN.md section 5).  Fewer: 4 groups from 1024 cells, whatever the
// queues -- batches whose kernels fill the GPU (C5 x 128, C2 with a0 = 0) lose little where two of their groups share a queue and
// more with a group fewer (4 queues: 3.58 against 3.88 s, 181 against 193 ms).
static int eg_default_groups(int hwq, long cells)
{
    if (hwq >= 10) return cells >= 1024 && hwq >= 20 ? 16 : (cells >= 512 ? 8 : (cells >= 64 ? 4 : 1));
    return cells >= 1024 ? 4 : 1;
}
// After a solve (egdst_sync, while the count is the library's own and history-based scheduling is on).  A chain that is mostly
// list-driven launches -- a few workgroups, each a long sequential stretch -- fills nothing, and two such chains on one queue run end
// to end: C2 x 4096 with a0 = -5 on 4 queues, 273 ms with 4 groups against 176 with 3.  Such a handle gets no more groups than chain
// queues.  The measure is the share of the guess streams that k_fixup regenerated in the solve, on handles whose envelope step takes the
// throughput path (the others have no list-driven launch besides k_fixup): 1.4 % on that batch, 0.16 % with a0 = 0; the line is drawn
// between the two at their geometric mean.
#define EG_SPARSE_HEAVY_SHARE 0.005
static int eg_history_groups(int hwq, long cells, bool env_tp, double regen_share)
{
    const int g = eg_default_groups(hwq, cells), q = eg_chain_queues(hwq);
    return (env_tp && regen_share >= EG_SPARSE_HEAVY_SHARE && g > q) ? q : g;
}

extern "C" int egdst_create(const egdst_desc *d, int ndraw, int keep_history, void *stream, egdst_handle **out)
{
    return egdst_create_compact(d, ndraw, keep_history, 0, stream, out);
}

extern "C" int egdst_create_compact(const egdst_desc *d, int ndraw, int keep_history, int rows_cap, void *stream,
                                    egdst_handle **out)
{
    if (!d || !out || ndraw < 1) return set_err(EGDST_E_ARG, "egdst_create: null descriptor/handle or ndraw<1");
    if (rows_cap < 0) return set_err(EGDST_E_ARG, "egdst_create_compact: rows_cap < 0");
    if (d->T < d->t0 || d->ngridm < 2 || d->ny < 1 || !d->quadrature || d->nthrhmax < 1)
        return set_err(EGDST_E_ARG, "egdst_create: inconsistent descriptor");
    if ((long long)MS_NST * d->ny > 65535)  // a candidate's evaluation count is packed in 16 bits (eg_sc_pack) and read back as a result
        return set_err(EGDST_E_ARG, "egdst_create: more than 65535 (next state, shock node) terms per evaluation");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return set_err(EGDST_E_NOGPU, "%s", egdst_strerror(EGDST_E_NOGPU));
    egdst_handle *h = (egdst_handle *)calloc(1, sizeof(egdst_handle));
    h->desc = *d;
    Geom &g = h->b.g;
    g.t0 = d->t0;
    g.T = d->T;
    g.nt = d->T - d->t0 + 1;
    g.ngridm = d->ngridm;
    g.ngridmax = d->ngridmax <= d->ngridm ? 2 * d->ngridm : d->ngridmax;  // egdstmodel.m:1145-1147
    g.nthrhmax = d->nthrhmax;
    g.ny = d->ny;
    g.ndraw = ndraw;
    g.nslots = keep_history ? g.nt : 2;
    g.S = g.ngridmax + 1;
    g.Cp = g.ngridmax;
    if (rows_cap > 0 && rows_cap < g.ngridmax) g.Cp = rows_cap < g.ngridm + 2 ? g.ngridm + 2 : rows_cap;
    g.Sp = g.Cp + 1;
    g.mmax = d->mmax;
    g.a0 = d->a0;
    h->keep_history = keep_history;
    h->opt = read_options();
    h->plan = plan_launches(g, h->opt);
    h->b.noseg = h->opt.noseg.value_or(0);
    if (stream) {
        h->stream = (hipStream_t)stream;
    } else {
        HIPCHK_H(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
        h->own_stream = 1;
    }
    // ---- carve one pool ---------------------------------------------------------------------
    const size_t nds = (size_t)ndraw * MS_NST;
    const size_t ntab = (size_t)g.nslots * nds;
    const size_t ncand = nds * MS_ND * (size_t)g.Cp;
    const size_t W = nds * (size_t)(MS_ND + 1) * g.Cp;
    const size_t nenv = nds * (size_t)g.Cp, nenvth = nds * MS_ND * (size_t)g.nthrhmax;
    size_t off = 0;
    struct Item { void **p; size_t bytes; };
    Batch &b = h->b;
    Item items[] = {
        {(void **)&b.par, sizeof(double) * (size_t)ndraw * (MS_NPARAM ? MS_NPARAM : 1)},
        {(void **)&b.qw, sizeof(double) * g.ny}, {(void **)&b.qz, sizeof(double) * g.ny},
        {(void **)&b.tM, sizeof(double) * ntab * g.Sp}, {(void **)&b.tC, sizeof(double) * ntab * g.Sp},
        {(void **)&b.tV, sizeof(double) * ntab * g.Sp},
        {(void **)&b.tD, sizeof(double) * ntab * g.nthrhmax}, {(void **)&b.tTH, sizeof(double) * ntab * g.nthrhmax},
        {(void **)&b.tlen, sizeof(int) * ntab}, {(void **)&b.tthlen, sizeof(int) * ntab},
        {(void **)&b.thw, sizeof(int) * ntab}, {(void **)&b.thhw, sizeof(int) * ntab},
        {(void **)&b.defer, sizeof(int) * nds},
        {(void **)&b.cM, sizeof(double) * ncand}, {(void **)&b.cC, sizeof(double) * ncand},
        {(void **)&b.cV, sizeof(double) * ncand},
        {(void **)&b.cSt, sizeof(int) * ncand},
        {(void **)&b.probe, sizeof(ProbeOut) * nds * MS_ND},
        {(void **)&b.pM, sizeof(double) * W}, {(void **)&b.pC, sizeof(double) * W}, {(void **)&b.pV, sizeof(double) * W},
        {(void **)&b.pF, sizeof(int) * W},
        {(void **)&b.sM, sizeof(double) * W}, {(void **)&b.sC, sizeof(double) * W}, {(void **)&b.sV, sizeof(double) * W},
        {(void **)&b.sF, sizeof(int) * W},
        {(void **)&b.qM, sizeof(double) * W}, {(void **)&b.qC, sizeof(double) * W}, {(void **)&b.qV, sizeof(double) * W},
        {(void **)&b.qF, sizeof(int) * W},
        {(void **)&b.rank, sizeof(int) * W}, {(void **)&b.gcls, sizeof(int) * W},
        {(void **)&b.eM, sizeof(double) * nenv}, {(void **)&b.eV, sizeof(double) * nenv},
        {(void **)&b.eC, sizeof(double) * nenv}, {(void **)&b.eTH, sizeof(double) * nenvth},
        {(void **)&b.eIX, sizeof(double) * nenvth},
        {(void **)&b.status, sizeof(int) * ndraw}, {(void **)&b.where, sizeof(int) * 2 * ndraw},
        {(void **)&b.evals, sizeof(unsigned long long) * ndraw},
        {(void **)&b.credited, sizeof(unsigned long long) * ndraw},
        {(void **)&b.segstat, sizeof(unsigned) * 2 * ndraw}, {(void **)&b.sortstat, sizeof(unsigned) * 4 * ndraw},
        {(void **)&b.dbg, sizeof(int) * 16 * ndraw},
        {(void **)&b.algbytes, sizeof(unsigned long long) * ndraw},
        {(void **)&b.obj, sizeof(double) * 2 * ndraw},
        {(void **)&b.order, sizeof(int) * ndraw}, {(void **)&b.work, sizeof(unsigned) * ndraw},
        {(void **)&b.nregen, sizeof(unsigned) * ndraw},
        {(void **)&b.fixn, sizeof(int) * EGDST_MAX_GROUPS * g.nt}, {(void **)&b.fixlist, sizeof(int) * nds * MS_ND},
        {(void **)&b.tickets, sizeof(int) * 2 * EGDST_MAX_GROUPS * g.nt},
        {(void **)&b.negflag, sizeof(int) * nds * MS_ND}, {(void **)&b.tsorted, sizeof(int) * nds},
        {(void **)&b.secn, sizeof(int) * nds * MS_ND}, {(void **)&b.secact, sizeof(int) * nds * MS_ND},
        {(void **)&b.secerr, sizeof(int) * nds * MS_ND}, {(void **)&b.secev, sizeof(double) * nds * MS_ND},
        {(void **)&b.secevals, sizeof(unsigned long long) * nds * MS_ND},
        {(void **)&b.tprec, sizeof(TpRec) * nds * MS_ND}, {(void **)&b.tpcell, sizeof(TpCell) * nds},
        {(void **)&b.tpn, sizeof(int) * EGDST_MAX_GROUPS * g.nt}, {(void **)&b.tplist, sizeof(int) * nds},
        {(void **)&b.tpbign, sizeof(int) * EGDST_MAX_GROUPS * g.nt}, {(void **)&b.tpbiglist, sizeof(int) * nds},
        {(void **)&b.tpstat, sizeof(unsigned) * 2 * ndraw}, {(void **)&b.tpinplace, sizeof(unsigned) * ndraw},
        EG_STAMP_DECL({(void **)&b.stamps, sizeof(unsigned long long) * EG_NSTAMP * ndraw},)
#if MS_ND == 1
        {(void **)&b.e1tiles, sizeof(Env1Tile) * nds * EG_E1_NB(d->ngridm)}, {(void **)&b.e1done, sizeof(unsigned) * nds},
#endif
    };
    const int nitems = sizeof(items) / sizeof(items[0]);
#ifdef EGDST_EMU
    // Sanitizer harness: every array is its own heap block of exactly its size, so that AddressSanitizer's red zones
    // sit between neighbours and an overrun from one array into the next traps (one pool would hide it).
    h->emu_nitems = nitems;
    h->emu_items = (void **)calloc(nitems, sizeof(void *));
    for (int i = 0; i < nitems; i++) {
        h->emu_items[i] = calloc(items[i].bytes ? items[i].bytes : 1, 1);
        *items[i].p = h->emu_items[i];
        off += items[i].bytes;
    }
    h->pool_bytes = off;
#else
    for (int i = 0; i < nitems; i++) off += align_up(items[i].bytes);
    h->pool_bytes = off;
    hipError_t e = hipMalloc(&h->pool, off);
    if (e != hipSuccess) {
        egdst_destroy(h);
        return set_err(EGDST_E_HIP, "hipMalloc(%zu bytes) failed: %s", off, hipGetErrorString(e));
    }
    off = 0;
    for (int i = 0; i < nitems; i++) {
        *items[i].p = (char *)h->pool + off;
        off += align_up(items[i].bytes);
    }
#endif
    {   // dynamic LDS of k_envelope, 32 B per sorted point (M, C, V, class word, 16-bit function id and position):
        // room for 1.5x the regular points of all choices, at most ~150 KiB (one workgroup per CU)
        long want = (long)MS_ND * g.ngridm * 3 / 2 + 64;
        if (want > 4200) want = 4200;  // 131 KB next to the 26 KB of static bookkeeping arrays
        if (h->opt.lcap) want = *h->opt.lcap;
#ifndef EGDST_EMU
        {   // what the kernel's own static arrays leave of the CU's 160 KiB
            hipFuncAttributes fa;
            if (hipFuncGetAttributes(&fa, (const void *)k_envelope) == hipSuccess) {
                const long room = ((long)160 * 1024 - (long)fa.sharedSizeBytes) / 32;
                if (want > room) want = room;
            }
        }
#endif
        h->lcap = (int)want;
        h->lds_bytes = (size_t)h->lcap * 32;
        // (Measured slower and removed: a first launch with a small LDS budget so that two workgroups share a CU, the
        //  cells that need more deferred to a second launch -- two co-resident walks cost each other ~1.55x, DESIGN.md §5.)
#ifndef EGDST_EMU
        HIPCHK_H(eg_reserve_envelope_lds(h->lds_bytes));
#if MS_ND > 1
        // the kernels of the throughput path may ask for more than the default 64 KB of dynamic LDS (a constant per kernel)
        HIPCHK_H(hipFuncSetAttribute((const void *)k_tp_sort, hipFuncAttributeMaxDynamicSharedMemorySize, 12 * EG_ENV_TP_MAX_KEYS + 2 * 8192 + 64));
        HIPCHK_H(hipFuncSetAttribute((const void *)k_tp_walk, hipFuncAttributeMaxDynamicSharedMemorySize, EG_TP_WALK_LDS_PER_POINT * EG_ENV_TP_MAX_KEYS));
#endif
#else
        if (h->lcap > 20480 * 8 / 32) h->lcap = 20480 * 8 / 32;  // the harness' static stand-in for the dynamic LDS
#endif
#if MS_ND > 1
        {   // k_tp_tail: the leftover cells get k_envelope's lcap and LDS, the second tier its streams (sort, then walk, in the
            // same bytes) and, past them, its TpShared.  The kernel's static LDS is k_envelope's and a few hundred bytes of the
            // second tier's helpers (its TpShared is in here); lcap is passed on as it is and the sum is checked, because an
            // lcap cut to fit would be silent and slow.
            const LaunchPlan &p = h->plan;
            const size_t walk_lds = (size_t)EG_TP_WALK_LDS_PER_POINT * p.tp_bigcap;
            const size_t big_lds = !p.tp_big ? 0 : (tp_sort_lds(p.tp_bigcap) > walk_lds ? tp_sort_lds(p.tp_bigcap) : walk_lds);
            h->tail_soff = (big_lds + 15) / 16 * 16;
            h->tail_lds = h->tail_soff + sizeof(TpShared) > h->lds_bytes ? h->tail_soff + sizeof(TpShared) : h->lds_bytes;
#ifndef EGDST_EMU
            hipFuncAttributes fa, fe;
            HIPCHK_H(hipFuncGetAttributes(&fa, (const void *)k_tp_tail));
            HIPCHK_H(hipFuncGetAttributes(&fe, (const void *)k_envelope));
            const size_t cu_lds = (size_t)160 * 1024;
            if (p.env_tp && fa.sharedSizeBytes + h->tail_lds > cu_lds) {
                egdst_destroy(h);
                return set_err(EGDST_E_HIP, "k_tp_tail: %zu B static (k_envelope: %zu) + %zu B dynamic LDS (lcap %d, second tier %zu) exceed %zu",
                               (size_t)fa.sharedSizeBytes, (size_t)fe.sharedSizeBytes, h->tail_lds, h->lcap, big_lds, cu_lds);
            }
            HIPCHK_H(hipFuncSetAttribute((const void *)k_tp_tail, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(cu_lds - fa.sharedSizeBytes)));
#else
            if (p.env_tp && h->tail_soff + (size_t)64 * 8 > sizeof(double) * (20480 + 64)) {  // (the stand-in, with the poisoned gaps of the second tier's regions)
                egdst_destroy(h);
                return set_err(EGDST_E_ARG, "k_tp_tail: the second tier's %zu B exceed the harness' stand-in for the dynamic LDS", h->tail_soff);
            }
#endif
        }
#endif
    }
#ifndef EGDST_EMU
    h->scratch_lo = (char *)b.cM;
    h->scratch_hi = (char *)b.status;
    HIPCHK_H(hipMemsetAsync(h->pool, 0, h->pool_bytes, h->stream));
#endif
    HIPCHK_H(hipMalloc(&h->b_dev, sizeof(Batch) * (EGDST_MAX_GROUPS + 1)));
    HIPCHK_H(hipHostMalloc((void **)&h->b_host, sizeof(Batch) * (EGDST_MAX_GROUPS + 1)));
    h->ngroups = 1;
    {
        const int hwq = h->opt.hwq.value_or(4);  // (the HIP runtime's default)
        const long cells = (long)ndraw * MS_NST;  // k_envelope workgroups per period
        int want = h->opt.groups ? *h->opt.groups : eg_default_groups(hwq, cells);
        h->hwq = hwq;
        h->adaptive = h->opt.adaptive.value_or(1);
        h->order_h = (int *)malloc(sizeof(int) * ndraw);
        h->work_h = (unsigned *)malloc(sizeof(unsigned) * ndraw);
        h->strag_h = (unsigned char *)calloc(ndraw, 1);
        int rc_ = egdst_set_groups(h, want);
        if (rc_) {
            egdst_destroy(h);
            return rc_;
        }
        h->auto_groups = !h->opt.groups;
    }
    // quadrature: weights as given, abscissae through the inverse normal cdf (egdst_solver.c:162-164)
    double *q = (double *)malloc(sizeof(double) * 2 * g.ny);
    for (int i = 0; i < g.ny; i++) {
        q[i] = d->quadrature[i];
        q[g.ny + i] = eg_inv_normal_cdf(d->quadrature[g.ny + i]);
    }
    hipError_t eq = hipMemcpyAsync((void *)b.qw, q, sizeof(double) * g.ny, hipMemcpyHostToDevice, h->stream);
    if (eq == hipSuccess) eq = hipMemcpyAsync((void *)b.qz, q + g.ny, sizeof(double) * g.ny, hipMemcpyHostToDevice, h->stream);
    if (eq == hipSuccess) eq = hipStreamSynchronize(h->stream);
    free(q);
    if (eq != hipSuccess) {
        egdst_destroy(h);
        return set_err(EGDST_E_HIP, "quadrature upload failed: %s", hipGetErrorString(eq));
    }
    h->desc.quadrature = nullptr;
    *out = h;
    return 0;
}

// Streams and join events of groups 1 .. n-1 (regular groups and straggler lanes).  Group 0 runs on the handle's own stream, which
// would otherwise sit idle, with a hardware queue behind it, from the fork to the join.
static int ensure_group_streams(egdst_handle *h, int n)
{
    if (!h->fork_ev) HIPCHK(hipEventCreateWithFlags(&h->fork_ev, hipEventDisableTiming));
    for (int g = 1; g < n; g++) {
        if (!h->gstream[g]) HIPCHK(hipStreamCreateWithFlags(&h->gstream[g], hipStreamNonBlocking));
        if (!h->join_ev[g]) HIPCHK(hipEventCreateWithFlags(&h->join_ev[g], hipEventDisableTiming));
    }
    return 0;
}

// Lay the draws out over the groups: the regular draws in index order, split evenly over the regular groups; the
// stragglers after them, on lanes of their own while hardware queues are left (one stream each needs one), otherwise
// dealt out over the regular groups.  Uploads the slot -> draw table on the handle's stream.
static int build_schedule(egdst_handle *h)
{
    const int nd = h->b.g.ndraw, G = h->ngroups;
    int spare = eg_chain_queues(h->hwq) - G;  // hardware queues not taken by the regular groups (group 0: the handle's stream) and the null stream
    if (spare > EGDST_MAX_GROUPS - G) spare = EGDST_MAX_GROUPS - G;
    if (spare > 8) spare = 8;
    const int lanes = (G > 1 && h->nstrag > 0 && spare > 0) ? (h->nstrag < spare ? h->nstrag : spare) : 0;
    const int nreg = nd - (lanes ? h->nstrag : 0);
    int k = 0;
    if (lanes) {
        for (int d = 0; d < nd; d++)
            if (!h->strag_h[d]) h->order_h[k++] = d;
        for (int gi = 0; gi <= G; gi++) h->gstart[gi] = (int)((long long)nreg * gi / G);
        // heaviest straggler first, each to the lane with the least re-basing work so far (the lanes run concurrently,
        // the draws of a lane hold up each other)
        const int ns = h->nstrag;
        int *sl = (int *)malloc(sizeof(int) * ns), *lane_of = (int *)malloc(sizeof(int) * ns), q = 0;
        unsigned long long load[EGDST_MAX_GROUPS] = {0};
        for (int d = 0; d < nd; d++)
            if (h->strag_h[d]) sl[q++] = d;
        for (int a = 1; a < ns; a++) {  // insertion sort by work, descending (a handful of entries)
            const int v = sl[a];
            int c = a - 1;
            for (; c >= 0 && h->work_h[sl[c]] < h->work_h[v]; c--) sl[c + 1] = sl[c];
            sl[c + 1] = v;
        }
        for (int a = 0; a < ns; a++) {
            int best = 0;
            for (int li = 1; li < lanes; li++)
                if (load[li] < load[best]) best = li;
            lane_of[a] = best;
            load[best] += h->work_h[sl[a]] + 1;
        }
        for (int li = 0; li < lanes; li++) {
            h->gstart[G + li] = k;
            for (int a = 0; a < ns; a++)
                if (lane_of[a] == li) h->order_h[k++] = sl[a];
        }
        h->gstart[G + lanes] = k;
        free(sl);
        free(lane_of);
        h->nlanes = G + lanes;
    } else if (G > 1 && h->nstrag > 0) {  // no queue to spare: deal the stragglers out over the regular groups
        int *slow = (int *)malloc(sizeof(int) * h->nstrag), ns = 0, dreg = 0;
        for (int d = 0; d < nd; d++)
            if (h->strag_h[d]) slow[ns++] = d;
        const int nr = nd - ns;
        int si = 0, ri = 0;
        h->gstart[0] = 0;
        for (int gi = 0; gi < G; gi++) {
            const int rend = (int)((long long)nr * (gi + 1) / G), send = (int)((long long)ns * (gi + 1) / G);
            for (; ri < rend; ri++) {
                while (h->strag_h[dreg]) dreg++;
                h->order_h[k++] = dreg++;
            }
            for (; si < send; si++) h->order_h[k++] = slow[si];
            h->gstart[gi + 1] = k;
        }
        free(slow);
        h->nlanes = G;
    } else {
        // (measured and removed in round 4: draws whose streams k_fixup regenerated in the last solve grouped together -- C2 x 4096 243 ms
        //  against 230: two groups that regenerate in every period finish last, regenerations spread over all groups delay all alike)
        for (int d = 0; d < nd; d++) h->order_h[k++] = d;
        for (int gi = 0; gi <= G; gi++) h->gstart[gi] = (int)((long long)nd * gi / G);
        h->nlanes = G;
    }
    int rc = ensure_group_streams(h, h->nlanes);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync((void *)h->b.order, h->order_h, sizeof(int) * nd, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));  // (order_h is reused by the next rebuild)
    return 0;
}

extern "C" int egdst_set_groups(egdst_handle *h, int ngroups)
{
    if (!h || ngroups < 1) return set_err(EGDST_E_ARG, "egdst_set_groups: bad arguments");
    if (ngroups > EGDST_MAX_GROUPS) ngroups = EGDST_MAX_GROUPS;
    if (ngroups > h->b.g.ndraw) ngroups = h->b.g.ndraw;
    HIPCHK(hipStreamSynchronize(h->stream));
    h->ngroups = ngroups;
    h->auto_groups = 0;  // (the caller's choice stands)
    memset(h->strag_h, 0, h->b.g.ndraw);
    h->nstrag = 0;
    return build_schedule(h);
}

extern "C" int egdst_get_work(egdst_handle *h, unsigned *out)
{
    if (!h || !out) return set_err(EGDST_E_ARG, "egdst_get_work: bad arguments");
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(out, h->b.work, sizeof(unsigned) * h->b.g.ndraw, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int egdst_get_regenerations(egdst_handle *h, unsigned *out)
{
    if (!h || !out) return set_err(EGDST_E_ARG, "egdst_get_regenerations: bad arguments");
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(out, h->b.nregen, sizeof(unsigned) * h->b.g.ndraw, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int egdst_get_schedule(egdst_handle *h, int *groups, int *lanes, int *stragglers)
{
    if (!h) return set_err(EGDST_E_ARG, "egdst_get_schedule: null handle");
    if (groups) *groups = h->ngroups;
    if (lanes) *lanes = h->nlanes - h->ngroups;
    if (stragglers) *stragglers = h->nstrag;
    return 0;
}

extern "C" int egdst_set_adaptive(egdst_handle *h, int on)
{
    if (!h) return set_err(EGDST_E_ARG, "egdst_set_adaptive: null handle");
    h->adaptive = on ? 1 : 0;
    if (!on && h->nstrag) {
        memset(h->strag_h, 0, h->b.g.ndraw);
        h->nstrag = 0;
        return build_schedule(h);
    }
    return 0;
}

extern "C" int egdst_geometry(egdst_handle *h, int *rows_cap, int *table_stride)
{
    if (!h) return set_err(EGDST_E_ARG, "egdst_geometry: null handle");
    if (rows_cap) *rows_cap = h->b.g.Cp;
    if (table_stride) *table_stride = h->b.g.Sp;
    return 0;
}

extern "C" int egdst_destroy(egdst_handle *h)
{
    if (!h) return 0;
    if (h->pool) (void)hipFree(h->pool);
    if (h->b_dev) (void)hipFree(h->b_dev);
    if (h->b_host) (void)hipHostFree(h->b_host);
    if (h->b.klog) (void)hipFree(h->b.klog);
    if (h->b.kcnt) (void)hipFree(h->b.kcnt);
    {
        void *simbufs[] = {h->sim_init, h->sim_rs, h->sim_sims, h->sim_means, h->sim_err, h->sim_counts,
                           h->sim_spec, h->sim_tgt, h->sim_W, h->sim_scores, h->sim_band,
                           h->pol_obs, h->pol_perm, h->pol_flag, h->pol_items, h->pol_term,
                           h->pan_obs, h->pan_perm, h->pan_flag, h->pan_items, h->pan_term};
        for (void *p : simbufs)
            if (p) (void)hipFree(p);
    }
    free(h->pan_first);
    if (h->emu_items) {
        for (int i = 0; i < h->emu_nitems; i++) free(h->emu_items[i]);
        free(h->emu_items);
    }
    if (h->ev) {
        for (int i = 0; i < h->nev; i++)
            if (h->ev[i]) (void)hipEventDestroy(h->ev[i]);
        free(h->ev);
    }
    free(h->imported);
    free(h->order_h);
    free(h->work_h);
    free(h->strag_h);
    for (int g = 0; g < EGDST_MAX_GROUPS; g++) {
        if (h->gstream[g]) (void)hipStreamDestroy(h->gstream[g]);
        if (h->join_ev[g]) (void)hipEventDestroy(h->join_ev[g]);
    }
    if (h->fork_ev) (void)hipEventDestroy(h->fork_ev);
    if (h->own_stream) (void)hipStreamDestroy(h->stream);
    free(h);
    return 0;
}

extern "C" int egdst_set_params(egdst_handle *h, const double *params, int ndraw)
{
    if (!h || ndraw != h->b.g.ndraw || (!params && MS_NPARAM)) return set_err(EGDST_E_ARG, "egdst_set_params: bad arguments");
    if (MS_NPARAM) {
        HIPCHK(hipMemcpyAsync((void *)h->b.par, params, sizeof(double) * (size_t)ndraw * MS_NPARAM, hipMemcpyHostToDevice,
                              h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    h->params_set = 1;
    return 0;
}

extern "C" int egdst_set_params_dev(egdst_handle *h, const double *params_dev, int ndraw)
{
    if (!h || ndraw != h->b.g.ndraw || (!params_dev && MS_NPARAM)) return set_err(EGDST_E_ARG, "egdst_set_params_dev: bad arguments");
    if (MS_NPARAM)
        HIPCHK(hipMemcpyAsync((void *)h->b.par, params_dev, sizeof(double) * (size_t)ndraw * MS_NPARAM,
                              hipMemcpyDeviceToDevice, h->stream));
    h->params_set = 1;
    return 0;
}

// The device copy of the Batch that launches outside a solve read (simulator, accessor, checksums, objective): the handle's
// current pointers, identity schedule range.  Enqueued on the handle's stream ahead of the kernel that reads it.
// The slot is uploaded when it is first needed and again whenever the handle's Batch has changed (egdst_set_dbgout; `call_slot_ok`):
// a launch outside a solve -- egdst_objective_dev in an estimation loop, the simulator -- then costs no host synchronisation and
// follows the solve it reads on the handle's stream.
static int batch_for_call(egdst_handle *h, const Batch **out)
{
    if (!h->call_slot_ok) {
        Batch *slot = h->b_host + EGDST_MAX_GROUPS;
        HIPCHK(hipStreamSynchronize(h->stream));  // (the staging entry may still be the source of an earlier upload)
        *slot = h->b;
        slot->draw0 = 0;
        slot->gdraws = slot->g.ndraw;
        slot->sorted_valid = 0;
        HIPCHK(hipMemcpyAsync(h->b_dev + EGDST_MAX_GROUPS, slot, sizeof(Batch), hipMemcpyHostToDevice, h->stream));
        h->call_slot_ok = 1;
    }
    *out = h->b_dev + EGDST_MAX_GROUPS;
    return 0;
}

// The ticket of a list-driven launch (eg_take_ticket): which = 0 k_fixup, 1 k_tp_tail.
static int *eg_ticket(const Batch &b, int which, int gi, int it) { return b.tickets + ((size_t)which * EGDST_MAX_GROUPS + gi) * b.g.nt + it; }

// One group's launches of one period: its stream, its device copy of the Batch and its range of the schedule.
struct GroupStep {
    egdst_handle *h;
    int gi, it;
    hipStream_t gs;
    const Batch *bg;
    int draw0, gdraws;
};

// profiling: class k in {0 probe/terminal, 1 the grid kernel, 2 k_envelope, 3 regeneration (k_fixup_scan + k_fixup), and the
// kernels of the envelope step's throughput path: 4 k_tp_prep, 5 / 6 k_tp_sort stage 0 / 1, 7 / 8 k_tp_walk stage 0 / 1; its tail
// launch, k_tp_tail, is class 2};
// events on the stream the kernels are launched on, [groups][EG_NPROF][nt][before, end]
// (events are created when first recorded: a handle uses a fraction of the groups x classes x periods x 2 slots, and the
//  runtime's pool of timed events is finite -- 46 080 of them at once failed with "invalid resource handle")
static void eg_rec(const GroupStep &s, int k, int which)
{
    if (!s.h->profile) return;
    hipEvent_t &e = s.h->ev[(((size_t)s.gi * EG_NPROF + k) * s.h->b.g.nt + s.it) * 2 + which];
    if (!e) (void)hipEventCreate(&e);
    if (e) (void)hipEventRecord(e, s.gs);
}
static void eg_before(const GroupStep &s, int k) { eg_rec(s, k, 0); }
static void eg_end(const GroupStep &s, int k) { eg_rec(s, k, 1); }
// EGDST_DEBUG_SYNC: wait for the launches so far and name them with the error they left
static void eg_after(const GroupStep &s, const char *name)
{
    if (!s.h->opt.debug_sync) return;
    hipError_t e = hipStreamSynchronize(s.gs);
    fprintf(stderr, "[egdst] %s it=%d -> %s\n", name, s.it, hipGetErrorString(e));
    fflush(stderr);
}

// The grid kernel of one group and period.
static void enqueue_grid(const GroupStep &s, int combos)
{
    const LaunchPlan &p = s.h->plan;
    const Geom &g = s.h->b.g;
    const dim3 grid((g.ngridm - 1 + GRID_BS - 1) / GRID_BS, combos);
    if (p.grid_wide)
        hipLaunchKernelGGL(k_grid_wide, dim3(((g.ngridm - 1) * EG_GW + EG_GRIDW_BS - 1) / EG_GRIDW_BS, combos), dim3(EG_GRIDW_BS), 0,
                           s.gs, s.bg, s.it);
    else if (p.grid_lrows > 0 && p.grid_cv)
        hipLaunchKernelGGL(k_grid_lds_cv, grid, dim3(GRID_BS), 3 * sizeof(double) * (size_t)p.grid_lrows, s.gs, s.bg, s.it, p.grid_lrows);
    else if (p.grid_lrows > 0)
        hipLaunchKernelGGL(k_grid_lds, grid, dim3(GRID_BS), sizeof(double) * (size_t)p.grid_lrows, s.gs, s.bg, s.it, p.grid_lrows);
    else
        hipLaunchKernelGGL(k_grid, grid, dim3(GRID_BS), 0, s.gs, s.bg, s.it);
    // (Measured slower and removed: several asset points per lane, k_grid_lds_n -- C2 x 4096 194.4 ms against 184.8 with a
    //  lane per point, C4 x 32 52.6 against 51.5, C5 x 128 3.72 s either way: 133 VGPRs, three waves per SIMD instead of six to eight.)
}

// The envelope step of one group and period (terminal: the last period).  env_tp / env_parts: the plan's choices, off while
// the kink log is on.  Profiling class 2, or on the throughput path its kernels one by one.
static void enqueue_envelope(const GroupStep &s, int terminal, bool env_tp, bool env_parts)
{
    egdst_handle *h = s.h;
    const LaunchPlan &p = h->plan;
    const Batch &b = h->b;
    const int it = s.it;
    const unsigned nc = (unsigned)(s.gdraws * MS_NST);  // cells of the group
#if MS_ND == 1
    (void)env_tp, (void)env_parts;
    eg_before(s, 2);
    if (p.e1_on) {
        const int e1_nb = (int)EG_E1_NB(b.g.ngridm);
        hipLaunchKernelGGL(k_env1, dim3(e1_nb, nc), dim3(E1_BS), 0, s.gs, s.bg, it, terminal, b.e1tiles, b.e1done, e1_nb, (unsigned)(it + 1),
                           p.e1_defer_all);
        hipLaunchKernelGGL(k_envelope, dim3(nc), dim3(ENV_MAXBS), h->lds_bytes, s.gs, s.bg, it, terminal, h->lcap, 1, 0, (const int *)nullptr,
                           (const int *)nullptr, (int *)nullptr);
    } else
        hipLaunchKernelGGL(k_envelope, dim3(nc), dim3(ENV_MAXBS), h->lds_bytes, s.gs, s.bg, it, terminal, h->lcap, 2, 0, (const int *)nullptr,
                           (const int *)nullptr, (int *)nullptr);
    eg_end(s, 2);
#else
    if (env_tp && !terminal) {
        int *tcnt = b.tpn + (size_t)s.gi * b.g.nt + it, *tlist = b.tplist + (size_t)s.draw0 * MS_NST;
        int *bigc = b.tpbign + (size_t)s.gi * b.g.nt + it, *bigl = b.tpbiglist + (size_t)s.draw0 * MS_NST;
        int *tail_tk = eg_ticket(b, 1, s.gi, it);
        eg_before(s, 4);
        hipLaunchKernelGGL(k_tp_prep, dim3(nc * MS_ND), dim3(TP_BS), 0, s.gs, s.bg, it);
        eg_end(s, 4);
        eg_before(s, 5);
        hipLaunchKernelGGL(k_tp_sort, dim3(nc * MS_ND), dim3(TP_SORT_BS), tp_sort_lds(p.tp_scap0), s.gs, s.bg, it, 0, p.tp_scap0, p.tp_lkcap0, 0,
                           (int *)nullptr, (int *)nullptr);
        eg_end(s, 5);
        eg_before(s, 7);
        hipLaunchKernelGGL(k_tp_walk, dim3(nc * MS_ND), dim3(p.tp_walk_bs0), (size_t)EG_TP_WALK_LDS_PER_POINT * p.tp_lkcap0, s.gs, s.bg, it, 0,
                           tlist, tcnt, p.tp_lkcap0);
        eg_end(s, 7);
        eg_before(s, 6);
        hipLaunchKernelGGL(k_tp_sort, dim3(nc), dim3(TP_SORT_BS), tp_sort_lds(p.tp_scap1), s.gs, s.bg, it, 1, p.tp_scap1, p.tp_lkcap,
                           p.tp_big ? p.tp_bigcap : 0, p.tp_big ? bigl : (int *)nullptr, p.tp_big ? bigc : (int *)nullptr);
        eg_end(s, 6);
        eg_before(s, 8);
        hipLaunchKernelGGL(k_tp_walk, dim3(nc), dim3(TP_WALK_BS), (size_t)EG_TP_WALK_LDS_PER_POINT * p.tp_lkcap, s.gs, s.bg, it, 1, tlist, tcnt,
                           p.tp_lkcap);
        eg_end(s, 8);
        eg_before(s, 2);
        // The tail of the period, one launch: the cells stage 1 left over (tlist, final after k_tp_walk) and its second tier (bigl,
        // final after k_tp_sort) behind one ticket, the slow leftover cells first; a second-tier cell that gives up is done in place.
        // Workgroups: the larger of what the two launches it replaces had (a workgroup holds most of a CU's LDS, so at most one per
        // CU either way).  A 1365-draw group: 256 whichever way; 16 groups of 256 draws: 64, measured against their sum, 96 -- ahead
        // in every pair of runs, by less than the runs' range (profiles/r08_tp_tail_C2_ndraw4096.txt).
        {
            unsigned ng = eg_sparse_grid(nc, nc, p.tp_rest_wg, p.tp_rest_wg_max);
            const unsigned ngb = p.tp_big ? eg_sparse_grid(nc, nc, p.tp_big_wg, p.tp_big_wg_max) : 0u;
            if (ngb > ng) ng = ngb;
            hipLaunchKernelGGL(k_tp_tail, dim3(ng), dim3(ENV_MAXBS), h->tail_lds, s.gs, s.bg, it, h->lcap, (const int *)tlist, (const int *)tcnt,
                               p.tp_bigcap, p.tp_big ? (const int *)bigl : (const int *)nullptr, p.tp_big ? (const int *)bigc : (const int *)nullptr,
                               tail_tk, (int)h->tail_soff, terminal, 1, 0);
        }
        eg_end(s, 2);
        return;
    }
    eg_before(s, 2);
    if (env_parts) {
        hipLaunchKernelGGL(k_envelope, dim3(nc * MS_ND), dim3(ENV_MAXBS), h->lds_bytes, s.gs, s.bg, it, terminal, h->lcap, 2, 1,
                           (const int *)nullptr, (const int *)nullptr, (int *)nullptr);
        hipLaunchKernelGGL(k_envelope, dim3(nc), dim3(ENV_MAXBS), h->lds_bytes, s.gs, s.bg, it, terminal, h->lcap, 2, 2, (const int *)nullptr,
                           (const int *)nullptr, (int *)nullptr);
    } else
        hipLaunchKernelGGL(k_envelope, dim3(nc), dim3(ENV_MAXBS), h->lds_bytes, s.gs, s.bg, it, terminal, h->lcap, 2, 0, (const int *)nullptr,
                           (const int *)nullptr, (int *)nullptr);
    eg_end(s, 2);
    // (Measured and removed in round 4: a SLOW LANE per group -- the cells whose guess streams k_fixup has to regenerate, 3 % of the
    //  cells of a C2 a0 = -5 period and 57 of the 172 ms of every group's chain (the regeneration itself, and the secondary envelope of a
    //  re-based stream: a dozen nearly coincident pieces, the slowest of a launch's 270 walks at 0.4 ms against a mean of 42 us), taken
    //  out of the period's launches and done by list-driven launches on a second stream of the group, the two meeting only before the
    //  period's last kernel.  Bit-exact, and 348 ms per solve against 168 with 16 groups, 224 with 10, 237 with 8: two cross-stream event
    //  dependencies per group and period (1 900 per solve) cost far more on this runtime than the overlap returns -- the same finding as
    //  round 3's side stream for k_fixup alone.)
#endif
}

// The attached panel's observations of one period for one group's draws (egdst_attach_panel): behind the period's envelope step
// on the group's own chain, while the period's table is live.  Nothing without a panel, nothing for a period without
// observations; not bracketed by the profile's events (its classes are the solve's).
// (On the chain deliberately: both side-stream experiments recorded below and in enqueue_envelope lost to the cost of cross-stream events.)
static void enqueue_panel(const GroupStep &s)
{
    egdst_handle *h = s.h;
    if (!h->pan_nobs) return;
    const int i0 = h->pan_first[s.it], nitems = h->pan_first[s.it + 1] - i0;
    if (nitems <= 0) return;
    PanelArgs a;
    a.it = s.it, a.slot = (h->b.g.nslots == 2) ? (s.it & 1) : s.it;
    a.nobs = h->pan_nobs, a.resid = h->pan_resid;
    a.obs = h->pan_obs, a.perm = h->pan_perm, a.items = h->pan_items + i0;
    a.term = h->pan_term, a.flag = h->pan_flag;
    for (int l0 = 0; l0 < s.gdraws; l0 += 65535) {   // (the grid's second dimension)
        const int nd = s.gdraws - l0 < 65535 ? s.gdraws - l0 : 65535;
        a.lane0 = l0;
        hipLaunchKernelGGL(k_policy_period, dim3((unsigned)nitems, (unsigned)nd), dim3(POL_BS), 0, s.gs, s.bg, a);
    }
    eg_after(s, "k_policy_period");
}

// Enqueues a solve on the handle's stream: the memsets, the fork to the group streams, every period's kernels per group (the
// plan of the handle), the join.  (Measured and removed: capturing this sequence once into a hipGraph and replaying
// it -- 19.4 ms against 19.6 ms for a single C2 solve and nothing for batches; the launches are already asynchronous.)
static int enqueue_solve(egdst_handle *h)
{
    Batch &b = h->b;
    const Geom &g = b.g;
    const LaunchPlan &p = h->plan;
    hipStream_t s = h->stream;
    HIPCHK(hipMemsetAsync(b.status, 0, sizeof(int) * g.ndraw, s));
    HIPCHK(hipMemsetAsync(b.where, 0, sizeof(int) * 2 * g.ndraw, s));
    HIPCHK(hipMemsetAsync(b.evals, 0, sizeof(unsigned long long) * g.ndraw, s));
    HIPCHK(hipMemsetAsync(b.credited, 0, sizeof(unsigned long long) * g.ndraw, s));
    HIPCHK(hipMemsetAsync(b.segstat, 0, sizeof(unsigned) * 2 * g.ndraw, s));
    HIPCHK(hipMemsetAsync(b.sortstat, 0, sizeof(unsigned) * 4 * g.ndraw, s));
    EG_STAMP_DECL(HIPCHK(hipMemsetAsync(b.stamps, 0, sizeof(unsigned long long) * EG_NSTAMP * g.ndraw, s));)
    HIPCHK(hipMemsetAsync(b.algbytes, 0, sizeof(unsigned long long) * g.ndraw, s));
    HIPCHK(hipMemsetAsync(b.tlen, 0, sizeof(int) * (size_t)g.nslots * g.ndraw * MS_NST, s));
    HIPCHK(hipMemsetAsync(b.tthlen, 0, sizeof(int) * (size_t)g.nslots * g.ndraw * MS_NST, s));
    const int G = (h->opt.debug_sync || h->opt.debug_poison) ? 1 : h->nlanes;
    HIPCHK(hipMemsetAsync(b.work, 0, sizeof(unsigned) * g.ndraw, s));
    HIPCHK(hipMemsetAsync(b.nregen, 0, sizeof(unsigned) * g.ndraw, s));
    if (b.kcnt) HIPCHK(hipMemsetAsync(b.kcnt, 0, sizeof(int) * (size_t)g.nt * g.ndraw * MS_NST, s));
    HIPCHK(hipMemsetAsync(b.fixn, 0, sizeof(int) * EGDST_MAX_GROUPS * g.nt, s));
    HIPCHK(hipMemsetAsync(b.tpn, 0, sizeof(int) * EGDST_MAX_GROUPS * g.nt, s));
    HIPCHK(hipMemsetAsync(b.tpbign, 0, sizeof(int) * EGDST_MAX_GROUPS * g.nt, s));
    HIPCHK(hipMemsetAsync(b.tickets, 0, sizeof(int) * 2 * EGDST_MAX_GROUPS * g.nt, s));
    HIPCHK(hipMemsetAsync(b.tpstat, 0, sizeof(unsigned) * 2 * g.ndraw, s));
    HIPCHK(hipMemsetAsync(b.tpinplace, 0, sizeof(unsigned) * g.ndraw, s));
#if MS_ND == 1
    // k_env1: descriptors carry the period as their tag, valid within one solve; the counters count on from zero
    HIPCHK(hipMemsetAsync(b.e1tiles, 0, sizeof(Env1Tile) * (size_t)g.ndraw * MS_NST * EG_E1_NB(g.ngridm), s));
    HIPCHK(hipMemsetAsync(b.e1done, 0, sizeof(unsigned) * (size_t)g.ndraw * MS_NST, s));
#endif
    h->solve_seq++;
    {   // the Batch every group's kernels read (constant address space), one copy per group with its schedule range
        // The staging entries are pinned, and the upload of an earlier solve that is still queued reads them when it runs:
        // solves may be enqueued back to back, so every field is stored once with its final value.  Between two such
        // solves only sorted_valid differs (the schedule changes in egdst_sync alone); a queued solve that picks up a
        // later solve's stamp uses it in all of its kernels, and a stamp left by an earlier solve reads as "out of
        // order", the general search.
        for (int gi = 0; gi < G; gi++) {
            Batch e = b;
            e.draw0 = (G > 1) ? h->gstart[gi] : 0;
            e.gdraws = ((G > 1) ? h->gstart[gi + 1] : g.ndraw) - e.draw0;
            e.sorted_valid = p.sortcheck ? (int)((h->solve_seq & 0x3ffffu) << 12) + 1 : 0;
            h->b_host[gi] = e;
        }
        HIPCHK(hipMemcpyAsync(h->b_dev, h->b_host, sizeof(Batch) * G, hipMemcpyHostToDevice, s));
    }
    if (G > 1) {  // fork: groups 1 .. start after everything enqueued on the handle's stream so far; group 0 follows on that stream itself
        HIPCHK(hipEventRecord(h->fork_ev, s));
        for (int gi = 1; gi < G; gi++) HIPCHK(hipStreamWaitEvent(h->gstream[gi], h->fork_ev, 0));
    }
    // the kink log (egdst_set_dbgout, which may be called after create) orders its rows per cell: one workgroup per cell
    const bool env_tp = p.env_tp && !b.klog, env_parts = p.env_parts && !b.klog;
    // (Measured and not kept, r03: k_fixup on a side stream per group -- k_fixup_scan leaving the cells of a draw with a stream to
    //  regenerate to k_envelope's list pass, which then waits for the side stream -- so that the half millisecond of a
    //  regeneration is off the group's chain of dependent launches.  Bit-exact, and slower: 190-210 ms against 167 for C2 x 4096
    //  with 10-16 side streams on 24 hardware queues; the regeneration then took 1.1-1.7 ms from scan to done instead of 0.5.)
    for (int it = g.nt - 1; it >= 0; it--) {
        if (h->opt.debug_poison) HIPCHK(hipMemsetAsync(h->scratch_lo, 0xAB, (size_t)(h->scratch_hi - h->scratch_lo), s));
        for (int gi = 0; gi < G; gi++) {
            const int draw0 = (G > 1) ? h->gstart[gi] : 0;
            const int gdraws = ((G > 1) ? h->gstart[gi + 1] : g.ndraw) - draw0;
            if (gdraws <= 0) continue;
            const GroupStep st = {h, gi, it, gi ? h->gstream[gi] : s, h->b_dev + gi, draw0, gdraws};  // (b_dev: uploaded above)
            const int combos = gdraws * MS_NST * MS_ND;
            if (it == g.nt - 1) {
                eg_before(st, 0);
                hipLaunchKernelGGL(k_terminal, dim3((g.ngridm + GRID_BS - 1) / GRID_BS, combos), dim3(GRID_BS), 0, st.gs, st.bg, it);
                eg_end(st, 0);
                eg_after(st, "k_terminal");
                enqueue_envelope(st, 1, env_tp, env_parts);
                eg_after(st, "k_envelope(T)");
                enqueue_panel(st);
                continue;
            }
            if (p.sortcheck)
                hipLaunchKernelGGL(k_sortcheck, dim3((unsigned)((g.Sp + SORTCHK_ROWS - 1) / SORTCHK_ROWS), gdraws * MS_NST), dim3(GRID_BS), 0,
                                   st.gs, st.bg, it);
            eg_before(st, 0);
            hipLaunchKernelGGL(k_probe, dim3(combos), dim3(WAVE), 0, st.gs, st.bg, it);
            eg_end(st, 0);
            eg_after(st, "k_probe");
            eg_before(st, 1);
            enqueue_grid(st, combos);
            eg_end(st, 1);
            eg_before(st, 3);
            int *cnt = b.fixn + (size_t)gi * g.nt + it, *list = b.fixlist + (size_t)draw0 * MS_NST * MS_ND;
            hipLaunchKernelGGL(k_fixup_scan, dim3(combos), dim3(WAVE), 0, st.gs, st.bg, it, cnt, list);
            hipLaunchKernelGGL(k_fixup, dim3(eg_sparse_grid((unsigned)(gdraws * MS_NST), (unsigned)combos, p.fix_wg, p.fix_wg_max)), dim3(FIX_BS), 0,
                               st.gs, st.bg, it, (const int *)cnt, (const int *)list, eg_ticket(b, 0, gi, it));
            eg_end(st, 3);
            eg_after(st, "k_grid+k_fixup");
            enqueue_envelope(st, 0, env_tp, env_parts);
            eg_after(st, "k_envelope");
            enqueue_panel(st);
        }
    }
    if (G > 1)  // join: the handle's stream, group 0's launches on it, continues when every other group is done
        for (int gi = 1; gi < G; gi++) {
            HIPCHK(hipEventRecord(h->join_ev[gi], h->gstream[gi]));
            HIPCHK(hipStreamWaitEvent(s, h->join_ev[gi], 0));
        }
    HIPCHK(hipGetLastError());
    h->solved = 1;
    h->pan_fit = h->pan_nobs > 0;
    if (h->imported) memset(h->imported, 0, (size_t)g.ndraw);
    return 0;
}

extern "C" int egdst_solve_async(egdst_handle *h)
{
    if (!h) return set_err(EGDST_E_ARG, "null handle");
    if (!h->params_set && MS_NPARAM) return set_err(EGDST_E_ARG, "egdst_solve: parameters not set");
    return enqueue_solve(h);
}

extern "C" int egdst_sync(egdst_handle *h)
{
    if (!h) return set_err(EGDST_E_ARG, "null handle");
    HIPCHK(hipStreamSynchronize(h->stream));
    int *st = (int *)malloc(sizeof(int) * h->b.g.ndraw);
    hipError_t e = hipMemcpy(st, h->b.status, sizeof(int) * h->b.g.ndraw, hipMemcpyDeviceToHost);
    int rc = 0;
    if (e != hipSuccess)
        rc = set_err(EGDST_E_HIP, "status copy failed: %s", hipGetErrorString(e));
    else
        for (int i = 0; i < h->b.g.ndraw && !rc; i++)
            if (st[i]) rc = set_err(st[i], "draw %d: %s", i, egdst_strerror(st[i]));
    free(st);
    int regrouped = 0;
    const long cells = (long)h->b.g.ndraw * MS_NST;
    if (h->adaptive && h->auto_groups && e == hipSuccess && h->b.g.nt > 1 &&
        eg_default_groups(h->hwq, cells) > eg_chain_queues(h->hwq)) {  // (only then can the history change the count)
        unsigned *nr = (unsigned *)malloc(sizeof(unsigned) * h->b.g.ndraw);
        if (hipMemcpy(nr, h->b.nregen, sizeof(unsigned) * h->b.g.ndraw, hipMemcpyDeviceToHost) == hipSuccess) {
            double sum = 0;
            for (int i = 0; i < h->b.g.ndraw; i++) sum += nr[i];
            const int want = eg_history_groups(h->hwq, cells, h->plan.env_tp, sum / ((double)cells * MS_ND * (h->b.g.nt - 1)));
            if (want != h->ngroups) h->ngroups = want, regrouped = 1;
        }
        free(nr);
    }
    if (h->adaptive && h->ngroups > 1 && e == hipSuccess) {
        // Stragglers: draws whose guess streams re-based more than EG_STRAGGLER_CALLS times in this solve (a normal
        // stream re-bases a few dozen times, a degenerate one ~9000 times in one period, strictly sequentially).
        // Parameters move slowly from one solve of an estimation loop to the next, so the next solve gives these
        // draws lanes of their own, where they hold up each other instead of a whole group.
        if (hipMemcpy(h->work_h, h->b.work, sizeof(unsigned) * h->b.g.ndraw, hipMemcpyDeviceToHost) == hipSuccess) {
            int changed = 0, ns = 0;
            for (int i = 0; i < h->b.g.ndraw; i++) {
                const unsigned char sl = (h->work_h[i] > EG_STRAGGLER_CALLS || (EG_STRAGGLER_EVERY && i % (EG_STRAGGLER_EVERY ? EG_STRAGGLER_EVERY : 1) == 1)) ? 1 : 0;
                if (sl != h->strag_h[i]) changed = 1;
                h->strag_h[i] = sl;
                ns += sl;
            }
            h->nstrag = ns;
            if (changed || regrouped) {
                const int rc2 = build_schedule(h);
                if (rc2 && !rc) rc = rc2;
            }
            regrouped = 0;
        }
    }
    if (regrouped) {
        const int rc2 = build_schedule(h);
        if (rc2 && !rc) rc = rc2;
    }
    return rc;
}

extern "C" int egdst_solve(egdst_handle *h)
{
    int rc = egdst_solve_async(h);
    if (rc) return rc;
    return egdst_sync(h);
}

extern "C" int egdst_get_status(egdst_handle *h, int *status, int *where)
{
    if (!h || !status) return set_err(EGDST_E_ARG, "egdst_get_status: bad arguments");
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(status, h->b.status, sizeof(int) * h->b.g.ndraw, hipMemcpyDeviceToHost));
    if (where) HIPCHK(hipMemcpy(where, h->b.where, sizeof(int) * 2 * h->b.g.ndraw, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int egdst_get_evals(egdst_handle *h, long long *total, long long *per_draw)
{
    if (!h || !total) return set_err(EGDST_E_ARG, "egdst_get_evals: bad arguments");
    const int n = h->b.g.ndraw;
    HIPCHK(hipStreamSynchronize(h->stream));
    unsigned long long *tmp = (unsigned long long *)malloc(sizeof(unsigned long long) * n);
    hipError_t e = hipMemcpy(tmp, h->b.evals, sizeof(unsigned long long) * n, hipMemcpyDeviceToHost);
    if (e != hipSuccess) {
        free(tmp);
        return set_err(EGDST_E_HIP, "evals copy failed: %s", hipGetErrorString(e));
    }
    long long t = 0;
    for (int i = 0; i < n; i++) {
        t += (long long)tmp[i];
        if (per_draw) per_draw[i] = (long long)tmp[i];
    }
    *total = t;
    free(tmp);
    return 0;
}

extern "C" int egdst_get_evals_credited(egdst_handle *h, long long *total, long long *per_draw)
{
    if (!h || !total) return set_err(EGDST_E_ARG, "egdst_get_evals_credited: bad arguments");
    const int n = h->b.g.ndraw;
    HIPCHK(hipStreamSynchronize(h->stream));
    unsigned long long *tmp = (unsigned long long *)malloc(sizeof(unsigned long long) * n);
    hipError_t e = hipMemcpy(tmp, h->b.credited, sizeof(unsigned long long) * n, hipMemcpyDeviceToHost);
    long long t = 0;
    if (e == hipSuccess)
        for (int i = 0; i < n; i++) {
            t += (long long)tmp[i];
            if (per_draw) per_draw[i] = (long long)tmp[i];
        }
    free(tmp);
    if (e != hipSuccess) return set_err(EGDST_E_HIP, "credited copy failed: %s", hipGetErrorString(e));
    *total = t;
    return 0;
}

static int check_cell(egdst_handle *h, int draw, int it, int ist)
{
    if (!h) return set_err(EGDST_E_ARG, "null handle");
    if (!h->keep_history) return set_err(EGDST_E_ARG, "cell export needs keep_history=1");
    if (!h->solved) return set_err(EGDST_E_NOT_SOLVED, "%s", egdst_strerror(EGDST_E_NOT_SOLVED));
    const Geom &g = h->b.g;
    if (draw < 0 || draw >= g.ndraw || it < 0 || it >= g.nt || ist < 0 || ist >= MS_NST)
        return set_err(EGDST_E_ARG, "cell index out of range");
    return 0;
}

extern "C" int egdst_cell_dims(egdst_handle *h, int draw, int it, int ist, int *len, int *thlen)
{
    int rc = check_cell(h, draw, it, ist);
    if (rc) return rc;
    const Geom &g = h->b.g;
    const size_t k = ((size_t)it * g.ndraw + draw) * MS_NST + ist;
    HIPCHK(hipStreamSynchronize(h->stream));
    if (len) HIPCHK(hipMemcpy(len, h->b.tlen + k, sizeof(int), hipMemcpyDeviceToHost));
    if (thlen) HIPCHK(hipMemcpy(thlen, h->b.tthlen + k, sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int egdst_get_cell_M(egdst_handle *h, int draw, int it, int ist, double *out)
{
    int len = 0, rc = egdst_cell_dims(h, draw, it, ist, &len, nullptr);
    if (rc) return rc;
    if (len <= 0) return 0;
    const Geom &g = h->b.g;
    const size_t k = ((size_t)it * g.ndraw + draw) * MS_NST + ist;
    HIPCHK(hipMemcpy(out, h->b.tM + k * g.Sp, sizeof(double) * len, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out + len, h->b.tC + k * g.Sp, sizeof(double) * len, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out + 3 * (size_t)len, h->b.tV + k * g.Sp, sizeof(double) * len, hipMemcpyDeviceToHost));
    for (int i = 0; i < len; i++) out[2 * (size_t)len + i] = out[i] - out[len + i];  // A = M - C (:937)
    return 0;
}

extern "C" int egdst_get_cell_D(egdst_handle *h, int draw, int it, int ist, double *out)
{
    int thlen = 0, rc = egdst_cell_dims(h, draw, it, ist, nullptr, &thlen);
    if (rc) return rc;
    if (thlen <= 0) return 0;
    const Geom &g = h->b.g;
    const size_t k = ((size_t)it * g.ndraw + draw) * MS_NST + ist;
    HIPCHK(hipMemcpy(out, h->b.tD + k * g.nthrhmax, sizeof(double) * thlen, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out + thlen, h->b.tTH + k * g.nthrhmax, sizeof(double) * thlen, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int egdst_get_solution(egdst_handle *h, int draw, int *lens, int *thlens, double *M, double *C, double *V,
                                  double *D, double *TH)
{
    int rc = check_cell(h, draw, 0, 0);
    if (rc) return rc;
    const Geom &g = h->b.g;
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int it = 0; it < g.nt; it++) {
        const size_t k = ((size_t)it * g.ndraw + draw) * MS_NST;  // MS_NST consecutive states
        const size_t o = (size_t)it * MS_NST;
        if (lens) HIPCHK(hipMemcpy(lens + o, h->b.tlen + k, sizeof(int) * MS_NST, hipMemcpyDeviceToHost));
        if (thlens) HIPCHK(hipMemcpy(thlens + o, h->b.tthlen + k, sizeof(int) * MS_NST, hipMemcpyDeviceToHost));
        // host arrays keep the logical row stride S; the device rows are Sp apart (Sp == S in exact mode)
        const size_t hp = sizeof(double) * g.S, dp = sizeof(double) * g.Sp;
        if (M) HIPCHK(hipMemcpy2D(M + o * g.S, hp, h->b.tM + k * g.Sp, dp, dp, MS_NST, hipMemcpyDeviceToHost));
        if (C) HIPCHK(hipMemcpy2D(C + o * g.S, hp, h->b.tC + k * g.Sp, dp, dp, MS_NST, hipMemcpyDeviceToHost));
        if (V) HIPCHK(hipMemcpy2D(V + o * g.S, hp, h->b.tV + k * g.Sp, dp, dp, MS_NST, hipMemcpyDeviceToHost));
        if (D) HIPCHK(hipMemcpy(D + o * g.nthrhmax, h->b.tD + k * g.nthrhmax, sizeof(double) * MS_NST * g.nthrhmax, hipMemcpyDeviceToHost));
        if (TH) HIPCHK(hipMemcpy(TH + o * g.nthrhmax, h->b.tTH + k * g.nthrhmax, sizeof(double) * MS_NST * g.nthrhmax, hipMemcpyDeviceToHost));
    }
    return 0;
}

// ---- solution import -------------------------------------------------------------------------------------------------------
// The reference's simulator and accessor gateways do not depend on a solve in the same process: they read the cell arrays
// M and D from the model object on every call (egdst_simulator.c:61-68, egdst_call.c:28-34), and the class is
// ConstructOnLoad (egdstmodel.m:1), so a model saved after solving can be simulated without solving again.  These entry
// points are the inverse of the export calls: a handle that never ran egdst_solve gets its tables from the host.
static int import_check(egdst_handle *h, int draw, int it, int ist, const char *who)
{
    if (!h) return set_err(EGDST_E_ARG, "%s: null handle", who);
    if (!h->keep_history) return set_err(EGDST_E_ARG, "%s needs keep_history=1", who);
    const Geom &g = h->b.g;
    if (draw < 0 || draw >= g.ndraw || it < 0 || it >= g.nt || ist < 0 || ist >= MS_NST)
        return set_err(EGDST_E_ARG, "%s: cell index out of range", who);
    return 0;
}

// rows [len, Sp) of the cell's three columns are zero afterwards (what a freshly created matrix holds past a table's end,
// egdst_solver.c:198-217) and the high-water mark says so
static int import_rows(egdst_handle *h, size_t k, int len, const double *M, const double *C, const double *V)
{
    const Geom &g = h->b.g;
    Batch &b = h->b;
    hipStream_t s = h->stream;
    if (len < 0 || len > g.S) return set_err(EGDST_E_ARG, "solution import: a cell has %d rows, the descriptor allows %d", len, g.S);
    if (len > g.Sp) return set_err(EGDST_E_CAPACITY, "%s", egdst_strerror(EGDST_E_CAPACITY));
    double *cols[3] = {b.tM + k * g.Sp, b.tC + k * g.Sp, b.tV + k * g.Sp};
    const double *src[3] = {M, C, V};
    for (int c = 0; c < 3; c++) {
        if (len > 0) HIPCHK(hipMemcpyAsync(cols[c], src[c], sizeof(double) * len, hipMemcpyHostToDevice, s));
        if (len < g.Sp) HIPCHK(hipMemsetAsync(cols[c] + len, 0, sizeof(double) * (size_t)(g.Sp - len), s));
    }
    const int hw = len > 0 ? len : 0;
    HIPCHK(hipMemcpyAsync(b.tlen + k, &len, sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(b.thw + k, &hw, sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));  // (the sources are the caller's, `len` and `hw` this frame's)
    return 0;
}

static int import_thresholds(egdst_handle *h, size_t k, int thlen, const double *D, const double *TH)
{
    const Geom &g = h->b.g;
    Batch &b = h->b;
    hipStream_t s = h->stream;
    if (thlen < 0 || thlen > g.nthrhmax)
        return set_err(EGDST_E_ARG, "solution import: a cell has %d thresholds, the descriptor allows %d", thlen, g.nthrhmax);
    double *cols[2] = {b.tD + k * g.nthrhmax, b.tTH + k * g.nthrhmax};
    const double *src[2] = {D, TH};
    for (int c = 0; c < 2; c++) {
        if (thlen > 0) HIPCHK(hipMemcpyAsync(cols[c], src[c], sizeof(double) * thlen, hipMemcpyHostToDevice, s));
        if (thlen < g.nthrhmax) HIPCHK(hipMemsetAsync(cols[c] + thlen, 0, sizeof(double) * (size_t)(g.nthrhmax - thlen), s));
    }
    HIPCHK(hipMemcpyAsync(b.tthlen + k, &thlen, sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(b.thhw + k, &thlen, sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

// The first import into a draw since the last solve (or since create) decides what the draw's OTHER cells are: on a handle that was
// never solved every draw first gets status EGDST_E_NOT_SOLVED, so that only draws that did receive cells simulate; and a draw that
// was never solved or whose solve failed has the lengths of all its cells cleared, so that a half-imported draw reads as empty cells
// (the reference's "not yet solved" state of a cell, egdst_call.c:36-40) rather than as a mixture with the failed solve's tables.
static int import_begin(egdst_handle *h, int draw)
{
    const Geom &g = h->b.g;
    Batch &b = h->b;
    hipStream_t s = h->stream;
    if (!h->imported) {
        h->imported = (unsigned char *)calloc((size_t)g.ndraw, 1);
        if (!h->imported) return set_err(EGDST_E_ARG, "solution import: out of host memory");
    }
    h->pan_fit = 0;   // (egdst_fit_dev answers for solves alone: the terms on the handle are not those of an imported table)
    if (h->imported[draw]) return 0;
    int st = EGDST_E_NOT_SOLVED;
    if (!h->solved) {
        int *all = (int *)malloc(sizeof(int) * (size_t)g.ndraw);
        if (!all) return set_err(EGDST_E_ARG, "solution import: out of host memory");
        for (int d = 0; d < g.ndraw; d++) all[d] = EGDST_E_NOT_SOLVED;
        hipError_t e = hipMemcpyAsync(b.status, all, sizeof(int) * g.ndraw, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        free(all);
        HIPCHK(e);
        h->solved = 1;
    } else {
        HIPCHK(hipMemcpyAsync(&st, b.status + draw, sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    if (st != 0) {
        const size_t pitch = sizeof(int) * (size_t)g.ndraw * MS_NST, off = (size_t)draw * MS_NST;
        int *lens[4] = {b.tlen, b.thw, b.tthlen, b.thhw};
        for (int *p : lens) HIPCHK(hipMemset2DAsync(p + off, pitch, 0, sizeof(int) * MS_NST, (size_t)g.nt, s));
    }
    h->imported[draw] = 1;
    return 0;
}

// an imported draw counts as solved without error: the simulator and the accessor skip draws whose status is set
static int import_done(egdst_handle *h, int draw)
{
    HIPCHK(hipMemsetAsync(h->b.status + draw, 0, sizeof(int), h->stream));
    HIPCHK(hipMemsetAsync(h->b.where + 2 * draw, 0, 2 * sizeof(int), h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->solved = 1;
    return 0;
}

extern "C" int egdst_set_cell_M(egdst_handle *h, int draw, int it, int ist, int len, const double *in)
{
    int rc = import_check(h, draw, it, ist, "egdst_set_cell_M");
    if (!rc) rc = import_begin(h, draw);
    if (rc) return rc;
    if (len > 0 && !in) return set_err(EGDST_E_ARG, "egdst_set_cell_M: null matrix");
    const size_t k = ((size_t)it * h->b.g.ndraw + draw) * MS_NST + ist;
    // column-major (len x 4) [M C A V]; A = M - C is derived again on export (saveoutput, egdst_solver.c:937)
    rc = import_rows(h, k, len, in, in + (len > 0 ? len : 0), in + 3 * (size_t)(len > 0 ? len : 0));
    return rc ? rc : import_done(h, draw);
}

extern "C" int egdst_set_cell_D(egdst_handle *h, int draw, int it, int ist, int thlen, const double *in)
{
    int rc = import_check(h, draw, it, ist, "egdst_set_cell_D");
    if (!rc) rc = import_begin(h, draw);
    if (rc) return rc;
    if (thlen > 0 && !in) return set_err(EGDST_E_ARG, "egdst_set_cell_D: null matrix");
    const size_t k = ((size_t)it * h->b.g.ndraw + draw) * MS_NST + ist;
    rc = import_thresholds(h, k, thlen, in, in + (thlen > 0 ? thlen : 0));  // column-major (thlen x 2) [D TH]
    return rc ? rc : import_done(h, draw);
}

extern "C" int egdst_set_solution(egdst_handle *h, int draw, const int *lens, const int *thlens, const double *M, const double *C,
                                  const double *V, const double *D, const double *TH)
{
    int rc = import_check(h, draw, 0, 0, "egdst_set_solution");
    if (!rc) rc = import_begin(h, draw);
    if (rc) return rc;
    if (!lens || !thlens || !M || !C || !V || !D || !TH) return set_err(EGDST_E_ARG, "egdst_set_solution: null array");
    const Geom &g = h->b.g;
    for (int it = 0; it < g.nt && !rc; it++)
        for (int ist = 0; ist < MS_NST && !rc; ist++) {
            const size_t k = ((size_t)it * g.ndraw + draw) * MS_NST + ist, o = (size_t)it * MS_NST + ist;
            rc = import_rows(h, k, lens[o], M + o * g.S, C + o * g.S, V + o * g.S);  // host arrays: logical row stride S
            if (!rc) rc = import_thresholds(h, k, thlens[o], D + o * g.nthrhmax, TH + o * g.nthrhmax);
        }
    return rc ? rc : import_done(h, draw);
}

// Device buffers of the simulator, kept on the handle and grown on demand (nothing is allocated per call once warm).
static int sim_reserve(void **p, size_t *have, size_t want)
{
    if (*have >= want) return 0;
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    *have = 0;
    HIPCHK(hipMalloc(p, want));
    *have = want;
    return 0;
}

static int sim_check(egdst_handle *h, const double *init, int nsim, long long nrand, int rndtype, int have_stream)
{
    if (!init || nsim < 1) return set_err(EGDST_E_ARG, "egdst_simulate: bad arguments");
    const Geom &g = h->b.g;
    if (!have_stream) return 0;
    // randstream length checks of the gateway (egdst_simulator.c:70-75, MINUNITRND 4)
    if (rndtype == 1 && nrand < 4LL * g.nt)
        return set_err(EGDST_E_RAND_SHORT, "Error: randstream is too short even to be re-used for each simulated agent!");
    if (rndtype != 1 && nrand < 4LL * nsim * g.nt) return set_err(EGDST_E_RAND_SHORT, "%s", egdst_strerror(EGDST_E_RAND_SHORT));
    return 0;
}

// Runs k_simulate for draws [draw0, draw0+nd) with one set of agents; the paths stay on the device in h->sim_sims
// ([nd][nout x nt x nsim]).  randstream: host uniforms (uploaded), or rs_dev: device uniforms, or neither: generated from seed.
static int run_simulation(egdst_handle *h, int draw0, int nd, int batch, const double *init, int nsim, const double *randstream,
                          const double *rs_dev, long long nrand, unsigned long long seed, int rndtype)
{
    int rc = check_cell(h, draw0, 0, 0);
    if (rc) return rc;
    if (!h->params_set && MS_NPARAM) return set_err(EGDST_E_ARG, "egdst_simulate: parameters not set");
    rc = sim_check(h, init, nsim, nrand, rndtype, randstream != nullptr || rs_dev != nullptr);
    if (rc) return rc;
    const Geom &g = h->b.g;
    const size_t per_draw = (size_t)EG_NOUT * g.nt * nsim, nsims = per_draw * nd;
    const long long nuse = (rndtype == 1) ? 4LL * g.nt : 4LL * nsim * g.nt;
    rc = sim_reserve((void **)&h->sim_init, &h->sim_init_bytes, sizeof(double) * 2 * nsim);
    if (!rc && randstream) rc = sim_reserve((void **)&h->sim_rs, &h->sim_rs_bytes, sizeof(double) * nuse);
    if (!rc) rc = sim_reserve((void **)&h->sim_sims, &h->sim_sims_bytes, sizeof(double) * nsims);
    if (!rc) rc = sim_reserve((void **)&h->sim_err, &h->sim_err_bytes, sizeof(int));
    if (rc) return rc;
    hipStream_t s = h->stream;
    int herr = 0;
    HIPCHK(hipMemcpyAsync(h->sim_init, init, sizeof(double) * 2 * nsim, hipMemcpyHostToDevice, s));
    if (randstream) HIPCHK(hipMemcpyAsync(h->sim_rs, randstream, sizeof(double) * nuse, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(h->sim_err, 0, sizeof(int), s));
    hipLaunchKernelGGL(k_fill_nan, dim3((unsigned)((nsims + 255) / 256)), dim3(256), 0, s, h->sim_sims, nsims, per_draw, batch ? 0 : 1);
    const Batch *bdev = nullptr;
    rc = batch_for_call(h, &bdev);
    if (rc) return rc;
    SimArgs a;
    a.draw = draw0;
    a.nsim = nsim;
    a.rndtype = rndtype;
    a.nout = EG_NOUT;
    a.batch = batch;
    a.init = h->sim_init;
    a.randstream = randstream ? h->sim_rs : rs_dev;
    a.seed = seed;
    a.sims = h->sim_sims;
    a.err = h->sim_err;
    hipLaunchKernelGGL(k_simulate, dim3((nsim + GRID_BS - 1) / GRID_BS, nd), dim3(GRID_BS), 0, s, bdev, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(&herr, h->sim_err, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (herr) return set_err(herr, "%s", egdst_strerror(herr));
    return 0;
}

extern "C" int egdst_simulate(egdst_handle *h, int draw, const double *init, int nsim, const double *randstream,
                              long long nrand, int rndtype, double *sims)
{
    if (!sims || !randstream) return set_err(EGDST_E_ARG, "egdst_simulate: bad arguments");
    int rc = run_simulation(h, draw, 1, 0, init, nsim, randstream, nullptr, nrand, 0ull, rndtype);
    if (rc) return rc;
    const size_t nsims = (size_t)EG_NOUT * h->b.g.nt * nsim;
    HIPCHK(hipMemcpy(sims, h->sim_sims, sizeof(double) * nsims, hipMemcpyDeviceToHost));
    return 0;
}

// N2 of SURVEY 8(f): simulated moments without moving the paths.  means[col + nout*it] = mean over the agents alive
// in period it of simulated column col, counts[col + nout*it] the number of agents it is taken over; the paths
// ([nout x nt x nsim] doubles) never leave the device.  The summation order is fixed (deterministic results).
extern "C" int egdst_simulate_moments(egdst_handle *h, int draw, const double *init, int nsim, const double *randstream,
                                      long long nrand, int rndtype, double *means, int *counts)
{
    if (!means || !counts || !randstream) return set_err(EGDST_E_ARG, "egdst_simulate_moments: bad arguments");
    int rc = run_simulation(h, draw, 1, 0, init, nsim, randstream, nullptr, nrand, 0ull, rndtype);
    if (rc) return rc;
    const int nt = h->b.g.nt, ncell = EG_NOUT * nt;
    rc = sim_reserve((void **)&h->sim_means, &h->sim_means_bytes, sizeof(double) * ncell);
    if (!rc) rc = sim_reserve((void **)&h->sim_counts, &h->sim_counts_bytes, sizeof(int) * ncell);
    if (rc) return rc;
    hipLaunchKernelGGL(k_moments, dim3(ncell), dim3(MOM_BS), 0, h->stream, (const double *)h->sim_sims, nsim, nt,
                       (const egdst_moment_lag *)nullptr, ncell, h->sim_means, h->sim_counts);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(means, h->sim_means, sizeof(double) * ncell, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(counts, h->sim_counts, sizeof(int) * ncell, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" double egdst_uniform(unsigned long long seed, unsigned long long k) { return eg_uniform(seed, k); }

#ifndef EG_SIM_SLICE_BYTES
#define EG_SIM_SLICE_BYTES (2ull << 30)
#endif
// The estimation step on the device, behind egdst_simulate_batch_moments and egdst_simulate_batch_spec (which check their
// arguments): every draw of the handle is simulated with the same agents and the same uniforms (common random numbers),
// k_moments reduces the paths to nmom moments per draw (k_quantiles those that are quantiles, launched only for a spec that has
// one) and k_moment_objective forms the draw's distance to the target.
// spec == nullptr: the moments are the nmom = EG_NOUT * nt per-period cells and W [nmom] is the diagonal of the weighting;
// otherwise spec [nmom] (host; the device sees the one record type, egdst_moment_lag) and W [nmom x nmom].  Draws [d0, d0+nd) are simulated together as long as their paths fit
// EG_SIM_SLICE_BYTES, and a slice is reduced on the handle's stream before the next one overwrites the paths
// (run_simulation waits for its kernel).  Nothing but the objective and, if asked for, the moments is written for the caller.
// cov_dev (egdst_simulate_batch_spec_cov only; needs spec): every slice also goes through k_moment_scores and k_moment_cov, which
// writes the slice's matrices straight into cov_dev [ndraw][nmom][nmom]; the scores of a slice then count beside its paths
// towards EG_SIM_SLICE_BYTES.  Without cov_dev the slices, the launches and the uploads are those of the step without it.
// With cov_dev and a quantile in the spec (it carries a bandwidth: the door checked) every slice also launches k_quantile_band
// over the span of quantile records, between k_quantiles and k_moment_scores, into h->sim_band [ndraw][nmom], which is reserved
// only then; a spec without one enqueues what it did.
static int estimation_step(egdst_handle *h, const double *init, int nsim, const double *randstream_dev, long long nrand,
                           unsigned long long seed, int rndtype, const egdst_moment_lag *spec, int nmom, const double *target,
                           const double *W, double *means_dev, int *counts_dev, double *obj_dev, double *cov_dev)
{
    const Geom &g = h->b.g;
    const size_t nW = spec ? (size_t)nmom * nmom : (size_t)nmom;
    int rc = sim_reserve((void **)&h->sim_means, &h->sim_means_bytes, sizeof(double) * (size_t)nmom * g.ndraw);
    if (!rc) rc = sim_reserve((void **)&h->sim_counts, &h->sim_counts_bytes, sizeof(int) * (size_t)nmom * g.ndraw);
    if (!rc && spec) rc = sim_reserve((void **)&h->sim_spec, &h->sim_spec_bytes, sizeof(egdst_moment_lag) * (size_t)nmom);
    if (!rc && obj_dev) rc = sim_reserve((void **)&h->sim_tgt, &h->sim_tgt_bytes, sizeof(double) * (size_t)nmom);
    if (!rc && obj_dev) rc = sim_reserve((void **)&h->sim_W, &h->sim_W_bytes, sizeof(double) * nW);
    if (rc) return rc;
    if (spec) HIPCHK(hipMemcpyAsync(h->sim_spec, spec, sizeof(egdst_moment_lag) * (size_t)nmom, hipMemcpyHostToDevice, h->stream));
    if (obj_dev) {
        HIPCHK(hipMemcpyAsync(h->sim_tgt, target, sizeof(double) * (size_t)nmom, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(h->sim_W, W, sizeof(double) * nW, hipMemcpyHostToDevice, h->stream));
    }
    int q_first = 0, q_last = -1;   // the records [q_first, q_last] hold every quantile (kind 3) of the spec: k_quantiles' grid
    for (int j = 0; spec && j < nmom; j++)
        if (spec[j].kind == 3) {
            if (q_last < 0) q_first = j;
            q_last = j;
        }
    const size_t score_draw = cov_dev ? sizeof(double) * (size_t)nsim * cov_padded(nmom) : 0;   // (a draw's scores)
    const size_t per_draw = sizeof(double) * (size_t)EG_NOUT * g.nt * nsim + score_draw;
    int slice = (int)(EG_SIM_SLICE_BYTES / (per_draw ? per_draw : 1));
    if (slice < 1) slice = 1;
    if (slice > g.ndraw) slice = g.ndraw;
    const bool banded = cov_dev && q_last >= q_first;   // (the covariance door takes a quantile only with its bandwidth)
    if (cov_dev) {
        rc = sim_reserve((void **)&h->sim_scores, &h->sim_scores_bytes, score_draw * slice);
        if (!rc && banded) rc = sim_reserve((void **)&h->sim_band, &h->sim_band_bytes, sizeof(double) * (size_t)nmom * g.ndraw);
        if (rc) return rc;
    }
    for (int d0 = 0; d0 < g.ndraw; d0 += slice) {
        const int nd = (g.ndraw - d0 < slice) ? g.ndraw - d0 : slice;
        rc = run_simulation(h, d0, nd, 1, init, nsim, nullptr, randstream_dev, nrand, seed, rndtype);
        if (rc) return rc;
        hipLaunchKernelGGL(k_moments, dim3(nmom, nd), dim3(MOM_BS), 0, h->stream, (const double *)h->sim_sims, nsim, g.nt,
                           spec ? (const egdst_moment_lag *)h->sim_spec : nullptr, nmom, h->sim_means + (size_t)d0 * nmom,
                           h->sim_counts + (size_t)d0 * nmom);
        if (q_last >= q_first)   // the quantile records, which k_moments leaves alone
            hipLaunchKernelGGL(k_quantiles, dim3(q_last - q_first + 1, nd), dim3(QNT_BS), 0, h->stream, (const double *)h->sim_sims,
                               nsim, g.nt, (const egdst_moment_lag *)h->sim_spec, q_first, nmom, h->sim_means + (size_t)d0 * nmom,
                               h->sim_counts + (size_t)d0 * nmom);
        if (banded)   // the sparsities of the banded quantiles, over the same span of records
            hipLaunchKernelGGL(k_quantile_band, dim3(q_last - q_first + 1, nd), dim3(QNT_BS), 0, h->stream, (const double *)h->sim_sims,
                               nsim, g.nt, (const egdst_moment_lag *)h->sim_spec, q_first, nmom, h->sim_band + (size_t)d0 * nmom,
                               (double *)nullptr);
        if (cov_dev) {
            const int ntile = cov_padded(nmom) / COV_T;
            hipLaunchKernelGGL(k_moment_scores, dim3((unsigned)(((size_t)nsim * cov_padded(nmom) + MOM_BS - 1) / MOM_BS), nd), dim3(MOM_BS),
                               0, h->stream, (const double *)h->sim_sims, nsim, g.nt, (const egdst_moment_lag *)h->sim_spec, nmom,
                               (const double *)(h->sim_means + (size_t)d0 * nmom), (const int *)(h->sim_counts + (size_t)d0 * nmom),
                               (const double *)(banded ? h->sim_band + (size_t)d0 * nmom : nullptr), h->sim_scores);
            hipLaunchKernelGGL(k_moment_cov, dim3(ntile * (ntile + 1) / 2, nd), dim3(COV_BS), 0, h->stream,
                               (const double *)h->sim_scores, nsim, nmom, cov_dev + (size_t)d0 * nmom * nmom);
        }
    }
    if (obj_dev)
        hipLaunchKernelGGL(k_moment_objective, dim3(g.ndraw), dim3(MOM_BS), 0, h->stream, (const double *)h->sim_means,
                           (const int *)h->sim_counts, nmom, (const double *)h->sim_tgt, (const double *)h->sim_W, spec ? 0 : 1,
                           obj_dev);
    HIPCHK(hipGetLastError());
    if (means_dev)
        HIPCHK(hipMemcpyAsync(means_dev, h->sim_means, sizeof(double) * (size_t)nmom * g.ndraw, hipMemcpyDeviceToDevice, h->stream));
    if (counts_dev)
        HIPCHK(hipMemcpyAsync(counts_dev, h->sim_counts, sizeof(int) * (size_t)nmom * g.ndraw, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

// The step with the fixed moments: per-period means of every simulated column, and the weighted squared distance to the
// target moments as the objective of a draw.
extern "C" int egdst_simulate_batch_moments(egdst_handle *h, const double *init, int nsim, const double *randstream_dev,
                                            long long nrand, unsigned long long seed, int rndtype, const double *target,
                                            const double *weight, double *means_dev, int *counts_dev, double *obj_dev)
{
    if (!h || (obj_dev && (!target || !weight)) || (!obj_dev && !means_dev))
        return set_err(EGDST_E_ARG, "egdst_simulate_batch_moments: bad arguments");
    return estimation_step(h, init, nsim, randstream_dev, nrand, seed, rndtype, nullptr, EG_NOUT * h->b.g.nt, target, weight,
                           means_dev, counts_dev, obj_dev, nullptr);
}

// The step with user-defined moments and a full weighting matrix: the objective is e' W e.  Every argument is checked before
// anything is enqueued.  The device sees one record type, egdst_moment_lag; egdst_simulate_batch_spec promotes its
// egdst_moment records with zero lags and `who` names the door in the messages.  cov_dev: the door is
// egdst_simulate_batch_spec_cov, which takes a quantile only with a bandwidth (hi) that keeps p - h and p + h inside (0, 1).
static_assert(sizeof(egdst_moment) == 56, "egdst_moment is 6 ints and 4 doubles (the Python dtype mirrors it)");
static_assert(sizeof(egdst_moment_lag) == 64 && offsetof(egdst_moment_lag, lag2) == 56 && offsetof(egdst_moment_lag, cond_lag) == 60,
              "egdst_moment_lag is egdst_moment and 2 ints (the Python dtype mirrors it)");
// What is wrong with bandwidth h of quantile p (0 < p < 1) for the covariance, or nullptr: the band's ends are the rounded fp64
// difference and sum, as k_quantile_band forms them.
static const char *qnt_band_problem(double p, double h)
{
    if (h == 0.0) return "a quantile has no covariance without a bandwidth (hi)";
    if (!(h > 0.0)) return "the bandwidth of a quantile (hi) is NaN or not positive";   // (NaN fails)
    const double lo = p - h, hi = p + h;
    if (lo <= 0.0) return "the bandwidth of a quantile (hi) reaches p - h <= 0";
    if (hi >= 1.0) return "the bandwidth of a quantile (hi) reaches p + h >= 1";
    return nullptr;
}

// Do the periods [it_first, it_last] shifted by -lag stay inside [0, nt)?  (64-bit: no int lag overflows)
static bool lag_inside(int it_first, int it_last, int lag, int nt)
{
    return (long long)it_first - lag >= 0 && (long long)it_last - lag < nt;
}

static int checked_estimation_step(const char *who, egdst_handle *h, const double *init, int nsim, const double *randstream_dev,
                                   long long nrand, unsigned long long seed, int rndtype, const egdst_moment_lag *spec, int nmom,
                                   const double *target, const double *W, double *means_dev, int *counts_dev, double *obj_dev,
                                   double *cov_dev = nullptr)
{
    const int nout = EG_NOUT, nt = h->b.g.nt;
    for (int j = 0; j < nmom; j++) {
        const egdst_moment_lag &q = spec[j];
        const char *bad = nullptr;
        if (q.kind < 0 || q.kind > 3) bad = "kind is not 0, 1, 2 or 3";
        else if (q.kind == 3 && !(q.lo > 0.0 && q.lo < 1.0)) bad = "the p of a quantile (lo) is not inside (0, 1)";   // (NaN fails both)
        else if (q.kind == 3 && cov_dev && qnt_band_problem(q.lo, q.hi)) bad = qnt_band_problem(q.lo, q.hi);   // (no other door reads hi)
        else if (q.col < 0 || q.col >= nout) bad = "col is outside the simulated columns";
        else if (q.col2 < 0 || q.col2 >= nout) bad = "col2 is outside the simulated columns";
        else if (q.cond_col < -1 || q.cond_col >= nout) bad = "cond_col is outside the simulated columns";
        else if (q.it_first < 0 || q.it_last < q.it_first || q.it_last >= nt) bad = "the period range is empty or outside the model's";
        else if (nsim > 0 && (long long)nsim * (q.it_last - q.it_first + 1) > 2147483647LL) bad = "nsim times its periods overflows a count";
        else if (q.lag2 != 0 && q.kind != 1) bad = "lag2 is set on a kind other than 1";
        else if (q.cond_lag != 0 && q.cond_col == -1) bad = "cond_lag is set without a condition";
        else if (!lag_inside(q.it_first, q.it_last, q.lag2, nt)) bad = "the period range shifted by lag2 leaves the model's periods";
        else if (!lag_inside(q.it_first, q.it_last, q.cond_lag, nt)) bad = "the period range shifted by cond_lag leaves the model's periods";
        if (bad) return set_err(EGDST_E_ARG, "%s: moment %d: %s", who, j, bad);
    }
    return estimation_step(h, init, nsim, randstream_dev, nrand, seed, rndtype, spec, nmom, target, W, means_dev, counts_dev,
                           obj_dev, cov_dev);
}

extern "C" int egdst_simulate_batch_spec(egdst_handle *h, const double *init, int nsim, const double *randstream_dev,
                                         long long nrand, unsigned long long seed, int rndtype, const egdst_moment *spec,
                                         int nmom, const double *target, const double *W, double *means_dev, int *counts_dev,
                                         double *obj_dev)
{
    if (!h || !spec || nmom <= 0 || (obj_dev && (!target || !W)) || (!obj_dev && !means_dev && !counts_dev))
        return set_err(EGDST_E_ARG, "egdst_simulate_batch_spec: bad arguments");
    egdst_moment_lag *rec = (egdst_moment_lag *)calloc((size_t)nmom, sizeof(egdst_moment_lag));   // (zero lags)
    if (!rec) return set_err(EGDST_E_HIP, "egdst_simulate_batch_spec: out of host memory");
    for (int j = 0; j < nmom; j++) memcpy(&rec[j], &spec[j], sizeof(egdst_moment));
    const int rc = checked_estimation_step("egdst_simulate_batch_spec", h, init, nsim, randstream_dev, nrand, seed, rndtype, rec, nmom,
                                           target, W, means_dev, counts_dev, obj_dev);
    if (rc) (void)hipStreamSynchronize(h->stream);   // (a failed step may leave the upload of rec enqueued)
    free(rec);
    return rc;
}

extern "C" int egdst_simulate_batch_spec_lag(egdst_handle *h, const double *init, int nsim, const double *randstream_dev,
                                             long long nrand, unsigned long long seed, int rndtype, const egdst_moment_lag *spec,
                                             int nmom, const double *target, const double *W, double *means_dev, int *counts_dev,
                                             double *obj_dev)
{
    if (!h || !spec || nmom <= 0 || (obj_dev && (!target || !W)) || (!obj_dev && !means_dev && !counts_dev))
        return set_err(EGDST_E_ARG, "egdst_simulate_batch_spec_lag: bad arguments");
    return checked_estimation_step("egdst_simulate_batch_spec_lag", h, init, nsim, randstream_dev, nrand, seed, rndtype, spec, nmom,
                                   target, W, means_dev, counts_dev, obj_dev);
}

// The step with the covariance of the moments: the records and the checks of egdst_simulate_batch_spec_lag, no objective, and
// per draw the matrix k_moment_cov forms from the per-agent scores (include/egdst.h).
extern "C" int egdst_simulate_batch_spec_cov(egdst_handle *h, const double *init, int nsim, const double *randstream_dev,
                                             long long nrand, unsigned long long seed, int rndtype, const egdst_moment_lag *spec,
                                             int nmom, double *means_dev, int *counts_dev, double *cov_dev)
{
    if (!h || !spec || nmom <= 0) return set_err(EGDST_E_ARG, "egdst_simulate_batch_spec_cov: bad arguments");
    if (!cov_dev) return set_err(EGDST_E_ARG, "egdst_simulate_batch_spec_cov: cov_dev is NULL");
    return checked_estimation_step("egdst_simulate_batch_spec_cov", h, init, nsim, randstream_dev, nrand, seed, rndtype, spec, nmom,
                                   nullptr, nullptr, means_dev, counts_dev, nullptr, cov_dev);
}

extern "C" int egdst_cov_parts(void) { return COV_P; }

// The policy at a data panel's observations, every draw of the handle (include/egdst.h).  Every argument is checked before
// anything is enqueued.  The observations are grouped by cell (it, ist) once per call -- a stable permutation, cut into items of
// at most POL_BS observations of one cell -- so that a workgroup of k_policy_obs searches one table of one draw; results go to the
// caller's index, so the grouping shows nowhere.  With a fit asked for, the terms of a slice of draws (EG_POL_SLICE_BYTES) go to
// scratch kept on the handle and k_policy_fit reduces them on the handle's stream before the next slice overwrites them; without,
// no scratch is reserved and the draws go in one launch (65535 at a time: the grid's second dimension).
#ifndef EG_POL_SLICE_BYTES
#define EG_POL_SLICE_BYTES (1ull << 30)
#endif
static_assert(sizeof(egdst_obs) == 40 && offsetof(egdst_obs, cash) == 16 && offsetof(egdst_obs, w) == 32,
              "egdst_obs is 4 ints and 3 doubles (the Python dtype mirrors it)");

extern "C" int egdst_policy_parts(void) { return POL_BS; }

#if MS_NCONT == 0
// The per-observation checks of egdst_policy_batch and egdst_attach_panel, with the observation's index in the message.
static int pol_check_obs(const char *who, const Geom &g, const egdst_obs *obs, int nobs, int resid)
{
    for (int k = 0; k < nobs; k++) {
        const egdst_obs &o = obs[k];
        const char *bad = nullptr;
        if (o.it < 0 || o.it >= g.nt) bad = "it is outside the model's periods";
        else if (o.ist < 0 || o.ist >= MS_NST) bad = "ist is outside the model's states";
        else if (o.id < -1 || o.id >= MS_ND) bad = "id is outside the model's decisions (-1: not observed)";
        else if (o.reserved != 0) bad = "reserved is not 0";
        else if (!(o.cash >= g.a0)) bad = "cash is NaN or below a0";   // (above mmax the policy is extrapolated, as the simulator does from its second period on)
        else if (!(o.w >= 0.0)) bad = "w is NaN or negative";
        else if (resid == 1 && o.cons <= 0.0) bad = "resid = 1 with a consumption that is not positive";
        if (bad) return set_err(EGDST_E_ARG, "%s: observation %d: %s", who, k, bad);
    }
    return 0;
}

// The grouping of both doors: a counting sort by cell keeps the caller's order inside a cell (perm), and every cell's run of the
// permutation is cut into items of at most POL_BS observations, in cell order -- so a period's items are one contiguous range.
static void pol_group(const Geom &g, const egdst_obs *obs, int nobs, std::vector<int> &perm, std::vector<PolItem> &items)
{
    const int ncell = g.nt * MS_NST;
    std::vector<int> first((size_t)ncell + 1, 0);
    perm.assign((size_t)nobs, 0);
    for (int k = 0; k < nobs; k++) first[(size_t)obs[k].it * MS_NST + obs[k].ist + 1]++;
    for (int c = 0; c < ncell; c++) first[c + 1] += first[c];
    {
        std::vector<int> next(first.begin(), first.end() - 1);
        for (int k = 0; k < nobs; k++) perm[next[(size_t)obs[k].it * MS_NST + obs[k].ist]++] = k;
    }
    items.clear();
    for (int c = 0; c < ncell; c++)
        for (int f = first[c]; f < first[c + 1]; f += POL_BS) {
            const int left = first[c + 1] - f;
            items.push_back(PolItem{c / MS_NST, c % MS_NST, f, left < POL_BS ? left : POL_BS});
        }
}
#endif

extern "C" int egdst_policy_batch(egdst_handle *h, const egdst_obs *obs, int nobs, int resid, double *cons_dev, int *id_dev,
                                  double *vf_dev, double *ssr_dev, int *hits_dev)
{
    const char *who = "egdst_policy_batch";
    if (!h || !obs || nobs <= 0) return set_err(EGDST_E_ARG, "%s: bad arguments", who);
#if MS_NCONT > 0
    return set_err(EGDST_E_ARG, "%s: a model with continuous states is not served (its policy is a blend over grid corners)", who);
#else
    if (resid != 0 && resid != 1) return set_err(EGDST_E_ARG, "%s: resid is not 0 or 1", who);
    if (!cons_dev && !id_dev && !vf_dev && !ssr_dev && !hits_dev) return set_err(EGDST_E_ARG, "%s: no output is given", who);
    if (!h->keep_history) return set_err(EGDST_E_ARG, "%s: needs keep_history=1", who);
    if (!h->solved) return set_err(EGDST_E_NOT_SOLVED, "%s", egdst_strerror(EGDST_E_NOT_SOLVED));
    if (!h->params_set && MS_NPARAM) return set_err(EGDST_E_ARG, "%s: parameters not set", who);
    const Geom &g = h->b.g;
    int rc = pol_check_obs(who, g, obs, nobs, resid);
    if (rc) return rc;
    std::vector<int> perm;
    std::vector<PolItem> items;
    pol_group(g, obs, nobs, perm, items);
    const bool fit = ssr_dev || hits_dev;
    const size_t per_draw = (sizeof(double) + sizeof(int)) * (size_t)nobs;
    int slice = fit ? (int)(EG_POL_SLICE_BYTES / per_draw) : g.ndraw;
    if (slice > 65535) slice = 65535;
    if (slice < 1) slice = 1;
    if (slice > g.ndraw) slice = g.ndraw;
    rc = sim_reserve((void **)&h->pol_obs, &h->pol_obs_bytes, sizeof(egdst_obs) * (size_t)nobs);
    if (!rc) rc = sim_reserve((void **)&h->pol_perm, &h->pol_perm_bytes, sizeof(int) * (size_t)nobs);
    if (!rc) rc = sim_reserve((void **)&h->pol_items, &h->pol_items_bytes, sizeof(PolItem) * items.size());
    if (!rc && fit) rc = sim_reserve((void **)&h->pol_term, &h->pol_term_bytes, sizeof(double) * (size_t)nobs * slice);
    if (!rc && fit) rc = sim_reserve((void **)&h->pol_flag, &h->pol_flag_bytes, sizeof(int) * (size_t)nobs * slice);
    if (rc) return rc;
    hipStream_t s = h->stream;
    const Batch *bdev = nullptr;
    rc = batch_for_call(h, &bdev);
    if (rc) return rc;
    hipError_t e = hipMemcpyAsync(h->pol_obs, obs, sizeof(egdst_obs) * (size_t)nobs, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(h->pol_perm, perm.data(), sizeof(int) * (size_t)nobs, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(h->pol_items, items.data(), sizeof(PolItem) * items.size(), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(s);   // (an upload may still read the vectors)
        return set_err(EGDST_E_HIP, "%s: upload failed: %s", who, hipGetErrorString(e));
    }
    PolArgs a;
    a.nobs = nobs, a.resid = resid;
    a.obs = h->pol_obs, a.perm = h->pol_perm, a.items = h->pol_items;
    a.cons = cons_dev, a.vf = vf_dev, a.id = id_dev;
    a.term = fit ? h->pol_term : nullptr, a.flag = fit ? h->pol_flag : nullptr;
    for (int d0 = 0; d0 < g.ndraw; d0 += slice) {
        const int nd = (g.ndraw - d0 < slice) ? g.ndraw - d0 : slice;
        a.draw0 = d0;
        hipLaunchKernelGGL(k_policy_obs, dim3((unsigned)items.size(), nd), dim3(POL_BS), 0, s, bdev, a);
        if (fit)
            hipLaunchKernelGGL(k_policy_fit, dim3(nd), dim3(POL_BS), 0, s, bdev, d0, nobs, (const double *)h->pol_term,
                               (const int *)h->pol_flag, ssr_dev, hits_dev);
    }
    e = hipGetLastError();
    const hipError_t e2 = hipStreamSynchronize(s);   // (the uploads read perm and items; the results are written on return)
    if (e != hipSuccess || e2 != hipSuccess) return set_err(EGDST_E_HIP, "%s: %s", who, hipGetErrorString(e != hipSuccess ? e : e2));
    return 0;
#endif
}

// The resident panel (include/egdst.h): egdst_policy_batch's checks and grouping, done once; the observations, the permutation and
// the items stay on the device, the host keeps where each period's items begin, and the terms of every (draw, observation) have
// storage of their own, which the solves fill (enqueue_panel) and egdst_fit_dev reduces with k_policy_fit.  A one-time host call:
// it waits for the handle's stream, since a solve still running there reads the panel it replaces.
static void panel_free(egdst_handle *h)
{
    void *bufs[] = {h->pan_obs, h->pan_perm, h->pan_flag, h->pan_items, h->pan_term};
    for (void *p : bufs)
        if (p) (void)hipFree(p);
    h->pan_obs = nullptr, h->pan_perm = nullptr, h->pan_flag = nullptr, h->pan_items = nullptr, h->pan_term = nullptr;
    free(h->pan_first);
    h->pan_first = nullptr;
    h->pan_nobs = h->pan_resid = h->pan_fit = 0;
}

extern "C" int egdst_attach_panel(egdst_handle *h, const egdst_obs *obs, int nobs, int resid)
{
    const char *who = "egdst_attach_panel";
    if (!h || nobs < 0 || (!obs) != (nobs == 0)) return set_err(EGDST_E_ARG, "%s: bad arguments", who);
    if (!obs) {   // detach
        HIPCHK(hipStreamSynchronize(h->stream));
        panel_free(h);
        return 0;
    }
#if MS_NCONT > 0
    return set_err(EGDST_E_ARG, "%s: a model with continuous states is not served (its policy is a blend over grid corners)", who);
#else
    if (resid != 0 && resid != 1) return set_err(EGDST_E_ARG, "%s: resid is not 0 or 1", who);
    const Geom &g = h->b.g;
    int rc = pol_check_obs(who, g, obs, nobs, resid);
    if (rc) return rc;
    std::vector<int> perm;
    std::vector<PolItem> items;
    pol_group(g, obs, nobs, perm, items);
    int *first = (int *)malloc(sizeof(int) * ((size_t)g.nt + 1));
    if (!first) return set_err(EGDST_E_HIP, "%s: out of host memory", who);
    {   // items are in cell order, so in period order
        size_t i = 0;
        for (int it = 0; it <= g.nt; it++) {
            while (i < items.size() && items[i].it < it) i++;
            first[it] = (int)i;
        }
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    panel_free(h);
    const size_t pairs = (size_t)nobs * g.ndraw;
    struct { void **p; size_t bytes; const void *src; } bufs[] = {
        {(void **)&h->pan_obs, sizeof(egdst_obs) * (size_t)nobs, obs},
        {(void **)&h->pan_perm, sizeof(int) * (size_t)nobs, perm.data()},
        {(void **)&h->pan_items, sizeof(PolItem) * items.size(), items.data()},
        {(void **)&h->pan_term, sizeof(double) * pairs, nullptr},
        {(void **)&h->pan_flag, sizeof(int) * pairs, nullptr}};
    for (auto &bf : bufs) {
        hipError_t e = hipMalloc(bf.p, bf.bytes);
        if (e == hipSuccess && bf.src) e = hipMemcpy(*bf.p, bf.src, bf.bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipGetLastError();   // (the failure is reported here: it is not left for the next launch's check to find)
            panel_free(h);
            free(first);
            return set_err(EGDST_E_HIP, "%s: %zu bytes on the device (%d observations x %d draws): %s", who, bf.bytes, nobs, g.ndraw,
                           hipGetErrorString(e));
        }
    }
    h->pan_first = first;
    h->pan_nobs = nobs, h->pan_resid = resid;
    h->pan_fit = 0;   // (no fit until the next solve has written the terms)
    return 0;
#endif
}

extern "C" int egdst_fit_dev(egdst_handle *h, double *ssr_dev, int *hits_dev)
{
    if (!h || (!ssr_dev && !hits_dev)) return set_err(EGDST_E_ARG, "egdst_fit_dev: bad arguments");
    if (!h->pan_nobs) return set_err(EGDST_E_ARG, "egdst_fit_dev: no panel is attached (egdst_attach_panel)");
    if (!h->pan_fit) return set_err(EGDST_E_NOT_SOLVED, "egdst_fit_dev: no solve since the panel was attached or a solution was imported");
    const Batch *bdev = nullptr;
    int rc = batch_for_call(h, &bdev);
    if (rc) return rc;
    hipLaunchKernelGGL(k_policy_fit, dim3(h->b.g.ndraw), dim3(POL_BS), 0, h->stream, bdev, 0, h->pan_nobs, (const double *)h->pan_term,
                       (const int *)h->pan_flag, ssr_dev, hits_dev);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int egdst_get_fit(egdst_handle *h, double *ssr, int *hits)
{
    if (!h || (!ssr && !hits)) return set_err(EGDST_E_ARG, "egdst_get_fit: bad arguments");
    // (staged in the handle's objective buffer, 2 x ndraw doubles: ssr in its first half, hits in its second)
    double *ssr_dev = h->b.obj;
    int *hits_dev = (int *)(h->b.obj + h->b.g.ndraw);
    int rc = egdst_fit_dev(h, ssr_dev, hits_dev);
    if (rc) return rc;
    if (ssr) HIPCHK(hipMemcpyAsync(ssr, ssr_dev, sizeof(double) * h->b.g.ndraw, hipMemcpyDeviceToHost, h->stream));
    if (hits) HIPCHK(hipMemcpyAsync(hits, hits_dev, sizeof(int) * h->b.g.ndraw, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

// egdst_call.c:17-164.  The index checks of the gateway are done here, in row order, because an out-of-range index
// turns the switch to -1 for the rest of the call (that row and every later one are NaN) and a wrong column count
// returns before anything is computed (the result stays zero); the rows before the first bad one are independent.
extern "C" int egdst_call(egdst_handle *h, int draw, int sw, int narg, int ncol, const double *args, double *res)
{
    int rc = check_cell(h, draw, 0, 0);
    if (rc) return rc;
    if (!args || !res || narg < 1 || ncol < 1) return set_err(EGDST_E_ARG, "egdst_call: bad arguments");
    if (!h->params_set && MS_NPARAM) return set_err(EGDST_E_ARG, "egdst_call: parameters not set");
    const Geom &g = h->b.g;
    const size_t n = (size_t)narg;
    for (int i = 0; i < narg; i++) res[i] = 0.0;
    int first_bad = narg, keeps_zero = 0;
    const int want = (sw == 1 || sw == 2) ? 4 : (sw == 3 ? 2 : ((sw == 4 || sw == 5) ? 6 : (sw == 6 ? 3 : 0)));
    for (int i = 0; i < narg && first_bad == narg; i++) {
        const double *arg = args + i;
        const int it = (int)arg[0] - g.t0, ist = (ncol > 1) ? (int)arg[n] - 1 : -1;
        bool bad = it < 0 || it > g.nt - 1 || ist < 0 || ist >= MS_NST;
        if (ncol > 2 && sw != 6) {
            const int id = (int)arg[2 * n] - 1;
            bad = bad || id < 0 || id >= MS_ND;
        }
        if (bad || want == 0) {  // (an unknown switch: every row is NaN as well)
            first_bad = i;
            break;
        }
        if (ncol != want) return 0;  // "Wrong number of arguments": returns at the first row, zeros stay
        if (sw == 4 || sw == 5) {
            const int it1 = it + 1, ist1 = (int)arg[4 * n] - 1;
            if (!(it1 > g.nt - 1) && !(arg[3 * n] < g.a0) && (ist1 < 0 || ist1 >= MS_NST)) first_bad = i, keeps_zero = 1;
        }
    }
    // arguments and results go through the handle's simulator buffers (kept, grown on demand: nothing leaks on an error path)
    rc = sim_reserve((void **)&h->sim_rs, &h->sim_rs_bytes, sizeof(double) * n * ncol);
    if (!rc) rc = sim_reserve((void **)&h->sim_means, &h->sim_means_bytes, sizeof(double) * n);
    if (rc) return rc;
    double *d_args = h->sim_rs, *d_res = h->sim_means;
    hipStream_t s = h->stream;
    HIPCHK(hipMemcpyAsync(d_args, args, sizeof(double) * n * ncol, hipMemcpyHostToDevice, s));
    CallArgs a;
    a.draw = draw, a.sw = sw, a.narg = narg, a.ncol = ncol, a.first_bad = first_bad, a.bad_keeps_zero = keeps_zero;
    a.args = d_args, a.res = d_res;
    const Batch *bdev = nullptr;
    rc = batch_for_call(h, &bdev);
    if (rc) return rc;
    hipLaunchKernelGGL(k_call, dim3((narg + GRID_BS - 1) / GRID_BS), dim3(GRID_BS), 0, s, bdev, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(res, d_res, sizeof(double) * n, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

extern "C" int egdst_objective_dev(egdst_handle *h, double *out_dev)
{
    if (!h || !out_dev) return set_err(EGDST_E_ARG, "egdst_objective_dev: bad arguments");
    if (!h->solved) return set_err(EGDST_E_NOT_SOLVED, "%s", egdst_strerror(EGDST_E_NOT_SOLVED));
    const Batch *bdev = nullptr;
    int rc = batch_for_call(h, &bdev);
    if (rc) return rc;
    hipLaunchKernelGGL(k_objective, dim3((h->b.g.ndraw + 63) / 64), dim3(64), 0, h->stream, bdev, out_dev);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int egdst_get_objective(egdst_handle *h, double *out)
{
    if (!h || !out) return set_err(EGDST_E_ARG, "egdst_get_objective: bad arguments");
    int rc = egdst_objective_dev(h, h->b.obj);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(out, h->b.obj, sizeof(double) * 2 * h->b.g.ndraw, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" int egdst_get_params(egdst_handle *h, double *out)
{
    if (!h || !out) return set_err(EGDST_E_ARG, "egdst_get_params: bad arguments");
    HIPCHK(hipMemcpyAsync(out, h->b.par, sizeof(double) * (size_t)h->b.g.ndraw * (MS_NPARAM ? MS_NPARAM : 1),
                          hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" int egdst_set_profile(egdst_handle *h, int on)
{
    if (!h) return set_err(EGDST_E_ARG, "null handle");
    if (on && !h->ev) {
        h->nev = EGDST_MAX_GROUPS * EG_NPROF * h->b.g.nt * 2;
        h->ev = (hipEvent_t *)calloc(h->nev, sizeof(hipEvent_t));   // (created when first recorded, enqueue_solve)
    }
    h->profile = on ? 1 : 0;
    return 0;
}

// Device time of the last solve by kernel class: ms[9] and launches[9] (classes: see include/egdst.h);
// algbytes: compulsory table bytes of the solve summed over draws.
extern "C" int egdst_get_profile(egdst_handle *h, double *ms, int *launches, long long *algbytes)
{
    if (!h) return set_err(EGDST_E_ARG, "null handle");
    HIPCHK(hipStreamSynchronize(h->stream));
    const Geom &g = h->b.g;
    if (ms && launches) {
        for (int k = 0; k < EG_NPROF; k++) ms[k] = 0, launches[k] = 0;
        if (h->ev && h->profile)
            for (int gi = 0; gi < h->nlanes; gi++)
                for (int k = 0; k < EG_NPROF; k++)
                    for (int it = 0; it < g.nt; it++) {
                        if ((k == 1 || k >= 3) && it == g.nt - 1) continue;  // the terminal period: k_terminal and k_envelope only
                        const size_t e0 = (((size_t)gi * EG_NPROF + k) * g.nt + it) * 2;
                        float t = 0;
                        if (h->ev[e0] && h->ev[e0 + 1] && hipEventElapsedTime(&t, h->ev[e0], h->ev[e0 + 1]) == hipSuccess) {
                            ms[k] += t;
                            launches[k]++;
                        }
                    }
    }
    if (algbytes) {
        unsigned long long *tmp = (unsigned long long *)malloc(sizeof(unsigned long long) * g.ndraw);
        hipError_t e = hipMemcpy(tmp, h->b.algbytes, sizeof(unsigned long long) * g.ndraw, hipMemcpyDeviceToHost);
        long long t = 0;
        if (e == hipSuccess)
            for (int i = 0; i < g.ndraw; i++) t += (long long)tmp[i];
        free(tmp);
        if (e != hipSuccess) return set_err(EGDST_E_HIP, "algbytes copy failed: %s", hipGetErrorString(e));
        *algbytes = t;
    }
    return 0;
}

extern "C" int egdst_get_group_profile(egdst_handle *h, int max_groups, double *out_ms, double *out_class_ms)
{
    if (!h || !out_ms || max_groups < 1) return set_err(EGDST_E_ARG, "egdst_get_group_profile: bad arguments");
    HIPCHK(hipStreamSynchronize(h->stream));
    const Geom &g = h->b.g;
    if (!h->ev || !h->profile) return 0;
    const int ng = h->nlanes < max_groups ? h->nlanes : max_groups;
    // the first event of the solve: class 0 (k_terminal) of the terminal period, group 0 is launched first
    hipEvent_t first = h->ev[(((size_t)0 * EG_NPROF + 0) * g.nt + (g.nt - 1)) * 2];
    for (int gi = 0; gi < ng; gi++) {
        out_ms[gi] = 0;
        // the last bracketed launch of a group: k_envelope (class 2) of period 0
        hipEvent_t last = h->ev[(((size_t)gi * EG_NPROF + 2) * g.nt + 0) * 2 + 1];
        float t = 0;
        if (first && last && hipEventElapsedTime(&t, first, last) == hipSuccess) out_ms[gi] = t;
        if (out_class_ms)
            for (int k = 0; k < EG_NPROF; k++) {
                double acc = 0;
                for (int it = 0; it < g.nt; it++) {
                    const size_t e0 = (((size_t)gi * EG_NPROF + k) * g.nt + it) * 2;
                    float d = 0;
                    if (h->ev[e0] && h->ev[e0 + 1] && hipEventElapsedTime(&d, h->ev[e0], h->ev[e0 + 1]) == hipSuccess) acc += d;
                }
                out_class_ms[gi * EG_NPROF + k] = acc;
            }
    }
    return ng;
}

extern "C" int egdst_get_debug(egdst_handle *h, int draw, int *out16)
{
    if (!h || !out16 || draw < 0 || draw >= h->b.g.ndraw) return set_err(EGDST_E_ARG, "egdst_get_debug: bad arguments");
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(out16, h->b.dbg + 16 * draw, sizeof(int) * 16, hipMemcpyDeviceToHost));
    return 0;
}

// Clock stamps of a diagnostic build (egdst_device.h): the names of the slots, the same table in every build, and one draw's
// slots as the last solve left them -- which only a library built with -DEGDST_STAMPS=<set> has.
extern "C" int egdst_stamp_names(const char **names, int cap)
{
#define EG_STAMP_NAME_(set, slot, name) name,
    static const char *const tab[EG_NSTAMP] = {EG_STAMP_SLOTS(EG_STAMP_NAME_)};
    for (int i = 0; names && i < cap && i < EG_NSTAMP; i++) names[i] = tab[i];
    return EG_NSTAMP;
}

extern "C" int egdst_get_stamps(egdst_handle *h, int draw, unsigned long long *out)
{
    if (!h || !out || draw < 0 || draw >= h->b.g.ndraw) return set_err(EGDST_E_ARG, "egdst_get_stamps: bad arguments");
#ifdef EGDST_STAMPS
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(out, h->b.stamps + (size_t)EG_NSTAMP * draw, sizeof(unsigned long long) * EG_NSTAMP, hipMemcpyDeviceToHost));
    return 0;
#else
    return set_err(EGDST_E_ARG, "egdst_get_stamps: this library was built without -DEGDST_STAMPS=<set>");
#endif
}

extern "C" int egdst_device_tables(egdst_handle *h, int it, const double **M_dev, const double **C_dev,
                                   const double **V_dev, const int **len_dev)
{
    if (!h || it < 0 || it >= h->b.g.nt) return set_err(EGDST_E_ARG, "egdst_device_tables: bad arguments");
    const Geom &g = h->b.g;
    const int slot = (g.nslots == 2) ? (it & 1) : it;
    const size_t k = (size_t)slot * g.ndraw * MS_NST;
    if (M_dev) *M_dev = h->b.tM + k * g.Sp;
    if (C_dev) *C_dev = h->b.tC + k * g.Sp;
    if (V_dev) *V_dev = h->b.tV + k * g.Sp;
    if (len_dev) *len_dev = h->b.tlen + k;
    return 0;
}

extern "C" int egdst_get_checksums(egdst_handle *h, int draw, unsigned long long *out)
{
    int rc = check_cell(h, draw, 0, 0);
    if (rc) return rc;
    if (!out) return set_err(EGDST_E_ARG, "egdst_get_checksums: bad arguments");
    const size_t n = (size_t)h->b.g.nt * MS_NST * 5;
    unsigned long long *d = nullptr;
    HIPCHK(hipMalloc(&d, sizeof(unsigned long long) * n));
    const Batch *bdev = nullptr;
    rc = batch_for_call(h, &bdev);
    if (rc) {
        (void)hipFree(d);
        return rc;
    }
    hipLaunchKernelGGL(k_checksum, dim3(h->b.g.nt * MS_NST), dim3(CHK_BS), 0, h->stream, bdev, draw, d);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(out, d, sizeof(unsigned long long) * n, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    (void)hipFree(d);
    if (e != hipSuccess) return set_err(EGDST_E_HIP, "egdst_get_checksums: %s", hipGetErrorString(e));
    return 0;
}

extern "C" int egdst_math_eval(int fn, int n, const double *x, const double *y, double *out)
{
    if (fn < 0 || fn > 4 || n < 1 || !x || !out || (fn >= 2 && !y)) return set_err(EGDST_E_ARG, "egdst_math_eval: bad arguments");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return set_err(EGDST_E_NOGPU, "%s", egdst_strerror(EGDST_E_NOGPU));
    double *d = nullptr;
    const size_t nx = (size_t)n * (fn >= 3 ? 3 : 1), ny = (size_t)n * (fn >= 3 ? 2 : 1);  // (fn 3, 4: x = [x | g0 | g1], y = [f0 | f1])
    HIPCHK(hipMalloc(&d, sizeof(double) * (nx + ny + (size_t)n)));
    hipError_t e = hipMemcpy(d, x, sizeof(double) * nx, hipMemcpyHostToDevice);
    if (e == hipSuccess && fn >= 2) e = hipMemcpy(d + nx, y, sizeof(double) * ny, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_math_eval, dim3((n + 255) / 256), dim3(256), 0, 0, fn, n, (const double *)d, (const double *)(d + nx), d + nx + ny);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(out, d + nx + ny, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return set_err(EGDST_E_HIP, "egdst_math_eval: %s", hipGetErrorString(e));
    return 0;
}

extern "C" int egdst_quantile_lds_keys(void) { return QNT_LDS_KEYS; }

// The selection of k_quantiles on caller-supplied values (diagnostics): x becomes column 0 of an [n][1][EG_NOUT] panel whose
// other columns are NaN, p[i] the kind-3 record i over that one period, and the kernel runs as in the estimation step.
extern "C" int egdst_quantile_eval(int n, const double *x, int np, const double *p, double *out, int *count)
{
    if (n < 1 || np < 1 || !x || !p || !out || !count) return set_err(EGDST_E_ARG, "egdst_quantile_eval: bad arguments");
    for (int i = 0; i < np; i++)
        if (!(p[i] > 0.0 && p[i] < 1.0)) return set_err(EGDST_E_ARG, "egdst_quantile_eval: p[%d] is not inside (0, 1)", i);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return set_err(EGDST_E_NOGPU, "%s", egdst_strerror(EGDST_E_NOGPU));
    const size_t npanel = (size_t)n * EG_NOUT;
    double *panel = (double *)malloc(sizeof(double) * npanel);
    egdst_moment_lag *rec = (egdst_moment_lag *)calloc((size_t)np, sizeof(egdst_moment_lag));
    int *cnt = (int *)malloc(sizeof(int) * (size_t)np);
    double *d_panel = nullptr, *d_means = nullptr;
    egdst_moment_lag *d_rec = nullptr;
    int *d_cnt = nullptr;
    if (!panel || !rec || !cnt) {
        free(panel), free(rec), free(cnt);
        return set_err(EGDST_E_HIP, "egdst_quantile_eval: out of host memory");
    }
    for (size_t i = 0; i < npanel; i++) panel[i] = NAN;
    for (int i = 0; i < n; i++) panel[(size_t)i * EG_NOUT] = x[i];
    for (int i = 0; i < np; i++) rec[i].kind = 3, rec[i].cond_col = -1, rec[i].lo = p[i];
    hipError_t e = hipMalloc(&d_panel, sizeof(double) * npanel);
    if (e == hipSuccess) e = hipMalloc(&d_rec, sizeof(egdst_moment_lag) * (size_t)np);
    if (e == hipSuccess) e = hipMalloc(&d_means, sizeof(double) * (size_t)np);
    if (e == hipSuccess) e = hipMalloc(&d_cnt, sizeof(int) * (size_t)np);
    if (e == hipSuccess) e = hipMemcpy(d_panel, panel, sizeof(double) * npanel, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_rec, rec, sizeof(egdst_moment_lag) * (size_t)np, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_quantiles, dim3(np), dim3(QNT_BS), 0, 0, (const double *)d_panel, n, 1, (const egdst_moment_lag *)d_rec, 0, np,
                           d_means, d_cnt);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(out, d_means, sizeof(double) * (size_t)np, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(cnt, d_cnt, sizeof(int) * (size_t)np, hipMemcpyDeviceToHost);
    if (e == hipSuccess) *count = cnt[0];   // (the records share the column and the period: one count)
    if (d_panel) (void)hipFree(d_panel);
    if (d_rec) (void)hipFree(d_rec);
    if (d_means) (void)hipFree(d_means);
    if (d_cnt) (void)hipFree(d_cnt);
    free(panel), free(rec), free(cnt);
    if (e != hipSuccess) return set_err(EGDST_E_HIP, "egdst_quantile_eval: %s", hipGetErrorString(e));
    return 0;
}

// k_quantile_band on caller-supplied values (diagnostics), the panel and the records laid out as egdst_quantile_eval does: record i
// is quantile p[i] with bandwidth h[i]; out [np][3] receives the band's ends a, b and the sparsity s.  k_quantiles runs beside it
// only for the count.
extern "C" int egdst_quantile_band_eval(int n, const double *x, int np, const double *p, const double *hband, double *out, int *count)
{
    const char *who = "egdst_quantile_band_eval";
    if (n < 1 || np < 1 || !x || !p || !hband || !out || !count) return set_err(EGDST_E_ARG, "%s: bad arguments", who);
    for (int i = 0; i < np; i++) {
        if (!(p[i] > 0.0 && p[i] < 1.0)) return set_err(EGDST_E_ARG, "%s: p[%d] is not inside (0, 1)", who, i);
        if (qnt_band_problem(p[i], hband[i])) return set_err(EGDST_E_ARG, "%s: record %d: %s", who, i, qnt_band_problem(p[i], hband[i]));
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return set_err(EGDST_E_NOGPU, "%s", egdst_strerror(EGDST_E_NOGPU));
    const size_t npanel = (size_t)n * EG_NOUT;
    double *panel = (double *)malloc(sizeof(double) * npanel);
    egdst_moment_lag *rec = (egdst_moment_lag *)calloc((size_t)np, sizeof(egdst_moment_lag));
    double *res = (double *)malloc(sizeof(double) * 3 * (size_t)np);   // [np] sparsities, then [np][2] ends
    int *cnt = (int *)malloc(sizeof(int) * (size_t)np);
    double *d_panel = nullptr, *d_res = nullptr, *d_means = nullptr;
    egdst_moment_lag *d_rec = nullptr;
    int *d_cnt = nullptr;
    if (!panel || !rec || !res || !cnt) {
        free(panel), free(rec), free(res), free(cnt);
        return set_err(EGDST_E_HIP, "%s: out of host memory", who);
    }
    for (size_t i = 0; i < npanel; i++) panel[i] = NAN;
    for (int i = 0; i < n; i++) panel[(size_t)i * EG_NOUT] = x[i];
    for (int i = 0; i < np; i++) rec[i].kind = 3, rec[i].cond_col = -1, rec[i].lo = p[i], rec[i].hi = hband[i];
    hipError_t e = hipMalloc(&d_panel, sizeof(double) * npanel);
    if (e == hipSuccess) e = hipMalloc(&d_rec, sizeof(egdst_moment_lag) * (size_t)np);
    if (e == hipSuccess) e = hipMalloc(&d_res, sizeof(double) * 3 * (size_t)np);
    if (e == hipSuccess) e = hipMalloc(&d_means, sizeof(double) * (size_t)np);
    if (e == hipSuccess) e = hipMalloc(&d_cnt, sizeof(int) * (size_t)np);
    if (e == hipSuccess) e = hipMemcpy(d_panel, panel, sizeof(double) * npanel, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_rec, rec, sizeof(egdst_moment_lag) * (size_t)np, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_quantiles, dim3(np), dim3(QNT_BS), 0, 0, (const double *)d_panel, n, 1, (const egdst_moment_lag *)d_rec, 0, np,
                           d_means, d_cnt);
        hipLaunchKernelGGL(k_quantile_band, dim3(np), dim3(QNT_BS), 0, 0, (const double *)d_panel, n, 1, (const egdst_moment_lag *)d_rec, 0,
                           np, d_res, d_res + np);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(res, d_res, sizeof(double) * 3 * (size_t)np, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(cnt, d_cnt, sizeof(int) * (size_t)np, hipMemcpyDeviceToHost);
    if (e == hipSuccess) {
        for (int i = 0; i < np; i++) out[3 * i] = res[np + 2 * i], out[3 * i + 1] = res[np + 2 * i + 1], out[3 * i + 2] = res[i];
        *count = cnt[0];   // (the records share the column and the period: one count)
    }
    if (d_panel) (void)hipFree(d_panel);
    if (d_rec) (void)hipFree(d_rec);
    if (d_res) (void)hipFree(d_res);
    if (d_means) (void)hipFree(d_means);
    if (d_cnt) (void)hipFree(d_cnt);
    free(panel), free(rec), free(res), free(cnt);
    if (e != hipSuccess) return set_err(EGDST_E_HIP, "%s: %s", who, hipGetErrorString(e));
    return 0;
}

// Third output of the solver gateway ([M,D,dbgout] = egdst_solver(model), egdst_solver.c:178-181,1866-1879): with the log
// on, every kink the envelopes record is kept per cell on the device; egdst_get_dbgout lays the rows of one draw out in
// the order the reference writes them (periods backwards, states ascending, within a cell the secondary envelopes by
// choice, then the primary one) in a [cap x 7] column-major matrix, cap = nt*nst*nd*2*nt, rows beyond cap dropped.
extern "C" int egdst_set_dbgout(egdst_handle *h, int on)
{
    if (!h) return set_err(EGDST_E_ARG, "egdst_set_dbgout: null handle");
    HIPCHK(hipStreamSynchronize(h->stream));
    h->call_slot_ok = 0;  // (the Batch changes below)
    Batch &b = h->b;
    const Geom &g = b.g;
    if (!on) {
        if (b.klog) (void)hipFree(b.klog);
        if (b.kcnt) (void)hipFree(b.kcnt);
        b.klog = nullptr, b.kcnt = nullptr, b.kcap = 0;
        return 0;
    }
    if (b.klog) return 0;
    const long long total = (long long)g.nt * MS_NST * MS_ND * 2 * g.nt;     // rows of the gateway's matrix
    long long cap = (long long)(MS_ND + 1) * g.nthrhmax;                      // kinks a cell can record at most
    if (cap > total) cap = total;
    const size_t cells = (size_t)g.nt * g.ndraw * MS_NST;
    HIPCHK(hipMalloc(&b.klog, sizeof(double) * 4 * (size_t)cap * cells));
    hipError_t e = hipMalloc(&b.kcnt, sizeof(int) * cells);
    if (e != hipSuccess) {
        (void)hipFree(b.klog);
        b.klog = nullptr;
        return set_err(EGDST_E_HIP, "egdst_set_dbgout: %s", hipGetErrorString(e));
    }
    b.kcap = (int)cap;
    HIPCHK(hipMemsetAsync(b.kcnt, 0, sizeof(int) * cells, h->stream));
    return 0;
}

extern "C" int egdst_get_dbgout(egdst_handle *h, int draw, double *out, int *nrows)
{
    if (!h || !out || draw < 0 || draw >= h->b.g.ndraw) return set_err(EGDST_E_ARG, "egdst_get_dbgout: bad arguments");
    if (!h->b.klog) return set_err(EGDST_E_ARG, "egdst_get_dbgout: call egdst_set_dbgout(h, 1) before solving");
    if (!h->solved) return set_err(EGDST_E_NOT_SOLVED, "%s", egdst_strerror(EGDST_E_NOT_SOLVED));
    const Batch &b = h->b;
    const Geom &g = b.g;
    const int cap = g.nt * MS_NST * MS_ND * 2 * g.nt;
    for (size_t i = 0; i < (size_t)cap * 7; i++) out[i] = 0.0;  // (mxCreateDoubleMatrix zero-fills)
    HIPCHK(hipStreamSynchronize(h->stream));
    double *rows = (double *)malloc(sizeof(double) * 4 * (size_t)b.kcap);
    int n = 0;
    for (int it = g.nt - 1; it >= 0; it--)
        for (int ist = 0; ist < MS_NST; ist++) {
            const size_t kc = ((size_t)it * g.ndraw + draw) * MS_NST + ist;
            int cnt = 0;
            hipError_t e = hipMemcpy(&cnt, b.kcnt + kc, sizeof(int), hipMemcpyDeviceToHost);
            if (cnt > b.kcap) cnt = b.kcap;
            if (e == hipSuccess && cnt > 0)
                e = hipMemcpy(rows, b.klog + kc * 4 * (size_t)b.kcap, sizeof(double) * 4 * (size_t)cnt, hipMemcpyDeviceToHost);
            if (e != hipSuccess) {
                free(rows);
                return set_err(EGDST_E_HIP, "egdst_get_dbgout: %s", hipGetErrorString(e));
            }
            for (int k = 0; k < cnt && n < cap; k++, n++) {
                const double *r = rows + 4 * (size_t)k;
                out[n] = it;
                out[n + (size_t)cap] = ist;
                out[n + 2 * (size_t)cap] = r[0];
                out[n + 3 * (size_t)cap] = r[1];
                out[n + 4 * (size_t)cap] = (r[2] == EG_ZEROC) ? -.9999 : r[2];
                out[n + 5 * (size_t)cap] = (r[3] == EG_ZEROC) ? -.9999 : r[3];
                out[n + 6 * (size_t)cap] = fabs(r[3] - r[2]);
            }
        }
    free(rows);
    if (nrows) *nrows = n;
    return 0;
}

extern "C" int egdst_get_tp_inplace(egdst_handle *h, unsigned *out)
{
    if (!h || !out) return set_err(EGDST_E_ARG, "egdst_get_tp_inplace: bad arguments");
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(out, h->b.tpinplace, sizeof(unsigned) * h->b.g.ndraw, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int egdst_get_tp_tail_counts(egdst_handle *h, int max_groups, int *rest, int *big)
{
    if (!h || !rest || !big || max_groups < 1) return set_err(EGDST_E_ARG, "egdst_get_tp_tail_counts: bad arguments");
    const size_t n = (size_t)(max_groups < EGDST_MAX_GROUPS ? max_groups : EGDST_MAX_GROUPS) * h->b.g.nt;
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(rest, h->b.tpn, sizeof(int) * n, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(big, h->b.tpbign, sizeof(int) * n, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int egdst_get_tp_stats(egdst_handle *h, unsigned *out)
{
    if (!h || !out) return set_err(EGDST_E_ARG, "egdst_get_tp_stats: bad arguments");
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(out, h->b.tpstat, sizeof(unsigned) * 2 * h->b.g.ndraw, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int egdst_get_walk_stats(egdst_handle *h, unsigned *out)
{
    if (!h || !out) return set_err(EGDST_E_ARG, "egdst_get_walk_stats: bad arguments");
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(out, h->b.segstat, sizeof(unsigned) * 2 * h->b.g.ndraw, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int egdst_get_sort_stats(egdst_handle *h, unsigned *out)
{
    if (!h || !out) return set_err(EGDST_E_ARG, "egdst_get_sort_stats: bad arguments");
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(out, h->b.sortstat, sizeof(unsigned) * 4 * h->b.g.ndraw, hipMemcpyDeviceToHost));
    return 0;
}

#ifdef EGDST_CENSUS
// diagnostic build only (tests/diag/gpu_census.py): the records of the device-side census, 8 ints each; returns how many were
// written (may exceed cap: the log is full), optionally clears the log
extern "C" int egdst_census_read(int *out, int cap, int reset)
{
    unsigned n = 0;
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(&n, HIP_SYMBOL(g_census_n), sizeof n) != hipSuccess) return -1;
    unsigned m = n < (unsigned)EG_CENSUS_CAP ? n : (unsigned)EG_CENSUS_CAP;
    if (m > (unsigned)cap) m = (unsigned)cap;
    if (out && m && hipMemcpyFromSymbol(out, HIP_SYMBOL(g_census), sizeof(int) * 8 * (size_t)m) != hipSuccess) return -1;
    if (reset) {
        const unsigned z = 0;
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_census_n), &z, sizeof z) != hipSuccess) return -1;
    }
    return (int)n;
}
#endif
