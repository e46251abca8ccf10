/*
 * include/tsp_hip.h -- C ABI of libtsp_hip.so, the MI355X (gfx950) 2-opt local-search engine.
 *
 * This is the drop-in boundary for the heuristics path of deno750/TSP_Optimization.  The
 * reference has no FFI layer; the seam is the set of C functions that its solver dispatch and
 * meta-heuristics call.  Each entry point below names the reference
 * function whose body it replaces.  Host code stays C: it keeps the reference's `instance`
 * struct and calls these functions with the struct's own arrays (see INTEGRATION.md and
 * tsp_optimization_amd/host/).
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no C++/torch types.
 *   - Return value: 0 = ok, 1 = WRONG_STARTING_NODE, 2 = TIME_LIMIT_EXCEEDED (the reference's
 *     include/heuristics.h:6-7); negative = TSP_DEV_E_* (the reference has no such class: its
 *     unrecoverable errors go through LOG_E -> exit(1), include/utility.h:33).
 *   - `xy` is the reference's `point` array: n x {double x, double y} (include/utility.h:126-129),
 *     so `(const double *)inst->nodes` can be passed as is.
 *   - Tours are successor lists.  `succ` + `succ_stride` (in ints) address them: stride 1 for a
 *     plain int array, stride 2 with succ = &inst->solution.edges[0].j for the reference's
 *     `edge {int i; int j;}` array (include/utility.h:134-137).  Batched tours are
 *     `tour_stride` ints apart.
 *   - Weight types are numbered like the reference's enum weight_type (include/utility.h:45-52).
 *   - Nothing here falls back to the CPU: without a usable HIP device every call fails with
 *     TSP_DEV_E_NODEVICE.
 */
#ifndef TSP_HIP_H
#define TSP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* weight types: include/utility.h:45-52 */
enum { TSP_EUC_2D = 0, TSP_MAX_2D = 1, TSP_MAN_2D = 2, TSP_CEIL_2D = 3, TSP_GEO = 4, TSP_ATT = 5 };

/* status codes */
enum {
    TSP_OK = 0,
    TSP_WRONG_STARTING_NODE = 1,  /* include/heuristics.h:6 */
    TSP_TIME_LIMIT_EXCEEDED = 2,  /* include/heuristics.h:7 */
    TSP_DEV_E_NODEVICE = -1,      /* no HIP device / HIP runtime error at init */
    TSP_DEV_E_HIP = -2,           /* a HIP call failed (tsp_dev_last_error() has the text) */
    TSP_DEV_E_ARG = -3,           /* bad argument (NULL, n < 3, unknown mode ...) */
    TSP_DEV_E_NOT_A_TOUR = -4,    /* a successor list is not one Hamiltonian cycle */
    TSP_DEV_E_NOMEM = -5,
    TSP_DEV_E_COMM = -6,          /* RCCL could not be opened or a collective failed (tsp_dev_comm_last_error()) */
    TSP_DEV_E_INTERNAL = -7       /* a device loop ran into its hard cap or a result failed its own check: a defect, not an input */
};

/* 2-opt move selection */
enum {
    TSP_2OPT_FIRST = 0, /* alg_2opt: first improvement in (i<j) node order, applied immediately
                           (src/heuristics.c:438-502) */
    TSP_2OPT_BEST = 1   /* alg_2opt_tabu: best improvement, ties -> first pair (src/tabusearch.c:107-178) */
};

/* constructive heuristics */
enum {
    TSP_CONSTRUCT_GREEDY = 0, /* greedy(): src/heuristics.c:18-78 */
    TSP_CONSTRUCT_GRASP = 1   /* grasp():  src/heuristics.c:82-156 */
};

/* 2-opt execution engine (a performance choice; results are identical) */
enum {
    TSP_ENGINE_AUTO = 0,
    TSP_ENGINE_GRID = 1, /* many workgroups per tour, tour state in HBM, one launch (two for the sorted
                            best-improvement sweep) per step */
    TSP_ENGINE_LDS = 2,  /* one workgroup per tour, whole descent inside one launch, state in LDS */
    TSP_ENGINE_CLUSTER = 3 /* C workgroups per tour (B C <= #CUs), each with a replica of the tour in LDS, whole
                            descent inside one launch; one candidate per workgroup and step exchanged through L2 */
};

typedef struct tsp_dev_ctx tsp_dev_ctx;     /* one device + stream */
typedef struct tsp_dev_inst tsp_dev_inst;   /* node coordinates resident in HBM */
typedef struct tsp_dev_tours tsp_dev_tours; /* B tours of one instance resident in HBM */
typedef struct tsp_dev_tabu tsp_dev_tabu;   /* n(n-1)/2 tabu stamps resident in HBM */
typedef struct tsp_dev_comm tsp_dev_comm;   /* one rank of an RCCL communicator (multi-start across GPUs) */

typedef struct {
    int64_t sweeps;        /* completed passes over the (i<j) pair space                         */
    int64_t evals;         /* delta evaluations the reference would have executed (non-skipped
                              pairs, src/heuristics.c:474 / src/tabusearch.c:150)                */
    int64_t moves;         /* applied 2-opt moves                                                */
    int64_t reversed;      /* tour positions rewritten by segment reversals                      */
    int64_t pairs_scanned; /* pairs the device actually evaluated (>= evals in FIRST mode: a
                              chunk is scanned past the first improving pair)                    */
    int64_t steps;         /* steps: launches of a step kernel (GRID) or chunk iterations (LDS)   */
    double seconds;        /* wall time of the call, host clock                                  */
    double device_ms;      /* device time of the call, HIP events on the engine's stream         */
    /* What the device executed to decide those pairs (the decisions are the reference's; the work is not).  CLUSTER
     * engine: counted; other engines: lane_pairs = pairs_scanned, the rest -1 (not counted).                      */
    int64_t lane_pairs;    /* pairs for which a lane evaluated a lower bound of delta or delta itself             */
    int64_t tier1_pairs;   /* ... that the first bound could not exclude                                           */
    int64_t exact_pairs;   /* delta expressions actually executed (src/heuristics.c:474 / src/tabusearch.c:150)   */
    int64_t staged_recs;   /* node records derived for the sorted scan (one rounded root each)                    */
} tsp_two_opt_stats;

/* ---- context ---------------------------------------------------------------------------- */

/* Opens device `device` (hipSetDevice) and creates the engine's stream. */
int tsp_dev_open(int device, tsp_dev_ctx **out);
void tsp_dev_close(tsp_dev_ctx *ctx);
/* Text of the last failing HIP call on this thread ("" if none). */
const char *tsp_dev_last_error(void);
/* Number of HIP devices visible (0 if none / no runtime).  Does not create a context. */
int tsp_dev_count(void);
int tsp_dev_synchronize(tsp_dev_ctx *ctx);
/* The hipStream_t the engine launches on (as void*), for callers that order work against it. */
void *tsp_dev_stream(tsp_dev_ctx *ctx);

/* ---- instance: replaces the operand side of calc_dist (src/distutil.c:73-92) -------------- */

int tsp_dev_inst_create(tsp_dev_ctx *ctx, const double *xy, int n, int weight_type,
                        int integer_cost, tsp_dev_inst **out);
void tsp_dev_inst_destroy(tsp_dev_inst *inst);
int tsp_dev_inst_size(const tsp_dev_inst *inst);
/* Diagnostics.  The TSP_* environment switches (none changes a result) are read once, when an instance handle is
 * created; tours / tabu handles take theirs from their instance when THEY are created.  This re-reads them for `inst` (tests
 * and measurement scripts that run one form of a kernel against another on the same instance); handles created from it
 * earlier keep what they were created with, except for the cluster / tabu-path choices that are looked up per run. */
int tsp_dev_inst_reload_switches(tsp_dev_inst *inst);

/* calc_dist(i,j) for `count` index pairs, evaluated on the device (parity / spot checks). */
int tsp_dev_dist_pairs(tsp_dev_inst *inst, const int *i, const int *j, int count, double *out);

/* Full n x n matrix of calc_dist (row-major, diagonal 0) -- the north star's "distance-matrix
 * build"; the reference recomputes distances on every call and has no such array.
 * out_host may be NULL (timing only).  Elements are int32 when as_int32 != 0 (valid only with
 * integer costs), else double.  *kernel_ms receives the kernel's device time if not NULL. */
int tsp_dev_dist_matrix(tsp_dev_inst *inst, void *out_host, int as_int32, float *kernel_ms);

/* Self-test: out[k] = the hardware's approximate v_sqrt_f64(in[k]).  The exact integer-root
 * variants used for integer coordinates rely on its error bound; tests measure it through this. */
int tsp_dev_selftest_raw_sqrt(tsp_dev_ctx *ctx, const double *in, int count, double *out);

/* ---- construction: greedy() / grasp() for B starting nodes at once ------------------------ */
/* kind = TSP_CONSTRUCT_*.  starts[B].  urand: B x n doubles in [0,1], the values URAND()
 * (include/utility.h:36) would return for start b, in draw order (grasp draws exactly n per
 * call, src/heuristics.c:127); ignored for greedy.  Outputs: successor lists and obj (obj is
 * the reference's reported value, i.e. GRASP's closing edge counted twice, :135,:152).
 * status_out[B] (may be NULL) receives 0 or TSP_WRONG_STARTING_NODE per start. */
int tsp_dev_construct(tsp_dev_inst *inst, int kind, int B, const int *starts, const double *urand,
                      int *succ, int succ_stride, int64_t tour_stride, double *obj, int *status_out);

/* One line of text in buf naming the kernel (and its variant) that tsp_dev_construct launches for this instance and kind under the
 * switches the instance was created with: "k_construct_nn<float2, packed>", "k_construct_nn_big<double2, generic>",
 * "k_construct_lds", "k_construct" (tests check that an input reached the path they mean to test). */
int tsp_dev_construct_describe(tsp_dev_inst *inst, int kind, char *buf, int cap);

/* HEU_extramileage (src/heuristics.c:208-314): farthest pair, then cheapest insertion of every other
 * node; writes the successor list and the reference's obj (2*d(A,B) + the sum of the extra mileages). */
int tsp_dev_extramileage(tsp_dev_inst *inst, int *succ, int succ_stride, double *obj);

/* ---- 2-opt on host-resident tours: replaces alg_2opt / alg_2opt_tabu(skip_edge==NULL) ------ */
/* B tours in/out.  obj[B] in/out: FIRST adds the applied deltas to the incoming value like
 * `obj_best += delta` (src/heuristics.c:486); BEST overwrites it with the recomputed tour cost
 * (src/tabusearch.c:168-172).  time_limit_s <= 0 = unlimited.  stats may be NULL, else B entries. */
int tsp_dev_two_opt(tsp_dev_inst *inst, int mode, int engine, int B, int *succ, int succ_stride,
                    int64_t tour_stride, double *obj, double time_limit_s, tsp_two_opt_stats *stats);

/* ---- tabu stamps + alg_2opt_tabu with skip_edge != NULL (src/tabusearch.c:107-178) --------- */
int tsp_dev_tabu_create(tsp_dev_inst *inst, tsp_dev_tabu **out); /* all stamps 0 (CALLOC, :195) */
void tsp_dev_tabu_destroy(tsp_dev_tabu *tabu);
/* stamps[idx[k]] = value[k]; idx = x_udir_pos(i,j,n) (src/utility.c:17-30), as :306-309 */
int tsp_dev_tabu_set(tsp_dev_tabu *tabu, const int *idx, const int *value, int count);
int tsp_dev_tabu_get(tsp_dev_tabu *tabu, const int *idx, int *value, int count);
int tsp_dev_tabu_upload(tsp_dev_tabu *tabu, const int *stamps);   /* n(n-1)/2 ints */
int tsp_dev_tabu_download(tsp_dev_tabu *tabu, int *stamps);
/* Diagnostics of the handle's compact list of non-zero stamps, from which runs with a list work (a few hundred entries
 * of the reference's n(n-1)/2, :195): *entries = upper bound of its length, or -1 while it is out of date (the host
 * wrote stamps; the next run scans); *used_by_last_run = 1 when the last alg_2opt_tabu call worked from the list, 0
 * when it read the stamps pair by pair (list too long, tour outside the sorted sweep).  Either may be NULL. */
int tsp_dev_tabu_list_info(tsp_dev_tabu *tabu, int *entries, int *used_by_last_run);
/* One call of alg_2opt_tabu(inst, skip_edge, stored_prev, iter, tenure) on one tour.
 * stored_prev (may be NULL) receives the predecessor array (:173-175). */
int tsp_dev_two_opt_tabu(tsp_dev_inst *inst, tsp_dev_tabu *tabu, int iter, int tenure, int *succ,
                         int succ_stride, double *obj, int *stored_prev, double time_limit_s,
                         tsp_two_opt_stats *stats);

/* ---- tour cost: fitness() for B permutations (src/genetic.c:51-60) ------------------------- */
int tsp_dev_perm_cost(tsp_dev_inst *inst, int B, const int *perm, int64_t perm_stride, double *cost);

/* ---- device-resident tours (what bench.py times: inputs already in HBM) -------------------- */
int tsp_dev_tours_create(tsp_dev_inst *inst, int B, tsp_dev_tours **out);
void tsp_dev_tours_destroy(tsp_dev_tours *t);
/* Upload B successor lists (+ their obj values) and remember them as the reset point. */
int tsp_dev_tours_upload(tsp_dev_tours *t, const int *succ, int succ_stride, int64_t tour_stride,
                         const double *obj);
/* Restore the uploaded tours on the device (device-to-device). */
int tsp_dev_tours_reset(tsp_dev_tours *t);
int tsp_dev_tours_download(tsp_dev_tours *t, int *succ, int succ_stride, int64_t tour_stride,
                           double *obj, tsp_two_opt_stats *stats);
/* Run at most max_steps GRID-engine steps (one step = one scan of the selection rule's range and at
 * most one move per tour) in `mode`; max_steps < 0 = until every tour is at its local optimum (needs sync != 0:
 * an unbounded run without polls is refused with TSP_DEV_E_ARG).
 * Does not wait for completion unless `sync` != 0.  *all_done (if not NULL, sync only). */
int tsp_dev_tours_run(tsp_dev_tours *t, int mode, int64_t max_steps, double time_limit_s, int sync,
                      int *all_done);
/* The same on a chosen engine (TSP_ENGINE_*), always waiting for completion: device-resident tours run to their
 * local optima (or for at most max_steps steps per tour when max_steps >= 0; not with TSP_ENGINE_LDS).  A capped or
 * timed-out best-improvement run leaves the recomputed cost in obj like a finished one (src/tabusearch.c:168-172).
 * TSP_ENGINE_AUTO picks CLUSTER where it applies, else GRID. */
int tsp_dev_tours_run_engine(tsp_dev_tours *t, int mode, int engine, int64_t max_steps, double time_limit_s,
                             int *all_done);
/* ---- drivers on resident tours: what tabu() (src/tabusearch.c:188-320) and HEU_VNS (src/vns.c:103-166) do between two
 * 2-opt calls, on the device, so that an iteration moves no tour and no stamp across PCIe ------------------------------ */
/* alg_2opt / alg_2opt_tabu(NULL) on the tours as they are: the cursor starts a new sweep, obj_best continues (FIRST adds its
 * deltas to the value the control block holds, src/heuristics.c:442,486).  obj[B] (may be NULL) receives the result. */
int tsp_dev_tours_two_opt(tsp_dev_tours *t, int mode, int engine, double time_limit_s, double *obj);
/* One alg_2opt_tabu(inst, skip_edge, prev, iter, tenure) on resident tour 0 with resident stamps (B == 1). */
int tsp_dev_tours_two_opt_tabu(tsp_dev_tours *t, tsp_dev_tabu *tabu, int iter, int tenure, double time_limit_s, double *obj);
/* One trial of tabu()'s kick (src/tabusearch.c:262-309) with the host-drawn nodes a, b: rejected if the two edges share a
 * node or one of (a,a1) (b,b1) (a,b) (a1,b1) is in the tabu list (check_tenure with its lazy clears, in that order); else
 * the 2-exchange is carried out and (a,a1), (b,b1) are stamped with iter.  *accepted = 1 / 0. */
int tsp_dev_tours_tabu_kick(tsp_dev_tours *t, tsp_dev_tabu *tabu, int a, int b, int iter, int tenure, int *accepted);
/* One iteration of tabu() (src/tabusearch.c:238-309) in one wait for the device (two when the descent does not finish in the
 * CLUSTER engine's first launch): alg_2opt_tabu on resident tour 0; if its
 * cost is below *best_obj the tour becomes the incumbent (as tsp_dev_tours_snapshot; *best_obj updated, *improved = 1,
 * :241-249); then ONE trial of the kick with the host-drawn a, b (as tsp_dev_tours_tabu_kick; *accepted) -- further
 * trials, if that one is rejected, go through tsp_dev_tours_tabu_kick.  Returns the run's status; with a time limit hit
 * no kick is made (:255-258).  obj / improved / accepted may be NULL. */
int tsp_dev_tours_tabu_iteration(tsp_dev_tours *t, tsp_dev_tabu *tabu, int iter, int tenure, double time_limit_s, int a, int b,
                                 double *best_obj, double *obj, int *improved, int *accepted);
/* `count` (<= 128) iterations of tabu() in ONE wait for the device: iteration iter0 + k runs alg_2opt_tabu with tenure[k], updates
 * the incumbent and makes the FIRST trial of its kick with the host-drawn nodes ab[2k], ab[2k + 1] (what
 * tsp_dev_tours_tabu_iteration does for one iteration) -- the iterations run inside one launch of the CLUSTER engine (or, TSP_TABU_INKERNEL=0, as launches queued back
 * to back) and a word on the device stops the chain as soon as an iteration cannot be completed there.  *completed = iterations that ran up to their kick's trial; obj[k] /
 * improved[k] are filled for those.  *last_accepted = 0: the trial of iteration iter0 + *completed - 1 was rejected (edges that
 * share a node, or tabu): the caller draws further trials for it (tsp_dev_tours_tabu_kick) and goes on; the pairs ab[2k ..] of
 * the iterations that did not run have not been consumed (the caller serves them first: the libc stream stays the
 * reference's).  An iteration whose descent did not finish inside its launch (or whose exchange gave up) is not counted: the
 * caller runs it through tsp_dev_tours_tabu_iteration with its own a, b.  *completed = 0 with return 0: the chain does not
 * apply here (another engine, a list too long for it); nothing was touched. */
int tsp_dev_tours_tabu_iterations(tsp_dev_tours *t, tsp_dev_tabu *tabu, int iter0, int count, const int *tenure, const int *ab,
                                  double time_limit_s, double *best_obj, double *obj, int *improved, int *completed, int *last_accepted);
/* The same with the kick's FURTHER trials on the device too (src/tabusearch.c:262-287 draws pairs until one is accepted): ab holds
 * `pairs` (count <= pairs <= 256) node pairs in the order tabu() would draw them, and the iterations take them in that order --
 * iteration iter0 + k starts with the pair after the last one iteration iter0 + k - 1 took, and a rejected trial is followed by
 * the next pair, all inside the launch (the CLUSTER engine's tabu variant runs the iterations itself: incumbent, trials, kick
 * and the next descent on the replicas).  trials[k] = pairs iteration k took (0 when the earlier iterations had used them all up: no trial was made); the caller has consumed
 * sum(trials[0 .. *completed - 1]) pairs and serves the rest of its look-ahead first.  *last_accepted = 0 only when the pairs ran
 * out in the middle of an iteration's trials: the caller draws on (tsp_dev_tours_tabu_kick).  Everything else as above.  Where
 * the iterations cannot run inside a launch (TSP_TABU_INKERNEL=0, another engine) *completed = 0 and the caller takes
 * tsp_dev_tours_tabu_iterations. */
int tsp_dev_tours_tabu_iterations_ex(tsp_dev_tours *t, tsp_dev_tabu *tabu, int iter0, int count, const int *tenure, int pairs, const int *ab,
                                     double time_limit_s, double *best_obj, double *obj, int *improved, int *trials, int *completed,
                                     int *last_accepted);
/* kick() of src/vns.c:11-100 with the three host-drawn, sorted tour positions p1 < p2 < p3 (positions of the walk from
 * node 0): segments tour[p1+1..p2] and tour[p2+1..p3] swap places; the recomputed cost (:77-86) goes to the control block
 * and to *obj (may be NULL). */
int tsp_dev_tours_vns_kick(tsp_dev_tours *t, int p1, int p2, int p3, double *obj);
/* Page-lock / release a caller's host array that is passed to the library again and again (uploads at PCIe speed). */
int tsp_dev_host_register(void *p, size_t bytes);
int tsp_dev_host_unregister(void *p);
/* Incumbent on the device: remember the current tours + costs / go back to them (src/vns.c:148-158, tabusearch.c:241-249). */
int tsp_dev_tours_snapshot(tsp_dev_tours *t);
int tsp_dev_tours_restore(tsp_dev_tours *t);
/* Launch `reps` best-improvement steps back to back on the current tours (they continue the descent)
 * with HIP events around the run on the engine's stream; returns the mean duration of a step's
 * launches in *mean_ms and the reference-equivalent evaluations per step in *evals_per_launch.
 * Roofline measurement. */
int tsp_dev_tours_time_scan(tsp_dev_tours *t, int reps, float *mean_ms, int64_t *evals_per_launch);
/* Device time of the last tsp_dev_tours_run_engine / tsp_dev_tours_two_opt on this handle (HIP events on the engine's stream
 * around the run; the same value tsp_dev_tours_download reports as stats.device_ms), without a copy or a wait. */
int tsp_dev_tours_device_ms(tsp_dev_tours *t, double *ms);
/* Diagnostics: the kernels one GRID-engine step of `mode` launches for this handle, as text (bench.py names the kernel its
 * roofline describes from this; tests check that a switch selected the path they mean to test). */
int tsp_dev_tours_describe(tsp_dev_tours *t, int mode, char *buf, int cap);
/* Diagnostics: the LDS engine's kernel body for this instance and `mode`, as one line of text such as
 *   k_lds_two_opt<EUC_2D_ICOORD, FIRST, cache=1, f32=1> lds=63120 of 163840
 * -- the metric variant, the rule, whether the edge-length cache and the fp32 first tier are compiled in (TSP_LDS_EDGE_CACHE,
 * TSP_LDS_F32_MIN_N and the fit of the cache decide, as they stood when the handle was created), the dynamic LDS a launch asks
 * for and the LDS a workgroup may be granted.  TSP_DEV_E_ARG when the instance does not fit the LDS engine at all.  Tests check
 * with it that a switch selected the body they mean to test. */
int tsp_dev_inst_lds_variant(tsp_dev_inst *inst, int mode, char *buf, int cap);
/* min over tours of (cost, tour index) packed as (int64(cost) << 24 | index); the value the
 * multi-start all-reduce(min) combines across ranks.  true_cost != 0 recomputes the cost from
 * the tour (GRASP's reported value carries an offset).  Written to *packed. */
int tsp_dev_tours_best(tsp_dev_tours *t, int true_cost, int64_t *packed);


/* ---- multi-start across the GPUs of a node: generalises HEU_Grasp_iter's "keep the best start"
 * (src/heuristics.c:510-544, :534-539) to starts sharded k % world over the ranks.  The path shards across tours only, so
 * the whole exchange is ONE RCCL all-reduce(min) of the packed (cost << 24 | start id) and ONE broadcast of the winner's
 * successor list (4n bytes) from the rank that owns it.  librccl is dlopen()ed by the first of these calls; errors of this
 * group return TSP_DEV_E_COMM with the text in tsp_dev_comm_last_error(). ------------------------------------------------ */
#define TSP_COMM_ID_BYTES 128
const char *tsp_dev_comm_last_error(void);
/* 1 if librccl could be opened (dlopen) and holds every symbol this group needs, else 0.  Forms no communicator: a rank can
 * ask before it enters the collective tsp_dev_comm_init_rank, in which a rank that cannot load RCCL would leave the others waiting. */
int tsp_dev_comm_available(void);
/* One process per GPU: rank 0 obtains the id (ncclGetUniqueId) and hands its TSP_COMM_ID_BYTES to every rank by a side
 * channel of the caller's choice; then every rank calls init_rank with its own context (collective: returns when all have). */
int tsp_dev_comm_unique_id(char *id);
int tsp_dev_comm_init_rank(tsp_dev_ctx *ctx, int world, int rank, const char *id, tsp_dev_comm **out);
/* One process, ndev devices (ncclCommInitAll): out[k] is rank k on ctxs[k]'s device; use the *_group calls below. */
int tsp_dev_comm_init_all(tsp_dev_ctx *const *ctxs, int ndev, tsp_dev_comm **out);
void tsp_dev_comm_destroy(tsp_dev_comm *comm);
int tsp_dev_comm_info(const tsp_dev_comm *comm, int *rank, int *world, int *rccl_version);
/* (cost, start id) -> the int64 whose minimum is (lowest cost, then lowest start id): cost << 24 | start_id.  Costs that
 * are not non-negative integers below 2^39 (--fcost, GEO) cannot be packed: TSP_DEV_E_ARG, nothing is written. */
int tsp_dev_multistart_pack(double cost, int start_id, int64_t *packed);
/* all-reduce(min) of one int64 per rank over RCCL; every rank receives the minimum. */
int tsp_dev_multistart_allreduce(tsp_dev_comm *comm, int64_t packed_local, int64_t *packed_best);
/* all-reduce(min) of one double per rank: the first of the TWO reductions that carry costs the packed word cannot (--fcost,
 * src/utility.c:285; `< bestobj` on doubles, src/heuristics.c:534) -- min of the cost, then tsp_dev_multistart_allreduce of the
 * start id among the ranks whose cost equals that minimum (ties -> lowest start, the strict `<` in stream order). */
int tsp_dev_multistart_allreduce_f64(tsp_dev_comm *comm, double cost_local, double *cost_best);
/* Every collective of this group waits at most TSP_COMM_TIMEOUT_S (300) seconds for its peers; after that the communicator is
 * aborted and the call returns TSP_DEV_E_COMM (RCCL itself would wait for ever for a rank that died before the collective). */
/* broadcast of n ints (a successor list, `succ_stride` ints apart: 2 for &inst->solution.edges[0].j) from rank `root`. */
int tsp_dev_multistart_bcast_tour(tsp_dev_comm *comm, int root, int *succ, int succ_stride, int n);
/* The same two collectives for all ndev communicators of ONE process (ncclGroupStart / ncclGroupEnd around them).
 * packed_local[k] / packed_best[k] belong to rank k; the tour travels from rank `root`'s device to every device and is
 * read back from `read_back_rank`'s (so that a caller can check what a non-root rank received). */
int tsp_dev_multistart_allreduce_group(tsp_dev_comm *const *comms, int ndev, const int64_t *packed_local, int64_t *packed_best);
int tsp_dev_multistart_allreduce_f64_group(tsp_dev_comm *const *comms, int ndev, const double *cost_local, double *cost_best);
int tsp_dev_multistart_bcast_tour_group(tsp_dev_comm *const *comms, int ndev, int root, const int *succ_root, int succ_stride,
                                        int n, int read_back_rank, int *succ_out);

/* ---- Or-opt (extension; the reference declares HEU_3opt, include/heuristics.h:51-56, and never defines it) ------------------
 * A move takes a segment f -> .. -> l of L = 1..3 nodes (p = pred f, s = succ l) out of the tour and puts it between a and
 * b = succ a, a not in {p, f .. l}, forward (a f .. l b) or reversed (a l .. f b; L > 1):
 *     delta = ((d(a,f) + d(l,b)) - d(a,b)) - ((d(p,f) + d(l,s)) - d(p,s))      [reversed: (d(a,l) + d(f,b)) in the first bracket]
 * Each decision takes the improving move (delta < 0) of smallest delta, ties -> smallest key ((f*3 + L-1)*n + a)*2 + o
 * (o = 1 reversed; node ids).  n(5n - 16) moves per decision; n < 5 returns TSP_OK with the tours unchanged. */
typedef struct {
    int64_t sweeps;          /* decisions taken: moves + the last one, which found no improving move                    */
    int64_t evals;           /* sum of n(5n - 16) over the decisions (the logical count, as tsp_two_opt_stats.evals)     */
    int64_t moves;           /* applied Or-opt moves                                                                     */
    int64_t moves_by_len[3]; /* ... of segments of 1, 2, 3 nodes                                                         */
    int64_t moves_reversed;  /* ... that inserted the segment reversed                                                   */
    int64_t deltas_executed; /* delta expressions the device actually ran (a full scan per decision, or the incremental
                                path: the rows a move touched rescanned, every other row checked on the new edges); a
                                full scan's count includes the lanes that own no row: about 1.04 x n(5n - 16)           */
    int64_t rounds;          /* tsp_dev_two_opt_or_opt: 2-opt + Or-opt rounds; 0 from tsp_dev_or_opt                     */
    double seconds;          /* wall time of the call, host clock                                                        */
    double device_ms;        /* device time of the call, HIP events on the engine's stream                               */
} tsp_or_opt_stats;

/* Or-opt descent (best improvement, as above) of B tours until no move improves or max_moves moves (max_moves < 0:
 * unlimited).  obj[B] out: the recomputed cost of the final tour (as tsp_dev_two_opt's BEST mode leaves it), not a sum of
 * deltas.  time_limit_s <= 0 = unlimited; on expiry TSP_TIME_LIMIT_EXCEEDED with the tours as they stand (valid) and their
 * costs.  stats may be NULL, else B entries. */
int tsp_dev_or_opt(tsp_dev_inst *inst, int B, int *succ, int succ_stride, int64_t tour_stride,
                   double *obj, int64_t max_moves, double time_limit_s, tsp_or_opt_stats *stats);
/* 2-opt + Or-opt: per tour, tsp_dev_two_opt(two_opt_mode, TSP_ENGINE_AUTO) then an Or-opt descent, repeated until an Or-opt
 * descent makes no move; the result is a local optimum of both neighbourhoods.  obj[B] in/out (in: as tsp_dev_two_opt
 * takes it; out: the recomputed cost).  One time budget over all phases.  The stats (NULL, or B entries each) sum the
 * phases of each tour; or_opt_stats[b].rounds = rounds. */
int tsp_dev_two_opt_or_opt(tsp_dev_inst *inst, int two_opt_mode, int B, int *succ, int succ_stride,
                           int64_t tour_stride, double *obj, double time_limit_s,
                           tsp_two_opt_stats *two_opt_stats, tsp_or_opt_stats *or_opt_stats);

/* ---- candidate neighbour lists (extension): a 2-opt + Or-opt descent over the moves that use an edge of the lists --------------
 * (A decision scans O(n K) moves and applies one in O(n) on one compute unit; DESIGN.md 4.11 has the measured times beside
 * tsp_dev_two_opt_or_opt's.)
 * Lists.  For 1 <= K <= min(TSP_NL_MAX_K, n - 1), nbr[v][0 .. K-1] are the K nodes u != v smallest by (calc_dist(v, u), u), in
 * that order: the instance's own distance (the value tsp_dev_dist_pairs returns), ties -> lower node id, coincident nodes are
 * neighbours at distance 0.  N(v) is the set; u ~ v when u in N(v) or v in N(u).  A caller's own lists may be any n x K array
 * with entries in [0, n) other than v itself; duplicates are allowed, only the set matters.
 * Moves.  kind 0, 2-opt: node pairs i < j with i1 = succ i, j1 = succ j, skipped when j = i1 or j1 = i;
 *     delta = ((d(i,j) + d(i1,j1)) - d(i,i1)) - d(j,j1)   (alg_2opt_tabu's), key = i * n + j;
 * in the list neighbourhood iff i ~ j or i1 ~ j1; applied as alg_2opt_tabu applies it (succ i = j, succ i1 = j1, the forward path
 * i1 .. j reversed).  kind 1, Or-opt: the moves (f, L, a, o) of tsp_dev_or_opt with their delta and key; in the list
 * neighbourhood iff, for o = 0, a ~ f or l ~ b, and for o = 1, a ~ l or f ~ b; applied as tsp_dev_or_opt applies them.
 * Decision.  Among the enabled kinds the move of smallest delta < 0, ties -> lower kind, then lower key; one move per decision.
 * The descent ends at the first decision without an improving move, after max_moves moves or at the time limit.  A kind that has
 * no move at the instance's size (2-opt: n < 4, Or-opt: n < 5) is left out; with none left the tours come back unchanged.
 * With K = n - 1 kind 0 alone follows alg_2opt_tabu(NULL) and kind 1 alone follows tsp_dev_or_opt. */
enum { TSP_NL_2OPT = 1, TSP_NL_OROPT = 2 }; /* kinds mask */
#define TSP_NL_MAX_K 16
#define TSP_NL_DEFAULT_K 10
/* The lists live in the instance handle.  Bad K or bad entries: TSP_DEV_E_ARG, and the lists the handle had stay in place. */
int tsp_dev_inst_knn_build(tsp_dev_inst *inst, int K, float *kernel_ms); /* exact, on the device; kernel_ms may be NULL */
int tsp_dev_inst_knn_set(tsp_dev_inst *inst, int K, const int *nbr);     /* the caller's n x K lists, validated        */
int tsp_dev_inst_knn_get(tsp_dev_inst *inst, int *K, int *nbr);          /* nbr may be NULL: K only (0 = no lists)     */
typedef struct {
    int64_t decisions;       /* decisions taken: moves + the last one, if it found no improving move                     */
    int64_t moves;           /* applied moves                                                                            */
    int64_t moves_2opt;      /* ... of kind 0                                                                            */
    int64_t moves_oropt;     /* ... of kind 1                                                                            */
    int64_t moves_by_len[3]; /* Or-opt moves of segments of 1, 2, 3 nodes                                                */
    int64_t moves_reversed;  /* Or-opt moves that inserted the segment reversed                                          */
    int64_t reversed;        /* successors rewritten by the 2-opt moves' reversals of the forward path i1 .. j (the
                                reference's count, tsp_two_opt_stats.reversed)                                           */
    int64_t deltas_executed; /* delta expressions the device ran (a move is reached through several list entries)        */
    double seconds;          /* wall time of the call, host clock                                                        */
    double device_ms;        /* device time of the call, HIP events on the engine's stream                               */
} tsp_nl_opt_stats;
/* Descent over the list neighbourhood of B tours (kinds: TSP_NL_2OPT | TSP_NL_OROPT, at least one).  Without lists in the
 * handle it builds them with K = min(TSP_NL_DEFAULT_K, n - 1).  obj[B] out: the recomputed cost of the final tour.  max_moves,
 * time_limit_s, the status and stats as tsp_dev_or_opt. */
int tsp_dev_nl_opt(tsp_dev_inst *inst, int kinds, int B, int *succ, int succ_stride, int64_t tour_stride,
                   double *obj, int64_t max_moves, double time_limit_s, tsp_nl_opt_stats *stats);

/* ---- candidate-list 3-opt (extension): the general segment move as a third kind of the list descent -------------------------
 * (The reference declares HEU_3opt, include/heuristics.h:51-56, and never defines it; Or-opt above is the case of a segment of
 * at most 3 nodes.  DESIGN.md 4.14 has the kernels.)
 * Labels.  Three distinct tour edges are removed, named by their tails a, b, c with heads a1 = succ a, b1 = succ b, c1 = succ c:
 * a is the tail with the lowest node id, b and c follow a in tour order.  Segments S1 = a1 .. b, S2 = b1 .. c, S3 = c1 .. a; a
 * segment may be one node.
 * Types.  The four pure reconnections, new edges (e1, e2, e3) and the new tour from a (S3 always keeps its direction):
 *     0: (a,b1) (c,a1) (b,c1)   a, S2, S1, c1 ..                     1: (a,b) (a1,c) (b1,c1)   a, S1 reversed, S2 reversed, c1 ..
 *     2: (a,c) (b1,a1) (b,c1)   a, S2 reversed, S1, c1 ..            3: (a,b1) (c,b) (a1,c1)   a, S2, S1 reversed, c1 ..
 * (a, b, c, type) is a move iff none of its three new edges is an edge of the current tour (that leaves out the reconnections
 * that are 2-opt moves because two removed edges are adjacent): 2n(n-2)(n-4)/3 moves per tour, none for n < 5.  A move with a
 * segment of one node has the same new edges as a second type (the one that reverses that segment); both are moves.
 *     delta = ((d(e1) + d(e2)) + d(e3)) - ((d(a,a1) + d(b,b1)) + d(c,c1)), every d with the lower node id first, evaluated in
 * exactly this order;  key = ((a*n + b)*n + c)*4 + type.
 * List neighbourhood.  A move is in it iff it has a removed edge (p, q = succ p) and two different new edges {p,u} and {q,w} with
 * u in N(p) and w in N(q): the lists as stored, directed, without the closure u ~ v of the two kinds above (LKH's step
 * t2 -> t3, t4 -> t5 without the gain rule).  With K = n - 1 every move is in it.
 * Apply.  The new tour of the table in forward orientation; order/pos by at most three reversals of forward paths.
 * Decision.  As above over the enabled kinds: smallest delta < 0, ties -> lower kind (2-opt 0, Or-opt 1, 3-opt 2), then lower
 * key.  The key takes 4n^3 below the kind bits: with TSP_NL_3OPT enabled, n > 2^20 is TSP_DEV_E_ARG. */
enum { TSP_NL_3OPT = 4 }; /* kinds mask of tsp_dev_nl_3opt, beside TSP_NL_2OPT and TSP_NL_OROPT */
typedef struct {
    int64_t decisions, moves, moves_2opt, moves_oropt, moves_by_len[3], moves_reversed, reversed, deltas_executed;
    double seconds, device_ms; /* the fields of tsp_nl_opt_stats, in its layout; moves and deltas_executed count all kinds */
    int64_t moves_3opt;        /* applied moves of kind 2                                                                  */
    int64_t moves_by_type[4];  /* ... of types 0 .. 3                                                                      */
} tsp_nl3_opt_stats;
/* tsp_dev_nl_opt with the third kind: kinds is any non-empty subset of TSP_NL_2OPT | TSP_NL_OROPT | TSP_NL_3OPT (tsp_dev_nl_opt
 * keeps refusing TSP_NL_3OPT); the 3-opt kind has no move for n < 5 and is then left out.  Lists, the default lists, obj,
 * max_moves, time_limit_s and the status as there.  With kinds inside TSP_NL_2OPT | TSP_NL_OROPT it follows tsp_dev_nl_opt move
 * for move. */
int tsp_dev_nl_3opt(tsp_dev_inst *inst, int kinds, int B, int *succ, int succ_stride, int64_t tour_stride,
                    double *obj, int64_t max_moves, double time_limit_s, tsp_nl3_opt_stats *stats);

/* ---- iterated local search (extension): double-bridge kicks and the list descent above, B independent chains ----------------
 * (DESIGN.md 4.15 has the kernels.)  All integer arithmetic below is unsigned and mod 2^64.
 * Random stream.  Counter based: no state, and libc's random() is not touched.
 *     mix(x):  x += 0x9E3779B97F4A7C15;  z = x;  z = (z ^ z>>30) * 0xBF58476D1CE4E5B9;  z = (z ^ z>>27) * 0x94D049BB133111EB;
 *              return z ^ z>>31                                                              (the splitmix64 step)
 * The draws of chain b at iteration it are  u_j = mix(mix(mix(seed ^ (b * 0x100000001B3)) + it) + j),  j = 0 .. 4.  They are
 * reduced with plain %: the modulo bias (below n / 2^64) is accepted.
 * Kick(it, span), n >= 8.  W = n when span <= 0, else min(span, n); a span of 1 .. 7 is TSP_DEV_E_ARG.  s = u_0 % n,
 * seq[0] = s, seq[k+1] = succ seq[k];
 *     o1 = 1 + u_1 % (W - 3),  o2 = o1 + 1 + u_2 % (W - 2 - o1),  o3 = o2 + 1 + u_3 % (W - 1 - o2),  o4 = o3 + 1 + u_4 % (W - o3),
 * so 1 <= o1 < o2 < o3 < o4 <= W.  With P = seq[0:o1], Bk = seq[o1:o2], Ck = seq[o2:o3], Dk = seq[o3:o4], R = seq[o4:n] (may be
 * empty) the new tour is P Dk Ck Bk R, every block in its old direction, closed back to seq[0]: exactly four successors change,
 * those of the last nodes of P, Bk, Ck and Dk (the double bridge; A C B D over three cuts is a 3-opt move of type 0 and is not
 * meant).  As undirected edges that is four out and four in, less one for every two single-node blocks that are neighbours on
 * the cycle (R P), Bk, Ck, Dk.  All of it lies within W nodes of s.
 * Chain b, given iterations I >= 0 and a cap M of moves per descent (M < 0: none):
 *   1. the tsp_dev_nl_3opt descent of the caller's tour b over `kinds`, ended after M moves: the incumbent;
 *   2. c* = the incumbent's recomputed cost (the sum over nodes in node order that every obj of this section is);
 *   3. for it = 0 .. I-1: work = kick(incumbent); the descent of work as in 1; c = its recomputed cost; work becomes the
 *      incumbent, and c* = c, iff c < c*;
 *   4. the incumbent and c* are returned: never a tour in the middle of a descent.
 * n < 8 has no kick: the call is step 1 alone and reports iterations = 0.
 * Time limit.  TSP_TIME_LIMIT_EXCEEDED; the unfinished iteration is discarded and stats.iterations counts the completed ones, so
 * a call without a limit and with iterations = that count returns the same tour and cost.  Until step 1 has ended the incumbent
 * is the caller's tour, and that is what a limit so short returns (start_cost = its cost).  The counters of the discarded
 * descent stay in the sums. */
typedef struct {
    int64_t decisions, moves, moves_2opt, moves_oropt, moves_by_len[3], moves_reversed, reversed, deltas_executed;
    double seconds, device_ms;
    int64_t moves_3opt, moves_by_type[4]; /* tsp_nl3_opt_stats, in its layout: the sums over all descents of the chain          */
    int64_t iterations;    /* completed iterations (kick, descent, accept or reject)                                           */
    int64_t accepted;      /* ... whose tour became the incumbent                                                              */
    int64_t last_improved; /* the last of those, or -1                                                                         */
    double start_cost;     /* c* after step 1                                                                                  */
} tsp_ils_stats;
/* B chains, chain b from tour b with stream b.  kinds, the lists and the default lists as tsp_dev_nl_3opt.  obj[B] out: c*.
 * Bad arguments (also iterations < 0, a span of 1 .. 7): TSP_DEV_E_ARG, and the caller's tours are untouched. */
int tsp_dev_ils(tsp_dev_inst *inst, int kinds, int B, int *succ, int succ_stride, int64_t tour_stride, double *obj,
                uint64_t seed, int64_t iterations, int span, int64_t max_moves_per_descent, double time_limit_s,
                tsp_ils_stats *stats);
/* The kick of iteration `it` (>= 0) of chain b applied to tour b, b = 0 .. B-1, and nothing else: the perturbation for a
 * caller's own loop.  n < 8, it < 0 or a span of 1 .. 7: TSP_DEV_E_ARG. */
int tsp_dev_ils_kick(tsp_dev_inst *inst, int B, int *succ, int succ_stride, int64_t tour_stride, uint64_t seed, int64_t it,
                     int span);

/* ---- don't-look bits (extension; Bentley, Johnson & McGeoch, LKH): the list descent and the chains over an active set -------
 * (DESIGN.md 4.16 has the kernels.)  A new descent rule behind new entry points: it takes other decisions than the full scan
 * of tsp_dev_nl_3opt, which keeps its trajectory, as does tsp_dev_ils.
 * Candidates of a node v, cand(v): the moves of the list neighbourhood that v's own list entries (v, u), u = nbr[v][k], generate.
 *     2-opt:  the moves with a new edge {v, u}: {i, j} = {v, u} or {i1, j1} = {v, u};
 *     Or-opt: the moves one of whose two attaching edges is {v, u};
 *     3-opt:  the moves with a removed edge (v, q = succ v) and new edges {v, u} and {q, w}, w in q's stored list.
 * The union of cand(v) over all v is the neighbourhood of tsp_dev_nl_3opt.  Deltas, keys, the order (delta, kind, key) and the way
 * a move is applied are those of tsp_dev_nl_3opt.
 * Decision with active set A (one set per tour).  For v in A, m_v = the best of cand(v), or none; m = the best of all m_v.  Every
 * decision counts in `decisions`.
 *   - m.delta < 0: m is applied and A becomes {v in A : m_v.delta < 0} + ends(m), where ends(m) are the tails and heads of the
 *     edges m removes, in the tour before the move: i, i1, j, j1 (2-opt); pred f, f, l, succ l, a, b (Or-opt); a, a1, b, b1, c, c1
 *     (3-opt).
 *   - otherwise, mode TSP_DLB_ON: the descent ends.
 *   - otherwise, mode TSP_DLB_CLOSE: if A was all of V at this decision's start the descent ends; else A becomes V,
 *     closing_scans += 1 and the descent goes on.  So a TSP_DLB_CLOSE result is a local optimum of the whole list neighbourhood.
 * max_moves and the time limit work as in tsp_dev_nl_3opt.
 * Start.  A = V, or the caller's set: `active`, B x n bytes, non-zero = active, NULL = all.  An empty set is allowed: mode
 * TSP_DLB_ON then takes one decision and ends, mode TSP_DLB_CLOSE goes to A = V.
 * Chains.  Step 1 of a chain starts with A = V.  Every kick sets A to exactly the tails and heads of its four removed edges and
 * clears everything else, also what a descent ended by the cap M left active: with seq the sequence of the kick's definition
 * before the kick, seq[o1-1], seq[o1], seq[o2-1], seq[o2], seq[o3-1], seq[o3], seq[o4-1], seq[o4 mod n]: at most eight nodes,
 * fewer when blocks are single nodes.  Accept and reject, the random stream and the time-limit rules are those of tsp_dev_ils.
 * Mode TSP_DLB_OFF is the full scan: the entry points below then follow tsp_dev_nl_3opt / tsp_dev_ils move for move, ignore
 * `active` and report active_nodes = closing_scans = 0.  The result does not depend on the order in which a set is stored: two
 * runs return the same bits. */
enum { TSP_DLB_OFF = 0, TSP_DLB_ON = 1, TSP_DLB_CLOSE = 2 };
typedef struct {
    int64_t decisions, moves, moves_2opt, moves_oropt, moves_by_len[3], moves_reversed, reversed, deltas_executed;
    double seconds, device_ms;
    int64_t moves_3opt, moves_by_type[4]; /* tsp_nl3_opt_stats, in its layout                                                   */
    int64_t active_nodes;   /* sum of |A| at the start of every decision                                                        */
    int64_t closing_scans;  /* times A was reset to V (mode TSP_DLB_CLOSE)                                                      */
} tsp_nl_dlb_stats;
typedef struct {
    int64_t decisions, moves, moves_2opt, moves_oropt, moves_by_len[3], moves_reversed, reversed, deltas_executed;
    double seconds, device_ms;
    int64_t moves_3opt, moves_by_type[4];
    int64_t iterations, accepted, last_improved;
    double start_cost;      /* tsp_ils_stats, in its layout                                                                     */
    int64_t active_nodes;   /* as above, summed over all descents of the chain                                                  */
    int64_t closing_scans;
} tsp_ils_dlb_stats;
/* tsp_dev_nl_3opt under dlb_mode from the set `active`.  A mode that is none of the three: TSP_DEV_E_ARG, and the caller's tours
 * are untouched. */
int tsp_dev_nl_3opt_dlb(tsp_dev_inst *inst, int kinds, int dlb_mode, int B, int *succ, int succ_stride, int64_t tour_stride,
                        double *obj, const unsigned char *active, int64_t max_moves, double time_limit_s,
                        tsp_nl_dlb_stats *stats);
/* tsp_dev_ils with every descent under dlb_mode.  A bad mode as above. */
int tsp_dev_ils_dlb(tsp_dev_inst *inst, int kinds, int B, int *succ, int succ_stride, int64_t tour_stride, double *obj,
                    uint64_t seed, int64_t iterations, int span, int64_t max_moves_per_descent, double time_limit_s,
                    int dlb_mode, tsp_ils_dlb_stats *stats);

/* ---- batched list descent (extension): many moves with disjoint arcs per decision ----------------------------------------------
 * (DESIGN.md 4.19 has the kernels.)  A new descent rule behind a new entry point: tsp_dev_nl_3opt, the don't-look entry points
 * and tsp_dev_ils keep their trajectories.  Moves, deltas, keys, the order (delta, kind, key), the candidates cand(v) of a node
 * and the way a move is applied are those above.  Positions are along the successor orientation, modulo n; ahead(p, q) = p - q.
 * Arc of a move: the cyclic range (start, len) of the positions the move rewrites, extended by the ends of its removed edges.
 *     2-opt (i, j):        start = pos i, len = ahead(pos j, pos i) + 2                 (i .. j1)
 *     3-opt (a, b, c, T):  start = pos a, len = ahead(pos c, pos a) + 2                 (a .. c1)
 *     Or-opt (f, L, a, o): with m1 = ahead(pos a, pos f + L) + 1 nodes s .. a and m2 = n - L - m1 nodes b .. p:
 *                          m1 <= m2: start = pos f - 1, len = m1 + L + 2 (p .. b);  else start = pos a, len = m2 + L + 2 (a .. s)
 * len is clipped to n.  Two arcs are disjoint iff ahead(s2, s1) >= len1 and ahead(s1, s2) >= len2.  Both ends of every new and of
 * every removed edge lie inside the arc and its two end positions keep their nodes, so moves with disjoint arcs commute and the
 * delta of each, computed before the decision, stays exact.
 * Decision.  For every node v the candidate is the best (delta, key) of the improving moves of cand(v) whose arc has
 * len <= max_arc; the overall best move of any arc length is kept beside them.  Up to `rounds` claim rounds run over the live
 * candidates (at first all): every live candidate claims every position of its arc, a position goes to the smallest (delta, key)
 * that claims it, a candidate that holds all of its positions is accepted, and the live candidates whose arc meets an accepted
 * arc die.  What is live after the last round is dropped.  With enough rounds (n at the most) that is the sequential greedy
 * selection by (delta, key).  Without any candidate the overall best move alone is applied, and without one the descent ends:
 * the result is a local optimum of the whole list neighbourhood.  max_moves >= 0: the accepted set is cut to its first
 * max_moves - moves members in (delta, key) order.  `decisions` counts decisions, `moves` moves; the other counters keep their
 * meaning.  The result does not depend on the order in which the accepted moves are carried out: two runs return the same bits. */
#define TSP_NL_BATCH_DEFAULT_ROUNDS 2
/* max_arc <= 0: n / 2 (more than n: n).  rounds <= 0: TSP_NL_BATCH_DEFAULT_ROUNDS (more than n: n).  Everything else, bad arguments
 * (TSP_DEV_E_ARG, the caller's tours untouched) included, as tsp_dev_nl_3opt. */
int tsp_dev_nl_3opt_batch(tsp_dev_inst *inst, int kinds, int max_arc, int rounds, int B, int *succ, int succ_stride,
                          int64_t tour_stride, double *obj, int64_t max_moves, double time_limit_s, tsp_nl3_opt_stats *stats);

/* ---- windowed iterated local search (extension; tour segmentation, Johnson & McGeoch): one kick-repair-accept trial per tour
 * window, all windows of an iteration at once ---------------------------------------------------------------------------------
 * (DESIGN.md 4.20 has the kernel.)  A new rule behind a new entry point: tsp_dev_ils, tsp_dev_ils_dlb and the descents keep their
 * trajectories.  The lists N(v), cand(v), the 2-opt and Or-opt moves, their deltas (every d with the lower node id first, in the
 * order given above), keys, the order (delta, kind, key), ends(m) and mix are those of the sections above.
 * Arguments.  kinds: a non-empty subset of TSP_NL_2OPT | TSP_NL_OROPT (TSP_NL_3OPT: TSP_DEV_E_ARG).  iterations I >= 0.
 * trials T >= 1.  max_moves_per_trial < 0: no cap.
 *     window W:  9 <= W <= min(TSP_SEG_ILS_MAX_WINDOW, n - 1);  window <= 0: min(TSP_SEG_ILS_DEFAULT_WINDOW, n - 1)
 *     span S:    8 <= S <= W - 1;                                span <= 0: W - 1
 * Any other window or span is TSP_DEV_E_ARG.  n < 10 has no window: the call returns the tours unchanged, iterations = 0 and
 * obj = the tour's cost.
 * Windows of iteration `it` of chain b.  M = n / W (rounded down).  base = mix(mix(seed ^ (b * 0x100000001B3)) + it), the base
 * of tsp_dev_ils; the anchor is node s = mix(base) % n.  Window w, 0 <= w < M, is the path seq_w[0 .. W-1] of W nodes that starts
 * w * W steps after s along succ; the n - M W nodes behind the last window belong to none.  (Nodes and succ only: how a caller
 * rotates a tour does not matter.)  The window's edges are the W - 1 tour edges (seq_w[k], seq_w[k+1]); out_w = succ seq_w[W-1]
 * is outside the window because W <= n - 1.
 * Window move.  A 2-opt or Or-opt move of the list neighbourhood every removed edge of which is a window edge and, Or-opt, whose
 * segment f .. l is a path of window edges (only at W = n - 1 and L = 3 can the three removed edges be window edges around a
 * segment seq_w[W-1], out_w, seq_w[0] that is not).  Delta and key are those of tsp_dev_nl_3opt.  Applied, it gives the same
 * undirected tour as there, written so that every node outside seq_w[1 .. W-2] keeps its successor: only the interior of the
 * window path is permuted.  A 2-opt move reverses the window sub-path between its two removed edges, whichever of i, j comes
 * first in the window, and `reversed` counts the nodes of that sub-path; an Or-opt move shifts inside the window.
 * Window cost.  x[k] = d(seq[k], seq[k+1]) for k < W - 1 and +0.0 up to P, the next power of two >= W - 1; for h = P/2, P/4, .., 1:
 * x[k] += x[k+h] for all k < h; the cost is x[0].
 * Trial t, 0 <= t < T, of window w.  bw = mix(base + 8 + w T + t), the draws v_j = mix(bw + j), j = 0 .. 4.
 *   1. c0 = the window cost of the incumbent window.
 *   2. Kick.  off = v_0 % (W - S); with q[k] = seq_w[off + k] the cuts o1 .. o4 are those of Kick above with W there replaced by S
 *      and u_1 .. u_4 by v_1 .. v_4; the window becomes seq_w[0:off] q[0:o1] q[o3:o4] q[o2:o3] q[o1:o2] q[o4:].  off + o4 <= W - 1:
 *      the first and the last window node stay.
 *   3. A = q[o1-1], q[o1], q[o2-1], q[o2], q[o3-1], q[o3], q[o4-1], q[o4], read before the kick.
 *   4. The descent of mode TSP_DLB_ON from A with cand(v) cut down to window moves: per decision the best (delta, kind, key)
 *      over v in A is applied and A becomes its nodes with an improving window move plus ends(m); it ends at the first decision
 *      without a move or after max_moves_per_trial moves.
 *   5. c1 = the window cost.  The kicked and repaired window becomes the incumbent iff c1 < c0; else the window is the
 *      incumbent's again.
 * The T trials of a window run one after the other; the windows of an iteration touch disjoint sets of successors, so the result
 * does not depend on their order; iterations run one after the other.  There is no descent before the first iteration: the
 * caller's tour is the incumbent (callers run tsp_dev_nl_3opt_batch first).  obj[b] is the recomputed cost of the final tour.
 * Time limit.  Checked between launches; TSP_TIME_LIMIT_EXCEEDED, stats.iterations counts the completed iterations, and a call
 * without a limit and with that count returns the same bits.  Chain b of a batch equals a single call with stream b.  Two runs
 * return the same bits in the tour, the cost and every counter but the times. */
#define TSP_SEG_ILS_MAX_WINDOW 2048     /* what the kernel's LDS layout holds within 64 KB a workgroup */
#define TSP_SEG_ILS_DEFAULT_WINDOW 1024 /* the lowest cost at equal time at n = 100 003 */
typedef struct {
    int64_t decisions, moves, moves_2opt, moves_oropt, moves_by_len[3], moves_reversed, reversed, deltas_executed;
    double seconds, device_ms; /* tsp_nl_opt_stats, in its layout: the sums over all trials                                    */
    int64_t iterations;        /* completed iterations (launches)                                                              */
    int64_t windows;           /* M                                                                                            */
    int64_t trials;            /* iterations * M * T                                                                           */
    int64_t accepted;          /* trials whose window became the incumbent                                                     */
    int64_t active_nodes;      /* sum of |A| at the start of every decision                                                    */
    double start_cost;         /* the recomputed cost of the caller's tour                                                     */
} tsp_seg_ils_stats;
/* B chains, chain b from tour b with stream b.  Lists and the default lists as tsp_dev_nl_3opt.  Bad arguments: TSP_DEV_E_ARG,
 * and the caller's tours are untouched. */
int tsp_dev_seg_ils(tsp_dev_inst *inst, int kinds, int B, int *succ, int succ_stride, int64_t tour_stride, double *obj,
                    uint64_t seed, int64_t iterations, int window, int span, int trials, int64_t max_moves_per_trial,
                    double time_limit_s, tsp_seg_ils_stats *stats);

/* ---- windowed iterated local search with the 3-opt kind (extension): segment moves inside a window -----------------------------
 * (DESIGN.md 4.21 has the kernel.)  A new entry point beside tsp_dev_seg_ils, which keeps refusing TSP_NL_3OPT and keeps its
 * trajectories.  kinds: a non-empty subset of TSP_NL_2OPT | TSP_NL_OROPT | TSP_NL_3OPT; with TSP_NL_3OPT, n > 2^20 is
 * TSP_DEV_E_ARG as in tsp_dev_nl_3opt.  Everything else -- windows, draws, kick, A, accept, window cost, time limit, n < 10 -- is
 * the text of the section above, with three additions.
 * Window 3-opt move.  A 3-opt move of the list neighbourhood all three removed edges of which are window edges: the tails a, b, c
 * lie at slots 0 .. W - 2 of the window path.  cand(v), delta, key and the order (delta, kind, key) are those of the don't-look
 * section and of tsp_dev_nl_3opt: the delta is summed in its stated order under the (a, b, c, type) labelling, where a is the tail
 * of lowest node id and b and c follow it in tour order, through the outside of the window where that is the way round.
 * ends(m) = a, a1, b, b1, c, c1.
 * Applied, it gives the same undirected tour as tsp_dev_nl_3opt's move, written so that slots 0 and W - 1 keep their nodes and no
 * successor outside the window changes.  With the tails at slots i < j < k, X = slots i+1 .. j, Y = slots j+1 .. k and a at slot
 * i (r = 0), j (r = 1) or k (r = 2), the slots i+1 .. k become (' = reversed)
 *                type 0   type 1   type 2   type 3
 *         r = 0   Y X     X' Y'    Y' X     Y X'
 *         r = 1   Y X     Y X'     X' Y'    Y' X
 *         r = 2   Y X     Y' X     Y X'     X' Y'
 * that is Y X for type 0 and else form (type - 1 + 2 r) mod 3 of (X' Y', Y' X, Y X').  Key and delta stay those of the
 * (a, b, c, type) labelling; only the permutation is relabelled.
 * Counters.  A window 3-opt move adds to moves, moves_3opt and moves_by_type[type], type as in its key, and to nothing else:
 * `reversed` stays the count of the 2-opt moves.
 * With kinds inside TSP_NL_2OPT | TSP_NL_OROPT the call returns the bits of tsp_dev_seg_ils. */
typedef struct {
    int64_t decisions, moves, moves_2opt, moves_oropt, moves_by_len[3], moves_reversed, reversed, deltas_executed;
    double seconds, device_ms;
    int64_t iterations, windows, trials, accepted, active_nodes;
    double start_cost;                    /* tsp_seg_ils_stats, in its layout                                                   */
    int64_t moves_3opt, moves_by_type[4]; /* the window 3-opt moves, summed over all trials                                     */
} tsp_seg_ils3_stats;
int tsp_dev_seg_ils3(tsp_dev_inst *inst, int kinds, int B, int *succ, int succ_stride, int64_t tour_stride, double *obj,
                     uint64_t seed, int64_t iterations, int window, int span, int trials, int64_t max_moves_per_trial,
                     double time_limit_s, tsp_seg_ils3_stats *stats);

/* ---- windowed iterated local search with groups (extension): several trial groups per window, disjoint commits ---------------
 * (DESIGN.md 4.22 has the kernels.)  A new rule behind a new entry point: tsp_dev_seg_ils and tsp_dev_seg_ils3 keep their
 * trajectories.  kinds, windows, anchor, base, kick, A, the repair, the window cost, the accept test, n < 10, the time limit,
 * the lists and the argument checks are those of tsp_dev_seg_ils3.
 * Groups G.  1 <= groups <= TSP_SEG_ILS_MAX_GROUPS; groups <= 0: max(1, min(TSP_SEG_ILS_MAX_GROUPS, 1024 / M)), a function of n
 * and W only (1024 = 256 CUs x the kernel's four resident workgroups), 1 where n < 10; more than TSP_SEG_ILS_MAX_GROUPS:
 * TSP_DEV_E_ARG, the caller's tours untouched.
 * Group g, 0 <= g < G, of window w in iteration `it` starts from seq_w as the iteration found it and runs T trials one after
 * the other, steps 1 - 5 of a trial, with bw = mix(base + 8 + (w G + g) T + t).  What it accepts carries into its own next trial;
 * no group sees another group.  At the end fin_g is its incumbent window, c_start the window cost of seq_w and c_g that of fin_g.
 * Offer.  g offers iff it accepted at least one trial; then fin_g != seq_w and c_g < c_start.  lo_g and hi_g are the lowest and
 * the highest slot at which fin_g differs from seq_w (1 <= lo_g <= hi_g <= W - 2) and gain_g = c_g - c_start, one fp64
 * subtraction.  The edges g changed are those of the slots lo_g - 1 .. hi_g.
 * Conflict and commit.  Two offers g and h conflict iff lo_h - 1 <= hi_g and lo_g - 1 <= hi_h.  g loses to h iff they conflict
 * and (gain_h, h) < (gain_g, g) lexicographically.  g commits iff it offers and loses to no group: the best offer of a window
 * always commits, and committed groups never conflict pairwise.
 * New window.  seq_w with, for every committed g, the slots lo_g .. hi_g replaced by those of fin_g; each such interval is a
 * permutation of itself.  Slots 0 and W - 1 and every successor outside the window stay.  The combined cost is not checked again
 * (the committed groups share no edge, so every gain is kept).  obj is the recomputed cost of the final tour.
 * Counters.  Every counter of tsp_seg_ils3_stats, `accepted` included, is the sum over all groups, committed or not;
 * trials = iterations * M * G * T.  iterations counts the completed iterations (two launches each).
 * G = 1: the call returns the bits of tsp_dev_seg_ils3 in the tour, the cost and every shared counter, and with kinds inside
 * TSP_NL_2OPT | TSP_NL_OROPT those of tsp_dev_seg_ils.  Two runs return the same bits, a time-limited run equals a run without a
 * limit of its completed iterations, and chain b of a batch equals a single call with stream b. */
#define TSP_SEG_ILS_MAX_GROUPS 64
typedef struct {
    int64_t decisions, moves, moves_2opt, moves_oropt, moves_by_len[3], moves_reversed, reversed, deltas_executed;
    double seconds, device_ms;
    int64_t iterations, windows, trials, accepted, active_nodes;
    double start_cost;
    int64_t moves_3opt, moves_by_type[4]; /* tsp_seg_ils3_stats, in its layout                                                 */
    int64_t groups;                       /* G                                                                                  */
    int64_t offers;                       /* groups that ended an iteration with a changed window                               */
    int64_t commits;                      /* offers written to the tour                                                         */
} tsp_seg_ils_groups_stats;
int tsp_dev_seg_ils_groups(tsp_dev_inst *inst, int kinds, int groups, int B, int *succ, int succ_stride, int64_t tour_stride,
                           double *obj, uint64_t seed, int64_t iterations, int window, int span, int trials,
                           int64_t max_moves_per_trial, double time_limit_s, tsp_seg_ils_groups_stats *stats);

/* ---- windowed iterated local search with Lin-Kernighan chains (extension): a fourth kind of the window repair ------------------
 * (DESIGN.md 4.23 has the kernel.)  A new kind behind a new entry point: tsp_dev_seg_ils, tsp_dev_seg_ils3, tsp_dev_seg_ils_groups
 * and tsp_host_set_seg_ils_kinds keep refusing TSP_NL_LK and keep their trajectories.  kinds: any non-empty subset of TSP_NL_2OPT |
 * TSP_NL_OROPT | TSP_NL_3OPT | TSP_NL_LK.  lk_depth D: 1 <= D <= TSP_SEG_LK_MAX_DEPTH; lk_depth <= 0: TSP_SEG_LK_DEFAULT_DEPTH; more
 * than TSP_SEG_LK_MAX_DEPTH: TSP_DEV_E_ARG, the caller's tours untouched.  Everything else -- windows, anchor, draws, kick, A, the
 * accept test, the window cost, groups / offers / commits, the time limit, n < 10, the lists, the argument checks -- is the text of
 * tsp_dev_seg_ils_groups.  Without TSP_NL_LK the call returns the bits of tsp_dev_seg_ils_groups in the tour, the cost and every
 * shared counter.
 * Chain.  For a window node t1 at slot i and a side s in {0, 1}; written for s = 0, side 1 is the same text on the window read
 * backwards (slot k <-> W - 1 - k).  It needs i <= W - 2.  It works on a private image cur of the window path and touches nothing
 * else.  Start with G = +0.0, best = +0.0, h* = 0, used = {}.  Step h = 1 .. D:
 *   e = cur[i + 1], and x = d(t1, e).
 *   A list entry y = nbr[e][k], k = 0 .. K - 1, is admissible when all of these hold: y != e; y is a window node at slot j of cur
 *   with i + 3 <= j <= W - 1; y is not in used; g1 = (G + x) - d(e, y) > best.
 *   For an admissible entry, p = cur[j - 1] and g2 = g1 + d(p, y).
 *   The step takes the admissible entry of largest g2, lowest k on ties.  Without one the chain ends.
 *   It reverses slots i + 1 .. j - 1 of cur.  used gains e and y, and e_h, y_h, p_h = e, y, p.
 *   G = g2 - d(p, t1).  If G > best, then best = G and h* = h.
 * Every d takes the lower node id first.  All sums are fp64 in the written order, with contraction off.
 * The chain offers iff h* >= 1.  Then the move is the first h* reversals; delta = -best; its kind index is 3, the last in the order
 * (delta, kind, key), so a chain loses ties to every other kind; key = 2 t1 + s; ends(m) = {t1} and e_h, y_h, p_h for h <= h*.
 * All removed edges are window edges and only slots inside 1 .. W - 2 move, so the move is a window move.  Its hull lo .. hi is
 * that of its reversals.
 * Decision.  With TSP_NL_LK every v in A also runs chain(v, 0) and chain(v, 1) on the window as the decision found it.  v gets a
 * hit if either chain offers.  The decision applies the best (delta, kind, key) over all kinds.  A becomes the nodes with a hit
 * plus ends(m), as before.  An applied chain counts as one move against max_moves_per_trial.
 * Counters.  tsp_seg_ils_lk_stats is tsp_seg_ils_groups_stats in its layout followed by lk_depth and four counters summed over
 * all trials and groups like the others.  An applied chain adds to moves, moves_lk and lk_flips and to nothing else: `reversed`
 * stays the count of the 2-opt moves. */
enum { TSP_NL_LK = 8 }; /* kinds mask of tsp_dev_seg_ils_lk, beside TSP_NL_2OPT, TSP_NL_OROPT and TSP_NL_3OPT */
#define TSP_SEG_LK_MAX_DEPTH 16    /* steps of a chain at most: what a chain's record in LDS holds                              */
#define TSP_SEG_LK_DEFAULT_DEPTH 16 /* the lowest cost after 10 s at n = 100 003, W = 1024                   */
typedef struct {
    int64_t decisions, moves, moves_2opt, moves_oropt, moves_by_len[3], moves_reversed, reversed, deltas_executed;
    double seconds, device_ms;
    int64_t iterations, windows, trials, accepted, active_nodes;
    double start_cost;
    int64_t moves_3opt, moves_by_type[4];
    int64_t groups, offers, commits; /* tsp_seg_ils_groups_stats, in its layout                                                */
    int64_t lk_depth;                /* the D used                                                                             */
    int64_t moves_lk;                /* applied chains                                                                         */
    int64_t lk_flips;                /* the sum of h* over the applied chains                                                  */
    int64_t lk_chains;               /* pairs (v, s), v in A, that have a first edge                                           */
    int64_t lk_steps;                /* reversals made by all chains, kept or not                                              */
} tsp_seg_ils_lk_stats;
int tsp_dev_seg_ils_lk(tsp_dev_inst *inst, int kinds, int lk_depth, int groups, int B, int *succ, int succ_stride,
                       int64_t tour_stride, double *obj, uint64_t seed, int64_t iterations, int window, int span, int trials,
                       int64_t max_moves_per_trial, double time_limit_s, tsp_seg_ils_lk_stats *stats);

/* ---- Held-Karp lower bound (extension): minimum 1-trees under node penalties, driven by subgradient ascent -------------------
 * (The reference bounds its tours with CPLEX models, which are out of scope here; DESIGN.md 4.12 has the kernels and times.)
 * d(i,j) is the value tsp_dev_dist_pairs returns; the penalties are pi[0 .. n-1], fp64.
 * Weight of edge {i,j}, lo = min, hi = max:  w = (d(lo,hi) + pi[lo]) + pi[hi], evaluated in exactly this order.
 * Edge order: lexicographic on (w, lo, hi) -- a strict total order, so the minimum spanning tree is unique.
 * 1-tree (n >= 3, special node 0): the minimum spanning tree of nodes 1 .. n-1 under that order plus the two smallest edges at
 * node 0 under the same order.  deg[v] = degree of v in it (the degrees sum to 2n).
 * Value: W(pi) = sum of w(e) over the 1-tree - 2 * sum of pi[v].  Every tour costs at least W(pi), for every pi.  The sums are
 * taken in a fixed order without floating-point atomics: two runs return the same bits.
 * Ascent (host-visible scalars fp64): pi as given (NULL = zeros), lambda = lambda0, best = -inf, stall = 0; per iteration
 *   1. the 1-tree, W and g = deg - 2;
 *   2. W > best: best = W, pi_best = pi, stall = 0; else stall += 1 and, when it reaches patience, lambda /= 2, stall = 0;
 *   3. |g|^2 == 0: the 1-tree is a tour: stop with tour_found = 1;
 *   4. t = lambda (ub - W) / |g|^2,  pi += t (0.7 g + 0.3 g_prev)   (first iteration: g_prev = g);
 *   5. stop after max_iters iterations or at the time limit;
 * and best, pi_best are returned.  At the time limit: TSP_TIME_LIMIT_EXCEEDED with the best so far, which is a valid bound. */
#define TSP_HK_DEFAULT_ITERS 300
#define TSP_HK_DEFAULT_LAMBDA 2.0
typedef struct {
    int64_t iterations;     /* ascent iterations carried out (0 from tsp_dev_one_tree)                                      */
    int64_t trees;          /* 1-trees built                                                                                */
    int64_t rounds;         /* Boruvka rounds over all trees                                                                */
    int64_t dists_executed; /* edge weights the scans evaluated (rows of the launched grid x (n - 1) columns per round)     */
    int tour_found;         /* a 1-tree was a tour: the bound is the optimum                                                */
    double lambda_final;
    double seconds;         /* wall time of the call, host clock                                                            */
    double device_ms;       /* device time of the call, HIP events on the engine's stream                                   */
} tsp_lb_stats;
/* One 1-tree for pi (NULL = zeros).  edges: n pairs (lo, hi), sorted; deg[n]; *value = W(pi).  Each output may be NULL.
 * Penalties that are not finite: TSP_DEV_E_ARG. */
int tsp_dev_one_tree(tsp_dev_inst *inst, const double *pi, int *edges, int *deg, double *value, tsp_lb_stats *stats);
/* The ascent.  ub: the cost of any tour, finite and > 0; max_iters >= 1; lambda0 > 0; patience <= 0 = max(10, n / 20);
 * time_limit_s <= 0 = unlimited (at least one iteration always runs).  pi (may be NULL): in, the start (zeros when NULL); out,
 * pi_best.  *bound = best.  Bad arguments: TSP_DEV_E_ARG with the reason in tsp_dev_last_error(). */
int tsp_dev_held_karp(tsp_dev_inst *inst, double ub, int max_iters, double lambda0, int patience, double time_limit_s,
                      double *pi, double *bound, tsp_lb_stats *stats);

/* ---- Held-Karp ascent over the candidate graph, certified by dense 1-trees (extension) -----------------------
 * d, pi, the weight w, the order (w, lo, hi), special node 0 and W are those of the Held-Karp section above.
 * Candidate graph C: the undirected edges {v, nbr[v][k]} of the lists in the handle (tsp_dev_inst_knn_build / _knn_set /
 * _alpha_build); an edge that several entries name counts once.  Without lists in the handle the call builds nearest-neighbour
 * lists with K = min(TSP_NL_DEFAULT_K, n - 1), as tsp_dev_nl_opt does.  Any lists tsp_dev_inst_knn_set accepts are legal: C may
 * be disconnected, a node may be named by every list, K may be 1.
 * Sparse 1-tree T_C(pi), n >= 3.  Spanning part: Kruskal over the edges of C among nodes 1 .. n-1 in the order (w, lo, hi); if
 * more than one component is left, Kruskal goes on over ALL edges among nodes 1 .. n-1 in the same order (the completion).
 * Node 0: the two smallest edges of C at node 0 in the same order; if C has fewer than two edges at node 0, the two smallest of
 * all n - 1 edges at node 0, as in the dense tree.  W_C(pi) is the same sum as W, taken over T_C.  W_C(pi) >= W(pi), and W_C is
 * NOT a lower bound.  With C complete (K = n - 1) T_C = T.
 * Rounds (deterministic under the strict order): sparse_rounds = the Boruvka rounds over C in which at least one component
 * hooks; completion_rounds = the Boruvka rounds over the complete graph behind them, counted while more than one component exists.
 * Ascent in two phases.  Sparse phase: steps 1 - 5 of the ascent above with T_C, W_C, best_C, pi_best_C in place of T, W, best,
 * pi_best, for at most sparse_iters iterations, with two changes: |g|^2 == 0 ends the phase WITHOUT tour_found (a sparse tree that
 * is a tour proves nothing), and W_C >= ub ends the phase before step 4 (the step length would not be positive).  Dense phase:
 * exactly tsp_dev_held_karp(ub, dense_iters, lambda0 = the sparse phase's final lambda, patience, what is left of the time
 * limit, pi = pi_best_C); its best, pi_best and tour_found are the call's.  The returned bound therefore always comes from dense
 * 1-trees and is valid.  With sparse_iters = 0 the call is tsp_dev_held_karp(ub, dense_iters, lambda0, ...) to the bit; with
 * K = n - 1 the sparse phase follows the dense ascent step for step.  The sparse phase stops at the time limit (after at least
 * one iteration), at least one dense iteration always runs, and the status is then TSP_TIME_LIMIT_EXCEEDED.  No floating-point
 * atomics: two runs return the same bits.
 * The number of queued rounds of one tree is limited to 32: lists whose candidate graph needs more sparse plus completion
 * rounds than that (more than about 2^15 components at n = 10^5) end in TSP_DEV_E_HIP with the reason in tsp_dev_last_error(). */
typedef struct {
    int64_t iterations;     /* the dense phase's counters, laid out as tsp_lb_stats ...                                     */
    int64_t trees;
    int64_t rounds;
    int64_t dists_executed;
    int tour_found;
    double lambda_final;
    double seconds;         /* ... but seconds and device_ms cover the whole call                                           */
    double device_ms;
    int64_t sparse_iterations;  /* iterations of the sparse phase                                                           */
    int64_t sparse_trees;       /* sparse 1-trees built                                                                     */
    int64_t sparse_rounds;      /* over all sparse trees                                                                    */
    int64_t completion_rounds;  /* over all sparse trees                                                                    */
    int64_t candidate_entries;  /* n * K                                                                                    */
    int64_t components;         /* of C on nodes 1 .. n-1 (0: no sparse tree was built)                                     */
    int64_t weights_executed;   /* edge weights the sparse scans evaluated: n * K per executed round over C                 */
    double sparse_best;         /* best_C (-inf: no sparse tree was built)                                                  */
    double lambda_sparse_final;
    double sparse_device_ms;    /* device time of the sparse phase, entry distances included                                */
} tsp_lb_sparse_stats;
/* One T_C(pi) (pi NULL = zeros).  Outputs as tsp_dev_one_tree's, *value = W_C(pi); stats (may be NULL): the sparse fields of the
 * one tree; of the dense counters dists_executed alone (the completion's scans; 0 for connected lists).  Penalties that are not
 * finite or n < 3: TSP_DEV_E_ARG. */
int tsp_dev_one_tree_sparse(tsp_dev_inst *inst, const double *pi, int *edges, int *deg, double *value, tsp_lb_sparse_stats *stats);
/* sparse_iters >= 0, dense_iters >= 1; ub, lambda0, patience, time_limit_s, pi, bound as tsp_dev_held_karp.  Bad arguments:
 * TSP_DEV_E_ARG with the reason in tsp_dev_last_error(); the caller's pi and the handle's lists are untouched. */
int tsp_dev_held_karp_sparse(tsp_dev_inst *inst, double ub, int sparse_iters, int dense_iters, double lambda0, int patience,
                             double time_limit_s, double *pi, double *bound, tsp_lb_sparse_stats *stats);

/* ---- alpha-nearness candidate lists (extension; Helsgaun's LKH): what the minimum 1-tree says about an edge ------------------
 * (DESIGN.md 4.13 has the kernels and times.)  d, pi, the edge weight w, the edge order (w, lo, hi) and the minimum 1-tree T(pi)
 * with special node 0 are those of the Held-Karp section above.  For two nodes i != j:
 *   {i,j} an edge of T:    alpha(i,j) = 0;
 *   else i = 0 or j = 0:   alpha(i,j) = w(i,j) - w0, w0 = the weight of the larger (in the edge order) of the two 1-tree edges at
 *                          node 0;
 *   else:                  alpha(i,j) = w(i,j) - beta(i,j), beta = the weight of the largest edge (in the edge order) on the path
 *                          from i to j in the spanning tree of nodes 1 .. n-1.
 * One fp64 subtraction of two weights, each evaluated as above.  alpha >= 0 without clamping (the tree is minimal under the
 * order), alpha is symmetric, and it equals W(minimum 1-tree forced to contain {i,j}) - W(T).
 * Alpha lists: for 1 <= K <= min(TSP_NL_MAX_K, n - 1), nbr[v][0 .. K-1] are the K nodes u != v smallest by
 * (alpha(v,u), w(v,u), u), in that order; the tree neighbours of v (alpha 0) therefore come first, by weight.
 * TSP_ALPHA_DEFAULT_K is Helsgaun's default: a convention, not a number measured here.  No floating-point atomics: two runs
 * return the same bits. */
#define TSP_ALPHA_DEFAULT_K 5
typedef struct {
    int64_t trees;          /* 1-trees built (1)                                                                            */
    int64_t rounds;         /* Boruvka rounds of the tree                                                                   */
    int64_t pairs_executed; /* alpha values the scan evaluated (lanes of the launched grid x n columns)                      */
    double tree_value;      /* W(pi) of the tree                                                                            */
    double seconds;         /* wall time of the call, host clock                                                            */
    double device_ms;       /* device time of the call: the tree + the alpha kernels, HIP events on the engine's stream     */
} tsp_alpha_stats;
/* Builds T(pi) (pi NULL = zeros), then the alpha lists, and stores them in the handle's list slot: tsp_dev_inst_knn_get returns
 * them and tsp_dev_nl_opt uses them.  alpha (may be NULL): n x K out, alpha(v, nbr[v][k]).  stats may be NULL.  Bad K, n < 3 or
 * a penalty that is not finite: TSP_DEV_E_ARG with the reason in tsp_dev_last_error(), and the lists the handle had stay in
 * place. */
int tsp_dev_inst_alpha_build(tsp_dev_inst *inst, int K, const double *pi, double *alpha, tsp_alpha_stats *stats);
/* Whole alpha rows for inspection and thresholds: out[r][u] = alpha(rows[r], u) for r < m (m >= 1), out[r][rows[r]] = 0.  A row
 * index out of range or a penalty that is not finite: TSP_DEV_E_ARG as above.  The handle's lists are left alone. */
int tsp_dev_alpha_rows(tsp_dev_inst *inst, const double *pi, int m, const int *rows, double *out);

/* ---- greedy-edge construction (extension; Bentley, Johnson & McGeoch: the customary start of 2-opt, 3-opt and LK codes) --------
 * (DESIGN.md 4.17 has the kernels.)  d(i,j) is the value tsp_dev_dist_pairs returns, taken with the lower node id first.
 * Edge order: lexicographic on (d, lo, hi), lo = min, hi = max -- the Held-Karp section's order with pi = 0, a strict total order.
 * Greedy edge, n >= 3: all n(n-1)/2 edges are walked in that order; {u,v} is accepted iff both nodes have degree < 2 and they are
 * not the two ends of one fragment (the accepted edges always form paths).  After n - 1 accepted edges the one Hamiltonian path
 * is closed by the edge between its two ends.
 * Output.  edges: the n - 1 accepted edges as pairs (lo, hi), sorted by (lo, hi); the closing edge is not among them.  The tour:
 * a successor list oriented so that succ[0] is the smaller-id one of node 0's two tour neighbours.  obj: the recomputed cost,
 * the sum over nodes in node order of d(v, succ v) as in every section above.  No floating-point atomics: two runs return the
 * same bits.  The device builds the same edge set in rounds (each fragment joins along its smallest valid edge when the fragment
 * at the other end agrees), not by sorting. */
typedef struct {
    int64_t rounds;             /* rounds carried out (at most n - 1: every round accepts an edge)                          */
    int64_t edges;              /* accepted edges: n - 1                                                                    */
    int64_t rows_scanned;       /* rows (free nodes) whose smallest valid edge was looked for, over all rounds: only rows
                                   whose cached edge had become invalid are scanned again                                   */
    int64_t dists_executed;     /* distances the scans evaluated (lanes of the waves that scanned x n columns)              */
    int64_t max_edges_in_round; /* most edges accepted by one round                                                         */
    double seconds;             /* wall time of the call, host clock                                                        */
    double device_ms;           /* device time of the call, HIP events on the engine's stream                               */
} tsp_greedy_edge_stats;
/* succ: n ints, succ_stride ints apart; edges: 2(n - 1) ints; each output may be NULL.  No instance, n < 3 or a stride below 1:
 * TSP_DEV_E_ARG, and the outputs are untouched.  There is no CPU fallback. */
int tsp_dev_greedy_edge(tsp_dev_inst *inst, int *succ, int succ_stride, double *obj, int *edges, tsp_greedy_edge_stats *stats);

/* ---- partition crossover (extension; Whitley's GPX, the merging step of LKH's multi-trial runs) -------------------------------
 * (DESIGN.md 4.24 has the kernels.)  Inputs are two tours A and B on the same instance, as successor lists, n >= 3.  d(i,j) is
 * the value tsp_dev_dist_pairs returns, lower id first.
 * Fixed-point length.  q(e) = llrint(ldexp(d(e), 20)), an int64.  All sums below are sums of q, so they do not depend on the order
 *   of summation: integer atomics, and two runs return the same bits.  A parent whose sum of q would reach 2^62: TSP_DEV_E_ARG,
 *   tours untouched.
 * Base.  The parent with the smaller sum of q is the base, A on ties.  Below, "A" means the base and "B" the other; stats.base
 *   says which one it was (0: the caller's A, 1: the caller's B).  The child is oriented like the base.
 * Common edges.  An edge is common when it is in both tours, undirected; common_edges counts them.
 * Degenerate cases.  If all n edges or no edge is common, the child is the base; components is 0 or 1 respectively, and
 *   exchangeable = taken = 0.
 * Graph H.  Its nodes are all nodes, its edges the non-common edges of A and of B.  At every node the two tours have equally many
 *   non-common edges: 0, 1 or 2.  c(v) is the smallest node id in v's component of H.  A component is a component of H with at
 *   least one edge.  A portal is a node with exactly one non-common edge per tour.
 * Common runs.  A common run is a maximal path of common edges; both its ends are portals.  It is internal when c of its two ends
 *   is equal, otherwise external.
 * Stretches.  Cut A's cycle at its external common runs.  The maximal pieces that remain are the A-stretches; they are made of
 *   non-common edges and internal common runs.  Each is a contiguous interval of A's order from one portal to another and lies in
 *   exactly one component.  The B-stretches are the same construction on B's order.  With no external run there are no stretches.
 *   stats.stretches counts the A-stretches (there are as many B-stretches: one per external run).
 * Exchangeable.  A component is exchangeable when it has at least one stretch and, for every A-stretch with ends {x, y}, there is a
 *   B-stretch with ends {x, y}.  The stretches of such a component cover the same node set in both tours, so replacing all its
 *   A-stretches by the B-stretches of the same ends leaves a Hamiltonian cycle; components are node-disjoint, so any subset of
 *   them can be exchanged at once.  (Exactly two external runs at a component is GPX's classic case and always qualifies.)
 * Taken.  qA(C) and qB(C) are the sums of q over the non-common edges of A and of B in C.  C is taken iff it is exchangeable and
 *   qB(C) < qA(C), strictly; ties keep A.
 * Child.  A's order with every stretch of a taken component replaced by the B-stretch of the same ends, read from the A-stretch's
 *   first node to its last (in B's order that may run backwards, and may wrap past position n - 1).  The call returns the child's
 *   successor list in A's direction and obj, the recomputed cost of the child (the tour-cost kernel of tsp_dev_perm_cost over the
 *   child's order).  gain_q is the sum of qA - qB over the taken components.  With integer costs obj = cost(base) - gain_q / 2^20
 *   exactly, and obj <= min(cost A, cost B).
 * Components are found by hook-and-jump rounds whose number is O(log n) and capped at 8 ceil(log2 n) + 16; a run into the cap is
 * TSP_DEV_E_INTERNAL.  rounds counts them, the one that found nothing left to do included; it is the one field that may differ
 * from run to run. */
typedef struct {
    int64_t common_edges;
    int64_t components;    /* components of H                                                                            */
    int64_t exchangeable;  /* ... that are exchangeable                                                                  */
    int64_t taken;         /* ... that the child takes from the other parent                                             */
    int64_t stretches;     /* A-stretches = external common runs                                                         */
    int64_t gain_q;        /* sum of q the child lies below the base                                                     */
    int64_t rounds;        /* component rounds the device carried out for this pair                                      */
    int base;              /* 0: the caller's succ_a was the base, 1: succ_b                                             */
    double cost_a, cost_b; /* the caller's two parents, from the tour-cost kernel                                        */
    double cost_child;     /* = obj                                                                                      */
    double seconds;        /* wall time of the call, host clock                                                          */
    double device_ms;      /* device time of the call, HIP events on the engine's stream                                 */
} tsp_gpx_stats;
/* P >= 1 pairs at once: pair k is succ_a + k tour_stride and succ_b + k tour_stride, n ints each, succ_stride ints apart; its child
 * goes to succ_child + k tour_stride in the same layout.  succ_child may alias succ_a (or succ_b).  obj (P doubles) and stats (P
 * entries) may be NULL.  No instance, P < 1, a NULL tour or a stride below 1: TSP_DEV_E_ARG; a successor list that is not one
 * Hamiltonian cycle: TSP_DEV_E_NOT_A_TOUR.  On any error the caller's arrays are untouched.  There is no CPU fallback. */
int tsp_dev_gpx(tsp_dev_inst *inst, int P, const int *succ_a, const int *succ_b, int succ_stride, int64_t tour_stride, int *succ_child,
                double *obj, tsp_gpx_stats *stats);

#ifdef __cplusplus
}
#endif
#endif
