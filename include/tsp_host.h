/*
 * tsp_host.h -- C host mirror of the reference's heuristics entry points (same names, same argument
 * meaning, same status codes), implemented on top of the C ABI in include/tsp_hip.h.
 *
 * A caller written against the reference's include/utility.h + include/heuristics.h +
 * include/solver.h + include/tabusearch.h recompiles against this header unchanged for the
 * functions listed here.  The data model below restates the reference's structs field for field
 * (include/utility.h:113-160) because their layout IS the interface: `inst->nodes` is handed to the
 * device library as `const double *xy`, `&inst->solution.edges[0].j` as a stride-2 successor list.
 * The only difference: <cplex.h> is not included (the heuristics path never needed it).
 *
 * There is no CPU implementation behind these functions: each of them runs on the MI355X through
 * libtsp_hip.so and terminates the process with an [ERROR] line (the reference's LOG_E convention,
 * include/utility.h:33) if no device is available.
 */
#ifndef TSP_HOST_H
#define TSP_HOST_H

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/time.h>

#include "tsp_hip.h"   /* tsp_two_opt_stats, TSP_DEV_E_* (extensions at the end of this header) */

#ifdef __cplusplus
extern "C" {
#endif

/* ---- logging / allocation idioms of the reference (include/utility.h:10-36) ---------------- */
#define LOG_I(...) do { fprintf(stdout, "[INFO]  "); fprintf(stdout, __VA_ARGS__); fprintf(stdout, "\n"); } while (0)
#define LOG_E(...) do { fprintf(stderr, "[ERROR] "); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); \
                        fflush(NULL); exit(1); } while (0)
#define URAND() (((double)random()) / RAND_MAX)   /* include/utility.h:36 */
#define DEFAULT_TIME_LIM 900                      /* include/utility.h:41 */

/* status codes: include/heuristics.h:6-7 */
#define WRONG_STARTING_NODE 1
#define TIME_LIMIT_EXCEEDED 2

/* ---- data model: include/utility.h:45-160 --------------------------------------------------- */
typedef enum { EUC_2D, MAX_2D, MAN_2D, CEIL_2D, GEO, ATT } weight_type;                 /* :45-52 */

typedef enum {                                                                           /* :56-84 */
    SOLVE_MTZ, SOLVE_MTZL, SOLVE_MTZI, SOLVE_MTZLI, SOLVE_MTZ_IND, SOLVE_GG, SOLVE_LOOP, SOLVE_CALLBACK,
    SOLVE_UCUT, SOLVE_HARD_FIXING, SOLVE_HARD_FIXING2, SOLVE_SOFT_FIXING,
    SOLVE_GREEDY, SOLVE_GREEDY_ITER, SOLVE_EXTR_MIL, SOLVE_GRASP, SOLVE_GRASP_ITER,
    SOLVE_2OPT_GRASP, SOLVE_2OPT_GRASP_ITER, SOLVE_2OPT_GREEDY, SOLVE_2OPT_GREEDY_ITER, SOLVE_2OPT_EXTR_MIL,
    SOLVE_VNS, SOLVE_TABU_STEP, SOLVE_TABU_LIN, SOLVE_TABU_RAND, SOLVE_GENETIC,
    SOLVE_2OPT_GRASP_MULTI,  /* extension of this build (after the reference's last value): BASELINE configs[3] */
    SOLVE_2OPT_POP_MULTI,    /* extension: BASELINE configs[4], random individuals + alg_2opt each, sharded over the GPUs */
    SOLVE_2OPT_OR_GREEDY,    /* extension: greedy, then 2-opt + Or-opt to a joint local optimum (alg_2opt_oropt) */
    SOLVE_2OPT_OR_GRASP,     /* extension: grasp, then alg_2opt_oropt */
    SOLVE_2OPT_OR_EXTR_MIL   /* extension: extra mileage, then alg_2opt_oropt */
} solver_type;

typedef enum { UDIR_EDGE, DIR_EDGE } edge_type;                                          /* :99-102 */

typedef struct { solver_type id; edge_type edge_type; char *name; int use_cplex; } sol_method;   /* :105-110 */

typedef struct {                                                                         /* :113-123 */
    char *file_path;
    int num_threads;
    int time_limit;
    sol_method method;
    int verbose;
    int integer_cost;
    int seed;
    int perf_prof;
    int callback_2opt;
} instance_params;

typedef struct { double x; double y; } point;                                            /* :126-129 */
typedef struct { int i; int j; } edge;                                                   /* :134-137 */

typedef struct {                                                                         /* :139-144 */
    double obj_best;
    edge *edges;
    double time_to_solve;
    double *xbest;
} solution;

typedef struct {                                                                         /* :147-160 */
    instance_params params;
    char *name;
    char *comment;
    point *nodes;
    int num_nodes;
    weight_type weight_type;
    long num_columns;
    int *ind;
    unsigned int *thread_seeds;
    solution solution;
} instance;

/* ---- src/distutil.c ---------------------------------------------------------------------- */
double calc_dist(int i, int j, instance *inst);                                          /* distutil.h:137 */

/* ---- src/utility.c helpers on the path ------------------------------------------------------ */
int x_udir_pos(int i, int j, int num_nodes);                                             /* utility.c:17  */
double get_elapsed_time(struct timeval start, struct timeval end);                       /* utility.c:701 */
void reverse_path(instance *inst, int start_node, int end_node, int *prev);              /* utility.c:708 */
void copy_instance(instance *dst, instance *src);                                        /* utility.c:724 */
int rand_choice(int from, int to);                                                       /* utility.c:752 */
void free_instance(instance *inst);                                                      /* utility.c:340 */

/* ---- src/heuristics.c ------------------------------------------------------------------------ */
int greedy(instance *inst, int starting_node);                                           /* :18  */
int grasp(instance *inst, int starting_node);                                            /* :82  */
int HEU_greedy(instance *inst);                                                          /* :160 */
int HEU_Greedy_iter(instance *inst);                                                     /* :168 */
int HEU_extramileage(instance *inst);                                                    /* :208 */
int alg_2opt(instance *inst);                                                            /* :438 */
int HEU_Grasp(instance *inst);                                                           /* :505 */
int HEU_Grasp_iter(instance *inst, int time_lim);                                        /* :510 */
int HEU_2opt_grasp(instance *inst);                                                      /* :547 */
int HEU_2opt_grasp_iter(instance *inst);                                                 /* :559 */
int HEU_2opt_greedy(instance *inst);                                                     /* :572 */
int HEU_2opt_greedy_iter(instance *inst);                                                /* :584 */
int HEU_2opt_extramileage(instance *inst);                                               /* :596 */

/* ---- Or-opt (extension: the reference declares HEU_3opt, include/heuristics.h:51-56, and never defines it; Or-opt is
 * not 3-opt and does not take that name).  Both leave the RECOMPUTED cost of the final tour in inst->solution.obj_best --
 * unlike alg_2opt after HEU_Grasp, which carries GRASP's double-counted closing edge (heuristics.c:135,:152) along. */
int alg_oropt(instance *inst);        /* Or-opt descent (tsp_dev_or_opt) of inst->solution                          */
int alg_2opt_oropt(instance *inst);   /* alg_2opt's rule (first improvement) and Or-opt in turn until Or-opt makes no
                                         move (tsp_dev_two_opt_or_opt): a local optimum of both neighbourhoods           */
int HEU_2opt_oropt_greedy(instance *inst);        /* HEU_greedy + alg_2opt_oropt       */
int HEU_2opt_oropt_grasp(instance *inst);         /* HEU_Grasp + alg_2opt_oropt        */
int HEU_2opt_oropt_extramileage(instance *inst);  /* HEU_extramileage + alg_2opt_oropt */

/* ---- neighbour lists (extension; include/tsp_hip.h, tsp_dev_nl_opt).  Library entry points only: the solver_type enum and
 * the -method table have no rows for them. */
int tsp_host_set_knn(int K);          /* list length of alg_nl_opt, 1 .. TSP_NL_MAX_K (default TSP_NL_DEFAULT_K); else TSP_DEV_E_ARG */
int alg_nl_opt(instance *inst);       /* 2-opt + Or-opt over the lists of the min(K, n - 1) nearest nodes of inst->solution;
                                         inst->solution.obj_best receives the recomputed cost                                */
int HEU_nl_greedy(instance *inst);        /* HEU_greedy + alg_nl_opt       */
int HEU_nl_grasp(instance *inst);         /* HEU_Grasp + alg_nl_opt        */
int HEU_nl_extramileage(instance *inst);  /* HEU_extramileage + alg_nl_opt */
/* Alpha-nearness lists (include/tsp_hip.h, tsp_dev_inst_alpha_build) for alg_nl_opt and HEU_nl_*.  K = 0 (the default): the
 * nearest-neighbour lists of tsp_host_set_knn, as before.  1 <= K <= TSP_NL_MAX_K: the min(K, n - 1) alpha-nearest nodes, rebuilt
 * by every call; ascent_iters = 0: from the 1-tree of zero penalties; ascent_iters > 0: from pi_best of
 * tsp_dev_held_karp(ub = inst->solution.obj_best, ascent_iters, TSP_HK_DEFAULT_LAMBDA, default patience, no time limit, from
 * zeros).  Anything else (also ascent_iters != 0 with K = 0): TSP_DEV_E_ARG, and the setting stays. */
int tsp_host_set_alpha(int K, int ascent_iters);
/* Where that ascent begins (include/tsp_hip.h, tsp_dev_held_karp_sparse).  0 (the default): as above.  sparse_iters > 0, with
 * tsp_host_set_alpha(K, ascent_iters > 0): the penalties come from tsp_dev_held_karp_sparse(ub, sparse_iters, dense_iters =
 * ascent_iters, TSP_HK_DEFAULT_LAMBDA, default patience, no time limit, from zeros) over the nearest-neighbour lists of
 * tsp_host_set_knn, built first; the alpha lists then replace them.  A negative value: TSP_DEV_E_ARG, and the setting stays. */
int tsp_host_set_alpha_ascent(int sparse_iters);
/* The list descent with the 3-opt kind (include/tsp_hip.h, tsp_dev_nl_3opt).  Library entry points only, as above. */
int alg_3opt(instance *inst);         /* 2-opt + Or-opt + 3-opt on inst->solution over the lists tsp_host_set_knn /
                                         tsp_host_set_alpha select; obj_best receives the recomputed cost                    */
/* The library still exports no HEU_3opt, the name the reference declares and never defines (tests/test_cpu_or_opt.py holds
 * that): HEU_greedy followed by alg_3opt is that heuristic. */

/* ---- iterated local search (extension; include/tsp_hip.h, tsp_dev_ils).  Library entry points only: no solver_type, no
 * -method row.  iterations >= 0 (default 100), span 0 or >= 8 (default 50), chains >= 1 (default 1); else TSP_DEV_E_ARG and the
 * settings stay. */
int tsp_host_set_ils(int iterations, int span, int chains);
int alg_ils(instance *inst);          /* tsp_dev_ils from inst->solution: all three kinds over the lists tsp_host_set_knn /
                                         tsp_host_set_alpha select, seed = params.seed (as unsigned), params.time_limit when
                                         > 0, no cap on the moves of a descent; `chains` chains start from the one tour with
                                         streams 0 .. chains-1 and the cheapest is kept, ties -> the lower chain; obj_best
                                         receives its recomputed cost                                                        */
int HEU_ils_greedy(instance *inst);   /* HEU_greedy + alg_ils */
/* Don't-look bits (include/tsp_hip.h, tsp_dev_nl_3opt_dlb / tsp_dev_ils_dlb) for alg_3opt (from every node active), alg_ils and
 * HEU_ils_greedy: TSP_DLB_OFF (the default: the full scan, as before), TSP_DLB_ON or TSP_DLB_CLOSE; else TSP_DEV_E_ARG and the
 * setting stays.  No -method row, as for the other extensions. */
int tsp_host_set_dlb(int mode);
/* The batched rule (include/tsp_hip.h, tsp_dev_nl_3opt_batch) for alg_nl_opt, alg_3opt and HEU_nl_*: max_arc < 0 (with rounds 0)
 * is off, the default: one move per decision, as before.  max_arc >= 0 turns it on: max_arc = 0 is n / 2 and rounds = 0 is
 * TSP_NL_BATCH_DEFAULT_ROUNDS.  rounds < 0, max_arc < 0 with rounds != 0, or on while tsp_host_set_dlb is not TSP_DLB_OFF:
 * TSP_DEV_E_ARG and the setting stays; so does tsp_host_set_dlb with a mode other than TSP_DLB_OFF while the batched rule is on.
 * alg_ils keeps the plain rule.  No -method row, as for the other extensions. */
int tsp_host_set_batch(int max_arc, int rounds);

/* ---- Held-Karp lower bound (extension; include/tsp_hip.h, tsp_dev_held_karp).  A library entry point only: no solver_type,
 * no -method row.  Runs the ascent on the instance's device handle from zero penalties with TSP_HK_DEFAULT_LAMBDA and the
 * default patience; ub = the cost of any tour (inst->solution.obj_best after a heuristic), max_iters <= 0 =
 * TSP_HK_DEFAULT_ITERS, time_lim <= 0 = unlimited.  Returns the bound (valid also when the time limit ended the ascent). */
double tsp_host_lower_bound(instance *inst, double ub, int max_iters, double time_lim);
/* The same through tsp_dev_held_karp_sparse: sparse_iters >= 0 iterations over the nearest-neighbour lists of tsp_host_set_knn's
 * K (built if the handle has none of that length), then dense_iters (<= 0 = 1) dense iterations, whose bound is returned. */
double tsp_host_lower_bound_sparse(instance *inst, double ub, int sparse_iters, int dense_iters, double time_lim);

/* ---- greedy-edge construction (extension; include/tsp_hip.h, tsp_dev_greedy_edge).  Library entry points only: no
 * solver_type, no -method row. */
int HEU_greedy_edge(instance *inst);       /* the greedy-edge tour into inst->solution, its recomputed cost into obj_best, as
                                              HEU_extramileage leaves its tour                                               */
int HEU_2opt_greedy_edge(instance *inst);  /* HEU_greedy_edge + alg_2opt   */
int HEU_nl_greedy_edge(instance *inst);    /* HEU_greedy_edge + alg_nl_opt */
int HEU_ils_greedy_edge(instance *inst);   /* HEU_greedy_edge + alg_ils    */

/* ---- windowed iterated local search (extension; include/tsp_hip.h, tsp_dev_seg_ils).  Library entry points only: no
 * solver_type, no -method row.  iterations >= 0 (default 100), window 0 (TSP_SEG_ILS_DEFAULT_WINDOW) or 9 ..
 * TSP_SEG_ILS_MAX_WINDOW, span 0 (window - 1) or >= 8 (default 50), trials >= 1 (default 1); else TSP_DEV_E_ARG and the settings
 * stay.  Whether window and span fit the instance is the device call's check. */
int tsp_host_set_seg_ils(int iterations, int window, int span, int trials);
int alg_seg_ils(instance *inst);              /* tsp_dev_seg_ils from inst->solution: 2-opt + Or-opt (or the kinds set below)
                                                 over the lists tsp_host_set_knn / tsp_host_set_alpha select, one chain, seed =
                                                 params.seed (as unsigned), params.time_limit when > 0, no cap on the moves of
                                                 a trial; a span above window - 1 is cut to it; obj_best receives the
                                                 recomputed cost                                                               */
int HEU_seg_ils_greedy_edge(instance *inst);  /* HEU_greedy_edge, the batched 2-opt + Or-opt list descent (tsp_dev_nl_3opt_batch
                                                 with its default max_arc and rounds), then alg_seg_ils                        */
/* The kinds of the two functions above: a non-empty subset of TSP_NL_2OPT | TSP_NL_OROPT | TSP_NL_3OPT (default: the first two);
 * else TSP_DEV_E_ARG and the setting stays.  With TSP_NL_3OPT alg_seg_ils calls tsp_dev_seg_ils3 and the batched descent of
 * HEU_seg_ils_greedy_edge runs over the same kinds; without it alg_seg_ils calls tsp_dev_seg_ils over `kinds`. */
int tsp_host_set_seg_ils_kinds(int kinds);
/* Trial groups per window of the two functions above (include/tsp_hip.h, tsp_dev_seg_ils_groups).  1 (the default): alg_seg_ils
 * makes the calls described above.  0: tsp_dev_seg_ils_groups with the device's default, as many groups as fill the device.
 * 2 .. TSP_SEG_ILS_MAX_GROUPS: tsp_dev_seg_ils_groups with that many.  Else TSP_DEV_E_ARG and the setting stays. */
int tsp_host_set_seg_ils_groups(int groups);
/* Lin-Kernighan chains in the repair of the two functions above (include/tsp_hip.h, tsp_dev_seg_ils_lk).  0 (the default): off,
 * alg_seg_ils makes the calls described above.  1 .. TSP_SEG_LK_MAX_DEPTH: alg_seg_ils calls tsp_dev_seg_ils_lk with the kinds set
 * above plus TSP_NL_LK, that depth and the groups set above.  -1: the same with TSP_SEG_LK_DEFAULT_DEPTH.  Else TSP_DEV_E_ARG and the
 * setting stays.  The batched descent of HEU_seg_ils_greedy_edge is not changed by it. */
int tsp_host_set_seg_ils_lk(int depth);
/* Chains of the two functions above, merged by partition crossover (include/tsp_hip.h, tsp_dev_gpx).  1 (the default): alg_seg_ils
 * makes exactly the calls described above.  C = 2 .. TSP_HOST_MAX_SEG_ILS_CHAINS: the same device call with B = C chains, all from
 * inst->solution under params.seed, chain c with the device's stream c of that seed; then rounds of pairwise tsp_dev_gpx over the C
 * results -- pairs (0,1), (2,3), ... in one device call a round, an odd last one passes through -- until one tour is left, which
 * goes to inst->solution with its recomputed cost.  The windowed search's counters are chain 0's.  Else TSP_DEV_E_ARG and the
 * setting stays. */
#define TSP_HOST_MAX_SEG_ILS_CHAINS 64
int tsp_host_set_seg_ils_chains(int chains);
/* Partition crossover of two successor lists of the instance (n ints each, 1 apart) into succ_child, which may be one of them.
 * Returns tsp_dev_gpx's status; on an error nothing is written. */
int tsp_host_gpx(instance *inst, const int *succ_a, const int *succ_b, int *succ_child);

/* ---- src/tabusearch.c (externally linked there, not in its header) --------------------------- */
int alg_2opt_tabu(instance *inst, int *skip_edge, int *stored_prev, const int iter, const int tenure); /* :107 */

/* ---- src/tabusearch.c / src/vns.c drivers (wall-clock bounded like the reference's) -------------- */
int HEU_Tabu_step(instance *inst);                                                       /* tabusearch.c:323 */
int HEU_Tabu_lin(instance *inst);                                                        /* :328 */
int HEU_Tabu_rand(instance *inst);                                                       /* :333 */
int kick(instance *inst);                                                                /* vns.c:11  */
int HEU_VNS(instance *inst);                                                             /* vns.c:103 */
int HEU_Genetic(instance *inst);                                                         /* genetic.c:448 */

/* ---- src/genetic.c : fitness of `count` chromosomes at once (the reference scores one at a time, :51) */
int fitness_batch(instance *inst, const int *chromosomes, int count, double *fitness_out);

/* ---- src/solver.c ---------------------------------------------------------------------------- */
int TSP_heuc(instance *inst);                                                            /* :262 */

/* ---- CLI edge (src/utility.c:47, :351; only what the heuristics path needs) ------------------- */
void parse_comand_line(int argc, const char *argv[], instance *inst);
void parse_instance(instance *inst);
void export_tour(instance *inst);

/* ---- extensions of this build (not in the reference) ------------------------------------------ */
/* Multi-start of BASELINE configs[3]: `starts` GRASP tours drawn exactly like HEU_Grasp_iter draws
 * them (heuristics.c:519 then :127), each refined by alg_2opt on the device, best TRUE cost kept in
 * inst->solution (ties -> lowest start).  rank/world shard the starts (k % world == rank).
 * world > 1 is COLLECTIVE (one process per GPU, device LOCAL_RANK; every rank must call it): after its shard the ranks agree
 * on the winner with one RCCL all-reduce(min) of (true cost << 24 | start) -- with --fcost: min of the double cost, then min
 * of the start among its holders -- and one broadcast of its tour (tsp_dev_multistart_* of include/tsp_hip.h); the RCCL id
 * travels from rank 0 through the file TSP_RCCL_ID_FILE.  A rank whose shard fails does not exit before the collective: it
 * contributes a value that wins the minimum, every rank sees it, and every rank ends with an [ERROR] line and status 1. */
int HEU_2opt_grasp_multistart(instance *inst, int starts, int rank, int world, double *best_true_cost,
                              int *best_start);
/* One rank's share of it and nothing else: the starts k % world == rank, the shard's best in inst->solution (no communication). */
int tsp_host_multistart_shard(instance *inst, int starts, int rank, int world, double *best_true_cost, int *best_start);
/* The same job in ONE process on devices 0 .. gpus-1 (one thread per GPU, ncclCommInitAll, grouped collectives);
 * shard_seconds[gpus] (may be NULL) receives every GPU's construct + 2-opt time. */
int tsp_host_multistart_gpus(instance *inst, int starts, int gpus, double *best_true_cost, int *best_start,
                             double *shard_seconds);

/* The population job of BASELINE configs[4], same three forms: `individuals` random individuals generated exactly as
 * random_generation does (genetic.c:349-364: identity, then n swaps of two rand_choice(0, n) positions, libc stream; every
 * rank walks the whole stream), individual k on rank k % world, each refined by alg_2opt starting from its fitness
 * (the mutation-3 path, genetic.c:426-443, without its 2 s limit unless -t is given); the best refined individual (first
 * strictly better in id order, heuristics.c:534) ends in inst->solution on every rank.
 * Optional outputs, indexed by the GLOBAL individual id and filled for the individuals THIS process refined (all of them
 * in the one-process forms): costs_out[individuals], succ_out[individuals x n] (successor lists), stats_out[individuals]. */
int HEU_2opt_population_multistart(instance *inst, int individuals, int rank, int world, double *best_cost, int *best_individual,
                                   double *costs_out, int *succ_out, tsp_two_opt_stats *stats_out);
int tsp_host_population_shard(instance *inst, int individuals, int rank, int world, double *best_cost, int *best_individual,
                              double *costs_out, int *succ_out, tsp_two_opt_stats *stats_out);
int tsp_host_population_gpus(instance *inst, int individuals, int gpus, double *best_cost, int *best_individual,
                             double *shard_seconds, double *costs_out, int *succ_out, tsp_two_opt_stats *stats_out);

/* The collective epilogue on its own (what the two *_multistart entries run after their shard), COLLECTIVE over `world`
 * ranks.  In: shard_rc (< 0: this rank's shard failed), *best / *best_id (best_id < 0: empty shard), the shard's best tour in
 * inst->solution.edges.  Out, on every rank: the global winner in *best / *best_id / inst->solution and 0 -- or the same
 * negative code everywhere: TSP_HOST_E_PEER when any rank reported a failure (text of this rank's own failure, if any, in
 * tsp_host_multistart_last_error()), a TSP_DEV_E_* when the transport failed on this rank. */
#define TSP_HOST_E_PEER (-7)
int tsp_host_multistart_epilogue(instance *inst, int rank, int world, int shard_rc, double *best, int *best_id);
const char *tsp_host_multistart_last_error(void);
/* The three collectives of the epilogue.  Default (NULL): RCCL through libtsp_hip.so.  A host program that already has a
 * communicator of its own (MPI, a test harness over gloo) can carry them instead; return 0 or a negative code. */
typedef struct tsp_host_collectives {
    int (*allreduce_min_i64)(void *self, int64_t local, int64_t *out);
    int (*allreduce_min_f64)(void *self, double local, double *out);
    int (*bcast_i32)(void *self, int root, int *buf, int stride, int n);   /* n ints `stride` apart, in place */
    void *self;
} tsp_host_collectives;
void tsp_host_set_collectives(const tsp_host_collectives *c);
/* The id file of the one-process-per-GPU form (TSP_RCCL_ID_FILE, default /tmp/tsp_rccl_id.<uid>.<launcher pid>.<MASTER_PORT>)
 * holds {magic, the 128-byte RCCL id, rank 0's pid, rank 0's start time}: a reader accepts it only while that very process is
 * alive, so the file a crashed run left behind is stale whatever its age.  State of the file at `path` (NULL: the default
 * path): 0 nothing readable (symlinks are not followed), 1 live, 2 stale. */
int tsp_host_rccl_id_file_state(const char *path);
/* Starts built by the last HEU_Grasp_iter / HEU_2opt_grasp_iter call of this thread (whole batches of 256: the clock is
 * read between batches, heuristics.c:519-525 reads it per start). */
long long tsp_host_last_grasp_iter_starts(void);
/* The two drivers with a cap on the number of rounds / iterations in addition to the time limit
 * (max < 0 = time limit only, which is what HEU_VNS / HEU_Tabu_* pass).  policy: 0 step, 1 linear,
 * 2 random.  The reference's loops are bounded by the wall clock alone, which no test can reproduce. */
int tsp_host_vns(instance *inst, long long max_rounds);
int tsp_host_tabu(instance *inst, int policy, long long max_iterations);
int tsp_host_genetic(instance *inst, long long max_generations);
/* the same with the probability of mutation method 3 (alg_2opt on the offspring, genetic.c:426-443) as an argument:
 * TWO_OPT_MUTATION_PROB is 0.00 in the reference (genetic.c:18); tests raise it so that the branch is executed */
int tsp_host_genetic_ex(instance *inst, long long max_generations, double two_opt_prob);
/* ... and with the offspring that drew mutation 3 spread over devices 0 .. gpus-1 (a contiguous block of them per GPU, one thread per GPU
 * and generation, context and instance per GPU kept for the whole run); gpus <= 0: this process's device as above.  The CLI's -gpus G. */
int tsp_host_genetic_gpus(instance *inst, long long max_generations, double two_opt_prob, int gpus);
/* Values of the libc stream that this library has drawn ahead of their turn and not consumed yet (tsp_host_tabu queues chains
 * of iterations and needs every iteration's first kick draws up front; what a chain leaves unconsumed is served first by every
 * later draw of this library: URAND() of this build, rand_choice()).  0 whenever a capped run (max_iterations) has returned. */
int tsp_host_random_lookahead(void);
/* Seconds the last tsp_host_tabu / tsp_host_vns call of this thread spent in its iteration loop (the initial
 * HEU_2opt_greedy_iter excluded): iterations / this = the driver's rate. */
double tsp_host_last_driver_loop_seconds(void);
/* Counters of the last alg_2opt / alg_2opt_tabu call of this thread. */
void tsp_host_last_stats(long long *sweeps, long long *evals, long long *moves, double *device_ms);
/* Counters of the Or-opt phases of the last alg_oropt / alg_2opt_oropt call of this thread (rounds = 0 after alg_oropt);
 * the 2-opt phases of alg_2opt_oropt go to tsp_host_last_stats. */
void tsp_host_last_or_stats(tsp_or_opt_stats *out);
/* Counters of the last alg_nl_opt call of this thread. */
void tsp_host_last_nl_stats(tsp_nl_opt_stats *out);
/* Counters of the last alg_3opt call of this thread. */
void tsp_host_last_nl3_stats(tsp_nl3_opt_stats *out);
/* Counters of the winning chain of the last alg_ils call of this thread. */
void tsp_host_last_ils_stats(tsp_ils_stats *out);
/* active_nodes and closing_scans of the last alg_3opt or alg_ils call of this thread (0 under TSP_DLB_OFF); either may be NULL. */
void tsp_host_last_dlb_stats(int64_t *active_nodes, int64_t *closing_scans);
/* Counters of the last tsp_host_lower_bound call of this thread. */
void tsp_host_last_lb_stats(tsp_lb_stats *out);
/* Counters of the last tsp_host_lower_bound_sparse call of this thread. */
void tsp_host_last_lb_sparse_stats(tsp_lb_sparse_stats *out);
/* Counters of the last HEU_greedy_edge call of this thread (also through HEU_2opt_ / HEU_nl_ / HEU_ils_greedy_edge). */
void tsp_host_last_greedy_edge_stats(tsp_greedy_edge_stats *out);
/* Counters of the last alg_seg_ils call of this thread (also through HEU_seg_ils_greedy_edge). */
void tsp_host_last_seg_ils_stats(tsp_seg_ils_stats *out);
/* ... with the counters of the 3-opt kind behind them (all 0 when the call ran without it). */
void tsp_host_last_seg_ils3_stats(tsp_seg_ils3_stats *out);
/* ... and groups, offers and commits behind those (all 0 when the call ran under tsp_host_set_seg_ils_groups(1)). */
void tsp_host_last_seg_ils_groups_stats(tsp_seg_ils_groups_stats *out);
/* ... and the chain counters behind those (all 0 when the call ran under tsp_host_set_seg_ils_lk(0)). */
void tsp_host_last_seg_ils_lk_stats(tsp_seg_ils_lk_stats *out);
/* Counters of this thread's last merge: tsp_host_gpx, or the last round of an alg_seg_ils call with more than one chain. */
void tsp_host_last_gpx_stats(tsp_gpx_stats *out);
/* Releases the cached device context / instances (optional; also done at exit). */
void tsp_host_shutdown(void);

#ifdef __cplusplus
}
#endif
#endif
