/*
 * emat_host.h -- C-ABI of the host-side driver that sits ABOVE the engine boundary
 * (include/emat_backend.h): the part of Delphy's `Run` that the north star keeps on the host.
 *
 *   reference                                              here
 *   ---------                                              ----
 *   generate_random_partition_stencil, partition_tree      emat_run_repartition
 *     (core/tree_partitioning.h:139-239)
 *   Run::repartition (core/run.cpp:110-193)                emat_run_repartition
 *   Run::push_global_params_to_subruns (run.cpp:267-275)   emat_run_push_params
 *   Run::run_local_moves (run.cpp:682-693)                 emat_run_moves        -> emat_run_moves_even of the backend (remainder spread over the parts)
 *   Run::reassemble (run.cpp:195-256)                      emat_run_reassemble
 *   Run::do_mcmc_steps without the global moves            emat_run_do_mcmc_steps
 *     (run.cpp:622-657; the global moves' four groups, each off by default, are further down)
 *   Run::alpha_moves, gibbs_sample_all_nus                 emat_run_site_rate_moves  -> emat_site_rate_moves of the backend
 *     (run.cpp:1105-1235)
 *   Run::mu_move, hky_frequencies_move, hky_kappa_move     emat_run_subst_moves      -> emat_parts_subst_moves of the backend
 *   Run::set_mpox_hack_enabled, mpox_hack_moves            emat_run_set_mpox, emat_run_mpox_moves -> emat_parts_mpox_moves of the backend
 *     (run.cpp:781-821, :953-1103)
 *
 * Also exports the seeded synthetic-EMAT generator used by the bench and the tests
 * (SURVEY section 8(d) configs C1..C5).
 */
#ifndef EMAT_HOST_H_
#define EMAT_HOST_H_

#include "emat_backend.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- synthetic EMATs ------------------------------------------------------------------------ */
typedef struct emat_synth_params {
  int32_t num_tips;
  int32_t num_sites;
  double tip_span;              /* tip dates ~ U[0, tip_span) days */
  double tip_date_uncertainty;  /* half-width of [t_min, t_max] for the uncertain tips */
  double frac_uncertain_tips;
  double pop_n0;                /* N(t0) * generation time at the latest tip, days */
  double pop_growth;            /* per day */
  double mu;                    /* substitutions / site / day */
  double kappa;
  double pi[4];
  int32_t gaps_per_tip;
  double mean_gap_len;
  uint64_t seed;
} emat_synth_params;

typedef struct emat_synth emat_synth;
emat_status emat_synth_create(const emat_synth_params* p, emat_synth** out);
void emat_synth_destroy(emat_synth* s);
/* Pointers stay valid until emat_synth_destroy. */
emat_status emat_synth_get(emat_synth* s, emat_flat_tree* tree_view, const uint8_t** ref_sequence, double* t_max_tip);

/* ---- host tree container + partitioning (usable without any GPU) -------------------------------- */
typedef struct emat_run emat_run;

/* `backend` may be NULL: the driver then only partitions / reassembles (CPU tests, and feeding the
 * parity oracle with exactly the same subtrees as the HIP engine). */
emat_status emat_run_create(emat_backend* backend, const emat_flat_tree* tree, const uint8_t* ref_sequence,
                            int32_t num_sites, uint64_t seed, emat_run** out);
emat_status emat_run_destroy(emat_run* r);
const char* emat_run_last_error(const emat_run* r);

/* reference Run::set_num_parts (run.h:46-47) */
emat_status emat_run_set_num_parts(emat_run* r, int32_t num_parts);
/* NOT in the reference: at every repartition, parts of more than `max_nodes` nodes get further cut nodes, because on the GPU a pass
 * lasts as long as the chain of its largest part, and the parts of a stencil drift apart in size while it is in use (run.cpp:87-108
 * redraws stencils every 200 cycles only).  The extra cut nodes are drawn uniformly at random among the part's inner nodes -- a rule
 * that reads nothing a pass can change, so that it leaves the sampler's stationary distribution alone (emat_run_partition.hpp, refine_stencil).
 * 0 (the DEFAULT since round 6) = off: the reference's rule exactly, so that a run that sets nothing reproduces the reference's (and the
 * oracle's) partition; -1 = three times the mean part size, at least 64 (what bench.py's `inclusive` and the posterior scripts opt into);
 * > 0 = that many nodes. */
emat_status emat_run_set_max_part_nodes(emat_run* r, int32_t max_nodes);
/* Test hook of the rule above: the (sorted) cut nodes that the last repartition's draw -- same stencil, same random stream of the
 * refinement -- gives on the tree as it is NOW.  A pass only moves nodes within parts and the rule reads nothing such a pass changes, so
 * after emat_run_reassemble the answer must be what it was right after emat_run_repartition (tests/test_host_driver.py): the premise of
 * the argument that the limit cannot bias the sampler.  `*num_cut_nodes`: capacity in, count out.  Changes no state. */
emat_status emat_run_debug_redraw_partition(emat_run* r, int32_t* cut_nodes, int32_t* num_cut_nodes);
/* The last repartition: how many parts, the node count of the largest, how many cut nodes the rule above added, the limit in effect. */
emat_status emat_run_partition_stats(emat_run* r, int32_t* num_parts, int32_t* largest_part_nodes, int32_t* extra_cuts, int32_t* max_part_nodes_in_effect);
/* HKY substitution model with per-site relative rates nu_l (NULL = all 1): reference Hky_model +
 * Run::derive_evo (evo_hky.cpp:7-50).  One site partition. */
emat_status emat_run_set_hky(emat_run* r, double mu, double kappa, const double pi[4], const double* nu_l);
emat_status emat_run_set_pop_model(emat_run* r, const emat_pop_model* pm);
emat_status emat_run_set_coalescent_t_step(emat_run* r, double t_step);
emat_status emat_run_set_flags(emat_run* r, int32_t only_displacing_inner_nodes, int32_t topology_moves_enabled);
/* How emat_run_moves / emat_run_do_mcmc_steps split `count` moves over P parts.  Default (0): count / P on every part and the
 * remainder one move each on the first parts -- NOT the reference's rule, which gives the whole remainder to subrun 0
 * (Run::run_local_moves, run.cpp:683-689): harmless with 8 parts, but with thousands of parts it makes part 0 the longest
 * chain of every pass by a factor of several.  1: the reference's rule, for runs that must reproduce its per-part move counts
 * (emat_run_local_moves of the backend).  Sharded runs (emat_run_moves_sharded) always spread. */
emat_status emat_run_set_reference_remainder(emat_run* r, int32_t on);
/* Run::set_paranoid (reference run.h:220-224; CLI flag --v0-paranoid, cmdline.cpp:177): emat_run_do_mcmc_steps then runs
 * emat_check_derived on every part after every pass of local moves and stops with its error if one is off. */
emat_status emat_run_set_paranoid(emat_run* r, int32_t on);

/* keep the authoritative tree in HBM (emat_tree_* of the backend).  From the next emat_run_repartition on,
 * a cycle moves only the partition to the device and topology + node times back: emat_run_repartition draws and applies
 * the stencil on the topology and calls emat_tree_repartition, emat_run_reassemble calls emat_tree_reassemble (which also
 * does Run::normalize_root's work).  emat_run_tree_get / emat_run_tree_sizes download the tree when asked;
 * emat_run_part_* (host copies of the parts) are not available.  Same seeds, same partitions, same trees as the host
 * cycle, bit for bit.  `on` = 0 brings the tree back to the host. */
emat_status emat_run_set_device_tree(emat_run* r, int32_t on);
/* A sharded run with the tree on the devices: emat_run_repartition cuts every process's own block of parts out of its own
 * copy of the tree (emat_tree_repartition_range); the gather goes through the backend's staged calls with the caller's
 * exchange between them (emat_backend.h: emat_tree_get_root_deltas ... emat_tree_reassemble_end; delphy_amd/sharding.py),
 * after which this tells the driver that the parts are back and which sites of the reference sequence changed. */
emat_status emat_run_note_device_reassembled(emat_run* r, int32_t num_root_deltas, const int32_t* site, const uint8_t* to);
/* Cut the tree into parts and (when a backend is attached) upload them and build their coalescent parts. */
emat_status emat_run_repartition(emat_run* r);
emat_status emat_run_num_parts(emat_run* r, int32_t* num_parts, int32_t* root_part_index);
/* Sizes / contents of part i as built by the last repartition (to feed another engine, e.g. the oracle). */
emat_status emat_run_part_sizes(emat_run* r, int32_t part, int32_t* num_nodes, int32_t* num_muts, int32_t* num_intervals, int32_t* num_from_states);
emat_status emat_run_part_get(emat_run* r, int32_t part, emat_flat_tree* out, int32_t* includes_run_root, uint64_t* seed);
/* Replace part i's subtree (e.g. with what another engine computed) before emat_run_reassemble. */
emat_status emat_run_part_put(emat_run* r, int32_t part, const emat_flat_tree* subtree);

emat_status emat_run_push_params(emat_run* r);
emat_status emat_run_moves(emat_run* r, int64_t count);
/* Gather the parts back into the whole tree; with a backend attached the parts are downloaded first. */
emat_status emat_run_reassemble(emat_run* r);
/* Several drivers in ONE process that are bound to draw the same partitions (same seed, same tree, same settings: the shards of
 * emat_run_create_multi) draw once: a follower takes the cut nodes its leader drew for the cycle instead of picking and refining the
 * stencil again on the same host cores.  The leader draws at its own emat_run_repartition, or ahead of it with emat_run_draw_partition,
 * after which leader and followers can cut side by side.  (Not in the reference, whose Run is one object; its refresh_partition_stencils
 * + pick, run.cpp:87-108, 127-129, is what is being shared.) */
emat_status emat_run_follow_draws(emat_run* follower, emat_run* leader /* NULL: draw for itself again */);
emat_status emat_run_draw_partition(emat_run* leader);
/* ---- one run over several processes, one GPU each ---------------------------------------------------
 * Every process creates the same run (same tree, same seed) with its own backend and calls emat_run_set_shard once.
 * The partition is then computed identically everywhere, but a process uploads only its contiguous block of parts
 * (emat_run_shard_range; backend part id = part - part_lo).  One cycle (reference run.cpp:622-657) is
 *
 *   emat_run_repartition                                     every rank, no communication
 *   emat_run_coalescent_begin -> all-reduce MIN / MAX        the staged form of emat_build_coalescent_parts
 *   emat_coalescent_set_range / _local_grid -> all-reduce SUM / _sample -> all-reduce SUM / _finish   (on the backend)
 *   emat_run_moves_sharded(count)                            count / parts moves on every part of the run, the remainder one move each on the first parts
 *   emat_run_pack_local_parts -> all-gather of the byte buffers -> emat_run_unpack_parts for every other rank's buffer
 *   emat_run_reassemble                                      every rank ends up with the same whole tree
 *   emat_get_totals on the backend -> all-reduce SUM (2 doubles)
 *
 * The collectives (RCCL over xGMI, or gloo in tests) belong to the caller: delphy_amd/sharding.py drives them through
 * torch.distributed.  emat_run_do_mcmc_steps is the single-process cycle and refuses a sharded run. */
emat_status emat_run_set_shard(emat_run* r, int32_t rank, int32_t world);
emat_status emat_run_shard_range(emat_run* r, int32_t* part_lo, int32_t* part_hi, int32_t* local_root_part /* -1: the root part lives on another rank */);
emat_status emat_run_coalescent_begin(emat_run* r, double* local_t_min, double* local_t_max);
emat_status emat_run_moves_sharded(emat_run* r, int64_t count);
/* Serialises this rank's parts as they are on its device now.  Call with buf = NULL to learn the size. */
emat_status emat_run_pack_local_parts(emat_run* r, uint8_t* buf, uint64_t capacity, uint64_t* bytes_needed);
emat_status emat_run_unpack_parts(emat_run* r, const uint8_t* buf, uint64_t bytes);

/* ---- one run over several GPUs of ONE process (delphy_amd/csrc/emat_multi.cpp) --------------------------------------------
 * replaces: the thread pool behind Run::run_local_moves (reference core/run.cpp:682-693: one task per Subrun, in-process) for a
 * C++ `Run` that owns several MI355X.  n backends, one per entry of `devices` (cfg->device is ignored), every one with the whole
 * tree in its HBM and a contiguous block of the partition's parts; the exchanges of a sharded cycle (above) are done inside, in
 * C++: an all-gather of what every shard's parts own -- emat_tree_export_nodes writes into the device buffer that
 * ncclAllGather sends over xGMI, emat_tree_apply_nodes reads what arrived -- and an ncclAllReduce of the two log-posterior
 * totals.  `exchange`: EMAT_EXCHANGE_RCCL (librccl.so is loaded at run time with dlopen: no link-time dependency),
 * EMAT_EXCHANGE_HOST (the same steps through host buffers: what two backends sharing one device must use, RCCL taking one
 * rank per device), or EMAT_EXCHANGE_AUTO (RCCL when every shard has a device of its own and the library loads).
 * One cycle = emat_multi_repartition, emat_multi_run_moves (returns with the kernels of every GPU in flight),
 * emat_multi_reassemble; emat_multi_do_mcmc_steps strings them together as Run::do_mcmc_steps does (run.cpp:622-657, without the
 * global moves).  The shards' own handles stay reachable for everything else (emat_multi_backend / emat_multi_shard: statistics of
 * the global moves, paranoid checks, part downloads).  Entry points are not thread-safe with respect to each other. */
typedef struct emat_multi emat_multi;
enum { EMAT_EXCHANGE_HOST = 0, EMAT_EXCHANGE_RCCL = 1, EMAT_EXCHANGE_AUTO = 2 };
emat_status emat_run_create_multi(const int32_t* devices, int32_t n, const emat_config* cfg, const emat_flat_tree* tree, const uint8_t* ref_sequence,
                                  int32_t num_sites, uint64_t seed, int32_t exchange, emat_multi** out);
emat_status emat_multi_destroy(emat_multi* m);
const char* emat_multi_last_error(const emat_multi* m);
const char* emat_multi_exchange(const emat_multi* m);          /* what the exchange goes through, in words */
int32_t emat_multi_num_shards(const emat_multi* m);
emat_backend* emat_multi_backend(emat_multi* m, int32_t shard);
emat_run* emat_multi_shard(emat_multi* m, int32_t shard);
emat_status emat_multi_set_num_parts(emat_multi* m, int32_t num_parts);
emat_status emat_multi_set_max_part_nodes(emat_multi* m, int32_t max_nodes);
emat_status emat_multi_set_option(emat_multi* m, const char* key, const char* value);   /* emat_set_option on every shard's backend */
/* Which RCCL to dlopen (name or path) instead of the usual names; process-wide, before emat_run_create_multi; NULL = the usual names. */
emat_status emat_multi_set_rccl_library(const char* name);
emat_status emat_multi_debug_rccl_load(char* err, int32_t err_cap);   /* test hook: EMAT_OK if RCCL loads with the present setting, else EMAT_ERR_HIP and why */
emat_status emat_multi_set_hky(emat_multi* m, double mu, double kappa, const double pi[4], const double* nu_l);
emat_status emat_multi_set_pop_model(emat_multi* m, const emat_pop_model* pm);
emat_status emat_multi_set_coalescent_t_step(emat_multi* m, double t_step);
emat_status emat_multi_set_flags(emat_multi* m, int32_t only_displacing_inner_nodes, int32_t topology_moves_enabled);
emat_status emat_multi_set_paranoid(emat_multi* m, int32_t on);
emat_status emat_multi_repartition(emat_multi* m);
emat_status emat_multi_run_moves(emat_multi* m, int64_t count);
emat_status emat_multi_check_derived(emat_multi* m, double tol_scale);
emat_status emat_multi_reassemble(emat_multi* m);
emat_status emat_multi_get_totals(emat_multi* m, double* log_G, double* log_augmented_coalescent_prior);
emat_status emat_multi_do_mcmc_steps(emat_multi* m, int64_t steps, int64_t local_moves_per_cycle);
emat_status emat_multi_tree_sizes(emat_multi* m, int32_t* num_nodes, int32_t* num_muts, int32_t* num_intervals, int32_t* num_from_states);
emat_status emat_multi_tree_get(emat_multi* m, int32_t shard, emat_flat_tree* out, uint8_t* ref_sequence /*[L]*/);

/* replaces: calc_Ttwiddle_l(tree_, evo_) (reference phylo_tree_calc.cpp:176-222, called at run.cpp:1109, 1184) while the parts
 * are on the device: the driver knows the tree of parts, which the staged engine calls need (emat_backend.h).  Single process;
 * a sharded run all-gathers emat_get_part_tree_lengths, calls emat_run_Ttwiddle_ext + emat_Ttwiddle_l_partial on every rank,
 * all-reduces S, R and the root's tree length, and finishes anywhere. */
emat_status emat_run_get_Ttwiddle_l(emat_run* r, double* Ttwiddle_l /*[num_sites]*/);
emat_status emat_run_Ttwiddle_ext(emat_run* r, const double* tree_length_of_part /*[all parts of the run]*/, int32_t* ext_offset /*[local parts + 1]*/,
                                  int32_t* ext_node, double* ext_length, int32_t capacity, int32_t* count);

/* The site-rate moves in the run (reference Run::alpha_moves + gibbs_sample_all_nus, run.cpp:1105-1235; engine call:
 * emat_site_rate_moves of emat_backend.h).  Off by default: a run without them keeps the nu_l of emat_run_set_hky.
 *   emat_run_set_site_rate_moves  on / off, and the alpha the steps start from (the reference's default is 1.0; finite, > 0).
 *   emat_run_site_rate_moves      one round while the parts are out, like emat_run_get_Ttwiddle_l: Ttwiddle_l as that call computes
 *                                 it, the mutations per site (emat_get_num_muts_l), ten alpha steps and the draw of every nu_l, with
 *                                 key = the first 64-bit word of Philox4x32-10(counter = rounds so far, key = run seed ^ a fixed tag).
 *                                 alpha and nu_l are kept in the driver, so that the next emat_run_push_params sends the same
 *                                 values.  `out` may be NULL.  A sharded run gets EMAT_ERR_STATE: its caller owns the collectives
 *                                 and calls the engine itself with the summed statistics.
 *   emat_run_get_site_rates       alpha and nu_l as the driver holds them (either pointer may be NULL).
 * With the moves on, emat_run_do_mcmc_steps does one round per cycle where the reference runs its global moves: after the
 * repartition and before the cycle's local moves (run.cpp:635-641).  With them off the cycle is what it was. */
emat_status emat_run_set_site_rate_moves(emat_run* r, int32_t on, double alpha /* start value, reference default 1.0 */);
emat_status emat_run_site_rate_moves(emat_run* r, emat_site_rate_result* out /* may be NULL */);   /* needs the parts out, like emat_run_get_Ttwiddle_l */
emat_status emat_run_get_site_rates(emat_run* r, double* alpha, double* nu_l /* either may be NULL */);

/* The Skygrid population moves of a run (Run::skygrid_tau_move, skygrid_gammas_zero_mode_gibbs_move, skygrid_gammas_hmc_move, reference
 * run.cpp:766-778; emat_skygrid_moves / emat_tree_skygrid_moves of emat_backend.h).  Off by default: a run without them keeps the curve of
 * emat_run_set_pop_model for ever, and its cycle's code path is what it was.
 *   emat_run_set_skygrid_moves  on / off, and Run's Skygrid settings with the tau to start from (EMAT_ERR_INVALID_ARGUMENT: what
 *                               emat_skygrid_moves refuses in a spec).
 *   emat_run_skygrid_moves      one round on the ASSEMBLED tree -- EMAT_ERR_STATE while the parts are out, the opposite of
 *                               emat_run_site_rate_moves.  With the tree in HBM: emat_tree_skygrid_moves, the statistics never leave the device;
 *                               with the tree on the host: the lineage grid and the coalescence times made from it here, then emat_skygrid_moves.
 *                               t_ref is the latest tip bound (calc_max_tip_time), t_step the coalescent step of the parts.  The key of round k is
 *                               the first word of Philox(counter k, key = run seed ^ a fixed tag), as for the site rates.  The accepted curve and
 *                               tau become the run's, and the next repartition builds the parts' coalescent tables from them.  `out` (may be NULL):
 *                               out->gamma and out->trace may each be NULL.  A sharded run is refused as the site-rate moves refuse it.
 *   emat_run_get_skygrid        the curve's gammas and tau as the run holds them (either pointer may be NULL).
 * With the group on, emat_run_do_mcmc_steps does one round at the top of every cycle, BEFORE the repartition.  The reference runs its
 * global moves on the whole tree right after ITS repartition and rebuilds the parts' coalescent tables afterwards (run.cpp:635-647,
 * :267-275); this driver's repartition builds those tables itself, so moving first gives the parts the new curve in one build. */
emat_status emat_run_set_skygrid_moves(emat_run* r, int32_t on, const emat_skygrid_spec* spec);
emat_status emat_run_skygrid_moves(emat_run* r, emat_skygrid_result* out /* may be NULL */);   /* needs the tree assembled */
emat_status emat_run_get_skygrid(emat_run* r, double* gamma /*[knots]*/, double* tau /* either may be NULL */);

/* The Exponential population moves of a run (Run::pop_size_move, pop_growth_rate_move, reference run.cpp:754-764, :1237-1319;
 * emat_exp_pop_moves / emat_tree_exp_pop_moves of emat_backend.h).  Off by default: a run without them keeps the n0 and g of
 * emat_run_set_pop_model for ever, and its cycle's code path is what it was.
 *   emat_run_set_exp_pop_moves  on / off, and Run's settings for the two moves with the number of rounds (50 in the reference)
 *                               (EMAT_ERR_INVALID_ARGUMENT: what emat_exp_pop_moves refuses in a spec).
 *   emat_run_exp_pop_moves      one call of `rounds` rounds on the ASSEMBLED tree -- EMAT_ERR_STATE while the parts are out -- exactly as
 *                               emat_run_skygrid_moves: emat_tree_exp_pop_moves with the tree in HBM, else the statistics made here and
 *                               emat_exp_pop_moves; the same t_ref and t_step; the key of call k is the first word of Philox(counter k,
 *                               key = run seed ^ a fixed tag of its own).  The accepted n0 and g become the run's, and the next repartition
 *                               builds the parts' coalescent tables from them.  `out` (may be NULL): out->trace may be NULL.  A sharded run is
 *                               refused as the site-rate moves refuse it; a model that is not exponential is EMAT_ERR_INVALID_ARGUMENT.
 *   emat_run_get_exp_pop        n0 and g as the run holds them (either pointer may be NULL).
 * With the group on, emat_run_do_mcmc_steps does one call at the top of every cycle, BEFORE the repartition, as for the Skygrid. */
emat_status emat_run_set_exp_pop_moves(emat_run* r, int32_t on, const emat_exp_pop_spec* spec);
emat_status emat_run_exp_pop_moves(emat_run* r, emat_exp_pop_result* out /* may be NULL */);   /* needs the tree assembled */
emat_status emat_run_get_exp_pop(emat_run* r, double* n0, double* g /* either may be NULL */);

/* The substitution-model moves of a run (Run::mu_move, hky_frequencies_move, hky_kappa_move, reference run.cpp:703-719, :781-821,
 * :953-1103; emat_parts_subst_moves of emat_backend.h).  Off by default: a run without them keeps the mu, kappa and pi of
 * emat_run_set_hky for ever, and its cycle's code path is what it was.
 *   emat_run_set_subst_moves  on / off, and Run's mu prior, the three switches and the number of rounds (10 in the reference).  mu, kappa
 *                             and pi of the spec are ignored: the run's own are used.  EMAT_ERR_INVALID_ARGUMENT: what emat_subst_moves
 *                             refuses in the rest of a spec, or more rounds than it holds.
 *   emat_run_subst_moves      one call while the parts are out, like emat_run_site_rate_moves (EMAT_ERR_STATE on an assembled tree): the
 *                             statistics of the parts never leave the device; the key of call k is the first word of Philox(counter k,
 *                             key = run seed ^ a fixed tag of its own).  The accepted mu, kappa and pi become the run's -- the backend
 *                             holds them already, and the next emat_run_push_params sends the same.  `out` (may be NULL): out->trace may
 *                             be NULL.  A sharded run is refused as the site-rate moves refuse it.
 *   emat_run_get_hky          mu, kappa and pi[4] as the run holds them (any pointer may be NULL).
 * With the group on, emat_run_do_mcmc_steps makes one call per cycle after the repartition and BEFORE the site-rate round, the
 * reference's order (run.cpp:703-732): the site-rate round's Ttwiddle_l is made from the new q. */
emat_status emat_run_set_subst_moves(emat_run* r, int32_t on, const emat_subst_spec* spec);
emat_status emat_run_subst_moves(emat_run* r, emat_subst_result* out /* may be NULL */);   /* needs the parts out */
emat_status emat_run_get_hky(emat_run* r, double* mu, double* kappa, double* pi /*[4]; any may be NULL */);

/* The APOBEC (mpox) model of a run (Run::set_mpox_hack_enabled, reference run.cpp:359-398; Run::derive_evo's second arm, :405-432;
 * Run::mpox_hack_moves, :823-951; emat_parts_mpox_moves of emat_backend.h).  Off by default: a run without it is what it was.
 *   emat_run_set_mpox            on: the sites are cut into two partitions by the APOBEC context (:370-382) of the sequence at node 0 of the
 *                                run's tree -- the reference sequence with the mutations on the path from the root down to node 0 applied
 *                                in order, missations ignored, as view_of_sequence_at does; host work, once per run (a tree resident in HBM
 *                                is brought to the host for it).  mu starts at the run's HKY mu and mu* at spec->mu_star (the reference: 0);
 *                                do_mu, rounds (10 in the reference) and the mu prior are the group's switches; mu of the spec is ignored.
 *                                From then on emat_run_push_params sends two partitions with mpox_derive_q(mu* / mu), and the run's kappa
 *                                and pi rest.  On a run that has the model on already only the switches are taken.  EMAT_ERR_STATE: node 0
 *                                is not a tip; the parts are out (reassemble first); no emat_run_set_hky yet; the substitution-model moves
 *                                are on -- and emat_run_set_subst_moves(on) and emat_run_subst_moves are refused likewise while the model is
 *                                on: the two groups are the two arms of one branch (:703-719).  EMAT_ERR_INVALID_ARGUMENT: what
 *                                emat_mpox_moves refuses in the rest of a spec, more rounds than it holds, or a run's mu that is not positive.
 *                                off (spec may be NULL): one partition again, and mu goes back to the HKY model (:391-395).
 *   emat_run_mpox_moves          one call while the parts are out, like emat_run_subst_moves: the statistics of the parts never leave the
 *                                device; the key of call k is the first word of Philox(counter k, key = run seed ^ a fixed tag of its own).
 *                                The new mu and mu* become the run's.  `out` (may be NULL): out->trace may be NULL.  A sharded run is
 *                                refused as the site-rate moves refuse it.
 *   emat_run_get_mpox            mu and mu* as the run holds them (either may be NULL); EMAT_ERR_STATE with the model off.
 *   emat_run_get_mpox_partition  the partition drawn at enabling and how many sites have APOBEC context (either may be NULL).
 * With the model on, emat_run_do_mcmc_steps makes one call per cycle where it makes the substitution-model moves' call. */
emat_status emat_run_set_mpox(emat_run* r, int32_t on, const emat_mpox_spec* spec);
emat_status emat_run_mpox_moves(emat_run* r, emat_mpox_result* out /* may be NULL */);   /* needs the parts out */
emat_status emat_run_get_mpox(emat_run* r, double* mu, double* mu_star);
emat_status emat_run_get_mpox_partition(emat_run* r, int32_t* partition_for_site /*[L]*/, int32_t* count);

/* [Skygrid or Exponential population moves when on] -> repartition -> [push params, substitution-model moves when on, site-rate moves
 * when on, local moves, reassemble] per cycle of `local_moves_per_cycle` moves (<= 0: 50 x nodes, the reference default
 * run.cpp:669-672), repartitioning at every cycle boundary. */
emat_status emat_run_do_mcmc_steps(emat_run* r, int64_t steps, int64_t local_moves_per_cycle);

/* Whole tree out (sizes first). The reference sequence may have been re-referenced to the root
 * sequence (Run::normalize_root, run.cpp:258-265). */
emat_status emat_run_tree_sizes(emat_run* r, int32_t* num_nodes, int32_t* num_muts, int32_t* num_intervals, int32_t* num_from_states);
emat_status emat_run_tree_get(emat_run* r, emat_flat_tree* out, uint8_t* ref_sequence /*[L]*/);
emat_status emat_run_t_max_tip(emat_run* r, double* t_max_tip);

/* ---- aligned FASTA in ------------------------------------------------------------------------------------------------------------
 * replaces: read_fasta (reference core/io.cpp:14-97) and the host's share of fasta_to_maple (core/cmdline.cpp:26-85); the rows themselves go
 * through the alignment store of the backend (include/emat_backend.h: emat_align_*), which forms the consensus and every tip's descriptors.
 *
 *   emat_seq_id_date_range   extract_date_range_from_sequence_id (core/sequence_utils.cpp:98-211): the date is a suffix of the id after '|' or
 *                            '-', in the forms YYYY-MM-DD/YYYY-MM-DD, YYYY-MM-DD, YYYY-MM, YYYY, tried in that order; times are days since
 *                            2020-01-01 (core/dates.cpp:12-46); a month or a year gives [its first day, the first day of the next].  *ok = 0
 *                            and EMAT_OK for an id without a date.  A month outside 1-12 or a day that the month does not have is no date:
 *                            the reference leaves such strings to absl::ParseCivilTime, and this one case is NOT verified against it.
 *   emat_fasta_frame_memory  frames the records of a text as read_fasta does -- empty lines and lines that begin with ';' are skipped; the id is
 *                            everything after '>' without the white space at its two ends (spaces inside belong to it); white space inside
 *                            sequence lines is skipped, a '\r' before the line end included; data before the first '>' is a record named "" --
 *                            and leaves their names, lengths and dates on the handle.  Needs no device.
 *   emat_fasta_load_memory   frames the text into one of two page-locked row buffers of `chunk_rows` rows (0: about 32 MB) while the other is on
 *                            its way through emat_align_push_rows, then calls emat_align_finish with given_ref ([L] of 0..3, or NULL for the
 *                            consensus) and row_dated from the ids.  It leaves on the handle the names, t_min / t_max as floats and the report;
 *                            the descriptors are the store's (emat_align_get).  On a handle without a device it frames the text, leaves that,
 *                            and returns EMAT_ERR_NO_DEVICE.
 *   emat_fasta_load          the same of a file (mapped, not gzip).  EMAT_ERR_IO when it cannot be opened or mapped.
 *   emat_fasta_sizes / _get  what the last of the three left: per record its name (NUL-terminated, back to back, names_bytes in all), the
 *                            number of its characters, t_min / t_max (NaN without a date) and whether it has a date; any pointer may be NULL.
 *
 * EMAT_ERR_INVALID_ARGUMENT (text in emat_last_error): a text without records ("Input has no sequences!"); a record whose length is not the
 * handle's L -- the text names it and the first record with their lengths, as fasta_to_maple's does.  The reference stops reading a record
 * at its first character that is no sequence letter and drops it whatever its length; here such a record must still have L characters,
 * and is then reported as invalid by the store.  EMAT_ERR_STATE: emat_fasta_sizes / emat_fasta_get before any of the three.  After any refusal
 * the next call works (the store is released). */
typedef struct emat_fasta_report {
  int32_t num_records;      /* framed */
  int32_t num_dated;        /* ... whose id ends in a date */
  int64_t names_bytes;      /* of all names with their NULs */
  emat_align_report rows;   /* emat_align_finish's (zeros after emat_fasta_frame_memory) */
} emat_fasta_report;
emat_status emat_seq_id_date_range(const char* id, double* t_min, double* t_max, int32_t* ok);
emat_status emat_fasta_frame_memory(emat_backend* h, const uint8_t* text, int64_t len, emat_fasta_report* out /* may be NULL */);
emat_status emat_fasta_load_memory(emat_backend* h, const uint8_t* text, int64_t len, const uint8_t* given_ref, int32_t chunk_rows, emat_fasta_report* out /* may be NULL */);
emat_status emat_fasta_load(emat_backend* h, const char* path, const uint8_t* given_ref, int32_t chunk_rows, emat_fasta_report* out /* may be NULL */);
emat_status emat_fasta_sizes(emat_backend* h, emat_fasta_report* out);
emat_status emat_fasta_get(emat_backend* h, char* names, int64_t* lengths, float* t_min, float* t_max, uint8_t* dated);

#ifdef __cplusplus
}
#endif
#endif /* EMAT_HOST_H_ */
