/*
 * emat_backend.h -- C-ABI of the MI355X-native EMAT local-move engine.
 *
 * This is the drop-in boundary for Delphy's per-iteration hot path.  The reference has no
 * FFI for this path; the seam is the C++ class `Subrun` as driven by `Run`
 * (reference core/subrun.h:16-135, core/run.cpp:110-293,610-693).  Every entry point below
 * names the reference interaction it replaces.  All functions return an `emat_status`
 * (0 = OK); nothing throws across the boundary; all pointers are plain host pointers and
 * the backend copies what it needs (the caller keeps ownership of its buffers).
 *
 * Conventions (reference core/tree.h:33-39, core/mutations.h:21-29, core/interval_set.h):
 *   - nodes are int32 indices local to the subtree, EMAT_NO_NODE = -1;
 *   - states are 0..3 = A,C,G,T (reference core/sequence.h `Real_seq_letter`);
 *   - mutations on a branch are sorted by (t, site); the subtree root's "mutations" are
 *     the deltas ref_sequence -> subroot sequence with t = -DBL_MAX;
 *   - missation intervals are sorted, disjoint, non-adjacent half-open [start,end).
 */
#ifndef EMAT_BACKEND_H_
#define EMAT_BACKEND_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EMAT_NO_NODE (-1)

typedef enum emat_status {
  EMAT_OK = 0,
  EMAT_ERR_INVALID_ARGUMENT = 1,
  EMAT_ERR_NO_DEVICE = 2,        /* HIP device / extension missing: the product path never falls back to CPU */
  EMAT_ERR_HIP = 3,
  EMAT_ERR_STATE = 4,            /* call sequence violated (e.g. run before upload) */
  EMAT_ERR_CAPACITY = 5,         /* a part ran out of slab space; see emat_part_get_status */
  EMAT_ERR_INTERNAL = 6,
  EMAT_ERR_BUFFER_TOO_SMALL = 7,
  EMAT_ERR_IO = 8                /* a file could not be opened, written in full, or closed (include/emat_dphy.h) */
} emat_status;

/* Flat (struct-of-arrays, CSR) image of one `Phylo_tree` (reference core/phylo_tree.h:14-64).
 * Used in both directions.  For downloads the caller provides the arrays and their capacities. */
typedef struct emat_flat_tree {
  int32_t num_nodes;
  int32_t root;
  int32_t* parent;       /* [num_nodes] */
  int32_t* child0;       /* [num_nodes], EMAT_NO_NODE for tips */
  int32_t* child1;       /* [num_nodes] */
  double*  t;            /* [num_nodes] */
  float*   t_min;        /* [num_nodes] tips: date bounds; inner nodes -FLT_MAX */
  float*   t_max;        /* [num_nodes] tips: date bounds; inner nodes +FLT_MAX */
  /* mutations, CSR by node */
  int32_t* mut_offset;   /* [num_nodes+1] */
  int32_t* mut_site;     /* [num_muts] */
  uint8_t* mut_from;     /* [num_muts] */
  uint8_t* mut_to;       /* [num_muts] */
  double*  mut_t;        /* [num_muts] */
  /* missation intervals, CSR by node */
  int32_t* miss_offset;  /* [num_nodes+1] */
  int32_t* miss_start;   /* [num_intervals] */
  int32_t* miss_end;     /* [num_intervals] */
  /* missation from_states (only sites whose state != ref_sequence), CSR by node */
  int32_t* mfs_offset;   /* [num_nodes+1] */
  int32_t* mfs_site;     /* [num_from_states] */
  uint8_t* mfs_state;    /* [num_from_states] */
  /* capacities of the variable-length arrays (used by downloads only) */
  int32_t cap_muts;
  int32_t cap_intervals;
  int32_t cap_from_states;
} emat_flat_tree;

/* Population model descriptor (reference core/pop_model.h:12-241). */
typedef enum emat_pop_model_kind {
  EMAT_POP_CONST = 0,            /* Const_pop_model{pop}                                  p[0]=pop */
  EMAT_POP_EXP = 1,              /* Exp_pop_model{t0, pop_at_t0, growth_rate, min_pop}    p[0..3]  */
  EMAT_POP_SKYGRID = 2           /* Skygrid_pop_model{x[], gamma[], type}                          */
} emat_pop_model_kind;

typedef struct emat_pop_model {
  int32_t kind;
  double  p[4];
  int32_t skygrid_type;          /* 1 = staircase, 2 = log-linear (reference pop_model.h:149-185) */
  int32_t skygrid_num_knots;     /* M+1 */
  const double* skygrid_x;       /* [num_knots] strictly increasing */
  const double* skygrid_gamma;   /* [num_knots] log N at knots */
} emat_pop_model;

typedef struct emat_config {
  int32_t device;                /* HIP device ordinal; -1 = host-only handle (uploads and coalescent staging work,
                                    every launch returns EMAT_ERR_NO_DEVICE: there is no CPU fallback) */
  int32_t num_sites;             /* L */
  int32_t max_parts;             /* upper bound on parts resident at once (0 = grow on demand) */
  double  slab_slack;            /* >=1: per-part working-set capacity as a multiple of its content (0 = default 3.0) */
  int32_t trace_moves;           /* >0: record the first N moves of every part in a trace ring (tests) */
  int32_t use_lds;               /* 1 = stage part working sets in LDS when they fit (default), 0 = always HBM */
} emat_config;

typedef struct emat_backend emat_backend;

/* ---- life cycle ------------------------------------------------------------------------- */
/* replaces: Subrun construction/destruction as a set (reference run.cpp:131,182-183) */
emat_status emat_backend_create(const emat_config* cfg, emat_backend** out);
emat_status emat_backend_destroy(emat_backend* h);
/* Tuning and test options of one handle, by name, set after emat_backend_create and before the first launch (defaults are what
 * bench.py measures; an unknown name is refused).  The library reads NO tuning from the environment (only EMAT_VERBOSE, which
 * makes it narrate on stderr -- or, with the value "spans", account for the host's time per named stretch of a cycle and print the
 * table when a handle is destroyed): an embedding process decides per handle.  The Python mirror forwards EMAT_<NAME> variables for
 * A/B scripts.
 *   "lds_classes"   percentile of part sizes the staging area must hold whole, default "60"; a comma list makes size classes
 *   "lds_max"       largest staging area in bytes (default 98304);  "lds_scratch"  extra LDS scratch arena per part (default 0)
 *   "giants"        0 disables the side launches;  "side_arena"  bytes of arena a part must be left with in the main area
 *   "chunks"        tickets per part and pass in the main class (default 4);  "ticket_taper"  0 = equal tickets
 *   "ticket_weights" "w1,w2,...";  "single_ticket_parts"  how many of the largest parts run a pass unsplit;  "parts_per_cu"
 *   "slack", "heap_per_node"   list-heap capacity = content x slack + bytes per node (3.0 / 64)
 *   "order_by_time" 1 = re-sort the launch order by measured chain times at every synchronisation
 *   "tree_host_coalescent"  1 = emat_tree_repartition builds the coalescent tables with the host's code (bit-identical to the host cycle)
 *   testing aids: "ticket_xcd_spread" (a part's tickets on different XCDs), "ticket_release" ("full": plain agent-scope releases),
 *   "tree_tight" (no spare room in the device tree), "build_blocks" (workgroups of the initial-tree builder),
 *   "no_uniform_sites" (1: the moves read the per-site partition and rate arrays even when the model is the reference's default of one
 *   site partition and nu_l == 1 everywhere, where the answers are known without a load: the A/B of that short cut, round 6),
 *   "debug_fail_gather" (1: the next deferred gather of the device-resident tree reports an inconsistency; may be set at any time);
 *   "mcc_table_log2" (log2 of the slots emat_mcc_derive's table of clade counts starts with, 0 = four per node: a small value makes it grow; may be set at any time);
 *   "samples_probe_chunk" (samples emat_tree_samples_probe_ancestors / emat_mcc_probe_ancestors and the site-state forms work on at a time, 0 = as many as fit: results do not depend on it; may be set at any time);
 *   "mcc_summary_chunk" (MCC nodes emat_mcc_node_times works on at a time, 0 = as many as fit: results do not depend on it; may be set at any time);
 *   profiling builds: "fn_min_lists", "phase_extra". */
emat_status emat_set_option(emat_backend* h, const char* key, const char* value);
/* Size of the library's host thread pool (per process, before its first parallel loop; 0 = default: min(cores, 16)). */
emat_status emat_set_host_threads(int32_t n);
const char* emat_last_error(const emat_backend* h);   /* human-readable text for the last failure */
/* First 16 hex digits of the SHA-256 of the sources the kernels of THIS library were compiled from (csrc/Makefile: DEVSRC, in
 * that order); "unstamped" for a build that bypassed the Makefile.  bench.py refuses a library whose id differs from the
 * sources beside it, and quotes a committed PMC profile only for the id the profile was measured on. */
const char* emat_build_id(void);

/* ---- shared, read-only inputs ----------------------------------------------------------- */
/* replaces: `subtree.ref_sequence = ref_seq` (reference run.cpp:139-140) */
emat_status emat_set_ref_sequence(emat_backend* h, const uint8_t* ref_sequence, int32_t num_sites);

/* replaces: Subrun::set_evo (reference subrun.h:29-30; evo_model.h:20-48).  q is row-major
 * q[beta][a][b] with q[a][a] = -sum_{b!=a} q[a][b].  Invalidates derived quantities. */
emat_status emat_set_evo(emat_backend* h, int32_t num_partitions, const double* mu /*[P]*/,
                         const double* pi /*[P][4]*/, const double* q /*[P][4][4]*/,
                         const double* nu_l /*[L]*/, const int32_t* partition_for_site /*[L]*/);

/* replaces: set_t_max_tip / set_only_displacing_inner_nodes / set_topology_moves_enabled
 * (reference subrun.h:24-40; pushed in run.cpp:267-275) */
emat_status emat_set_flags(emat_backend* h, double t_max_tip, int32_t only_displacing_inner_nodes,
                           int32_t topology_moves_enabled);

/* ---- parts ------------------------------------------------------------------------------ */
/* replaces: the loop that builds one Subrun per partition part (reference run.cpp:131-184).
 * Discards all resident parts, then expects exactly `num_parts` emat_part_upload calls
 * followed by emat_end_upload. */
emat_status emat_begin_upload(emat_backend* h, int32_t num_parts);
/* replaces: Subrun(bitgen, tree, includes_run_root, evo) (reference subrun.cpp:10-15).  `seed`
 * keys the part's counter-based RNG stream (the reference seeds one std::mt19937 per part,
 * run.cpp:112-114). */
/* Thread-safety: between emat_begin_upload and emat_end_upload, emat_part_upload may be called concurrently for
 * DISTINCT part ids; every other entry point expects one caller at a time per handle. */
emat_status emat_part_upload(emat_backend* h, int32_t part_id, const emat_flat_tree* subtree,
                             int32_t includes_run_root, uint64_t seed);
emat_status emat_end_upload(emat_backend* h);

/* replaces: Run::reset_very_scalable_coalescent_parts -> make_very_scalable_coalescent_prior_parts
 * + Subrun::set_coalescent_prior_part (reference run.cpp:277-293; very_scalable_coalescent.cpp:85-232).
 * Builds every part's k_bar_p / k_twiddle_bar_p and the shared k_twiddle_bar, popsize_bar,
 * num_active_parts from the resident subtrees.  Invalidates derived quantities. */
emat_status emat_build_coalescent_parts(emat_backend* h, const emat_pop_model* pop_model,
                                        int32_t root_part_index, double t_step);

/* Staged form of emat_build_coalescent_parts for a run whose parts are sharded over several GPUs (one
 * process per GPU).  Between the stages the caller all-reduces tiny vectors over RCCL:
 *   begin       -> this rank's [t_min, t_max]                       -> all-reduce MIN / MAX
 *   set_range   -> number of grid cells
 *   local_grid  -> this rank's k_bar / num_active_parts             -> all-reduce SUM   (very_scalable_coalescent.cpp:153-188)
 *   sample      -> this rank's share of k_twiddle_bar (Gaussian draws from each part's stream, :198-219) -> all-reduce SUM
 *   finish      -> every resident part gets its Very_scalable_coalescent_prior_part
 * `root_part_index` is -1 on ranks that do not hold the run's root part. */
emat_status emat_coalescent_begin(emat_backend* h, const emat_pop_model* pop_model, int32_t root_part_index, double t_step,
                                  double* local_t_min, double* local_t_max);
emat_status emat_coalescent_set_range(emat_backend* h, double all_t_min, double all_t_max, int32_t* num_cells);
emat_status emat_coalescent_local_grid(emat_backend* h, double* k_bar /*[num_cells]*/, int32_t* num_active_parts /*[num_cells]*/);
emat_status emat_coalescent_sample(emat_backend* h, const double* k_bar, const int32_t* num_active_parts, double* k_twiddle_bar_local /*[num_cells]*/);
emat_status emat_coalescent_finish(emat_backend* h, const double* k_twiddle_bar /*[num_cells]*/);

/* ---- the hot path ----------------------------------------------------------------------- */
/* replaces: Run::run_local_moves(count) (reference run.cpp:682-693): `count / num_parts` calls of
 * Subrun::mcmc_sub_iteration() on every part, the remainder going to part 0.  Asynchronous with
 * respect to the host; emat_synchronize (or any getter) waits. */
emat_status emat_run_local_moves(emat_backend* h, int64_t count);
/* Same, with an explicit number of moves per part (all parts the same). */
emat_status emat_run_moves_per_part(emat_backend* h, int64_t moves_per_part);
/* Same, plus `extra_moves_part0` more on this handle's part 0: the split of Run::run_local_moves when the run's parts are
 * spread over several handles (the handle holding the run's part 0 gets the remainder). */
emat_status emat_run_moves_split(emat_backend* h, int64_t moves_per_part, int64_t extra_moves_part0);
/* NOT the reference's rule: `moves_per_part` moves on every part and one more on the parts [0, one_more_below).  The
 * reference hands the whole remainder of count / parts to subrun 0 -- at most parts - 1 moves, nothing next to a subrun's
 * share at 8 threads, but six times a part's share at 8 000 parts, where that one chain then sets the length of the pass
 * (measured at C4: 62 ms instead of 34).  Spreading the remainder one move per part runs the same total. */
emat_status emat_run_moves_even(emat_backend* h, int64_t moves_per_part, int32_t one_more_below);
/* Waits for the launches issued so far and checks that every part ran its chain to completion.  The reference's containers
 * grow without bound; a slab has fixed room.  A part that runs out of it -- list heap, scratch, or the cells the root part's
 * coalescent grid grows into the past -- is re-materialised with more room (twice; four times the cells) and the rest of
 * its moves run, transparently, up to four times (then EMAT_ERR_CAPACITY): it either stopped BEFORE a move (the heap
 * reserve is checked there, and the moves that can grow the grid ask before they change anything), or a container
 * overflowed INSIDE a move and the state its leg started from was put back (the untouched HBM copy of a staged part, a
 * shadow copy for a part run on its HBM slab).  Either way the chain continues exactly as it would have with unbounded
 * containers.  A part that broke an invariant the reference CHECKs makes this -- and every getter, all of which
 * synchronise first -- fail with EMAT_ERR_INTERNAL naming the part and the device source line; the reference aborts in that
 * situation. */
emat_status emat_synchronize(emat_backend* h);

/* ---- The whole tree resident in HBM -------------------------------------------------------------
 * Run::repartition (core/run.cpp:110-193) copies every part out of the whole Phylo_tree into its Subrun's tree and
 * Run::reassemble (core/run.cpp:195-256) copies the parts back; through emat_part_upload / emat_part_download that is a
 * host round trip of every node, mutation and missation per cycle.  With the tree uploaded ONCE, a cycle needs from the
 * host only the partition itself -- which nodes form which part -- and moves topology + node times (a few MB) back:
 *
 *   emat_tree_upload            the whole tree -> HBM (node arrays + three record heaps); the root node must carry no
 *                               mutations (Run::normalize_root, run.cpp:258-265)
 *   emat_tree_get_topology      parent / children / node times / root, as of the last upload or reassemble: what
 *                               generate_random_partition_stencil and partition_tree (tree_partitioning.h:88-239) read
 *   emat_tree_repartition       run.cpp:110-193 + reset_very_scalable_coalescent_parts (run.cpp:277-293): the parts as
 *                               CSR over part-local nodes -- `orig` maps a part's node to the tree's node, local node 0
 *                               being the part's cut point, `kid0` / `kid1` are part-local children (EMAT_NO_NODE at the
 *                               part's tips).  One kernel computes the sequence state at every cut point
 *                               (phylo_tree_calc.cpp:19-56) and sizes the parts, a second writes the slabs -- byte for
 *                               byte what emat_part_upload + emat_build_coalescent_parts + the first launch would have
 *                               produced for the same parts and seeds.  The coalescent cell tables are built on the host
 *                               from topology + times.
 *   emat_tree_reassemble        run.cpp:195-256 + normalize_root: every part writes the nodes it owns back, the record
 *                               heaps are rebuilt, the changes of the root sequence are folded into the reference
 *                               sequence on the device (and reported, so that the caller's copy can follow).  It returns
 *                               when links, root and root changes are on the host (emat_tree_get_kids); the gather of the
 *                               lists may still be running, and the next emat_tree_* call that needs them waits for it
 *                               (that is also where a failure of the gather is reported)
 *   emat_tree_download          the whole tree (and its reference sequence) back as a flat tree
 *
 * Between emat_tree_repartition and emat_tree_reassemble the backend holds ordinary parts: every run / getter /
 * reduction entry point above works on them unchanged. */
emat_status emat_tree_upload(emat_backend* h, const emat_flat_tree* tree);
emat_status emat_tree_get_sizes(emat_backend* h, int32_t* num_nodes, int32_t* num_muts, int32_t* num_intervals, int32_t* num_from_states);
emat_status emat_tree_download(emat_backend* h, emat_flat_tree* out, uint8_t* ref_sequence /* [num_sites] or NULL */);
emat_status emat_tree_get_topology(emat_backend* h, int32_t* parent, int32_t* child0, int32_t* child1, double* t, int32_t* root);
/* What generate_random_partition_stencil and partition_tree (tree_partitioning.h:88-239) read of the tree and nothing more: every
 * node's two children side by side ((*kids)[2 v], (*kids)[2 v + 1]; EMAT_NO_NODE at the tips), the root and the root's time.
 * `*kids` points into the backend's own page-locked mirror, which every reassemble refreshes (1.6 MB at 200 000 nodes instead of
 * the 4 MB of emat_tree_get_topology, and no copy): valid until the next emat_tree_reassemble(_end) or emat_tree_upload. */
emat_status emat_tree_get_kids(emat_backend* h, const int32_t** kids, int32_t* num_nodes, int32_t* root, double* t_root);
/* partition_tree (tree_partitioning.h:88-135, 196-239) on the device, for callers that only have the cut nodes of a stencil:
 * one thread per part walks the part down from its cut point and numbers its nodes exactly as the reference's work list does.
 * Part i has cut node cut_nodes[i]; unless the stencil names the run's root, the root part comes last.  The arrays stay on
 * the device: emat_tree_repartition(_range) cuts THIS partition when it is given NULL for part_offset / orig / kid0 / kid1;
 * emat_tree_get_partition downloads them (any pointer may be NULL). */
emat_status emat_tree_partition(emat_backend* h, int32_t num_cuts, const int32_t* cut_nodes, int32_t* num_parts, int32_t* root_part, int32_t* part_sizes /* [num_cuts + 1] or NULL */);
emat_status emat_tree_get_partition(emat_backend* h, int32_t* part_offset, int32_t* orig, int32_t* kid0, int32_t* kid1);
emat_status emat_tree_repartition(emat_backend* h, int32_t num_parts, const int32_t* part_offset /* [num_parts + 1] */, const int32_t* orig,
                                  const int32_t* kid0, const int32_t* kid1, int32_t root_part, const uint64_t* seeds /* [num_parts] */,
                                  const emat_pop_model* pop_model, double t_step);
/* `site` / `from` / `to` [capacity] receive the changes of the reference sequence (old state, new state); any of the
 * output arguments may be NULL / 0 when the caller reads the sequence through emat_tree_download instead. */
emat_status emat_tree_reassemble(emat_backend* h, int32_t* num_root_deltas, int32_t* site, uint8_t* from, uint8_t* to, int32_t capacity);
/* ---- the tree probers on the resident tree: where, over time, a fresh sample would coalesce --------------------------------
 * They read the tree as it stands in HBM after emat_tree_upload or emat_tree_reassemble (with the run driver: between
 * emat_run_reassemble and the next emat_run_repartition) and return (members x cells) doubles; the tree itself stays where it
 * is.  While the parts are out on their slabs they fail with EMAT_ERR_STATE, as emat_tree_download does.  The time grid is the
 * reference's: num_t_cells cells of equal size over [t_start, t_end); when t_start lies after the root's time, cells of that size
 * are prepended until the root is covered (`cells_to_skip`), computed on but not returned.  Bad arguments are
 * EMAT_ERR_INVALID_ARGUMENT with the reference's complaint in emat_last_error: a site outside [0, num_sites), a marked node that
 * is neither -1 nor a node, t_end <= t_start, num_t_cells < 1, a population model its constructor refuses; a grid of more than
 * 2^22 cells or 2^26 values is EMAT_ERR_CAPACITY.  Results are bit-for-bit the same from call to call.
 *
 *   emat_tree_probe_ancestors    probe_ancestors_on_tree (core/ancestral_tree_prober.cpp:31-77): p[i][c] = probability that the
 *                                closest marked ancestor of a sample taken at the end of cell c is marked_nodes[i]; the last
 *                                member, i = num_marked, is "none of them".  -1 marks nothing (its member stays 0); of a node
 *                                given twice the first entry counts.
 *   emat_tree_probe_site_states  probe_site_states_on_tree (core/site_states_tree_prober.cpp:43-99): p[s][c] = probability that
 *                                the sample carries state s (A, C, G, T) at `site`, starting from the root's state.
 *   emat_tree_branch_counts      the Staircase_family of branch counts either prober hands to Tree_prober (core/tree_prober.h;
 *                                ancestral_tree_prober.cpp:7-29 / site_states_tree_prober.cpp:5-41 on core/staircase.cpp's
 *                                add_boxcar / add_trapezoid): counts[member][cell] over ALL *num_cells cells, the *cells_to_skip
 *                                prepended ones included, the first starting at *x_start.  With counts = NULL only the three
 *                                sizes are returned.  `kind` selects the prober; the arguments of the other one are ignored. */
typedef enum emat_probe_kind { EMAT_PROBE_ANCESTORS = 0, EMAT_PROBE_SITE_STATES = 1 } emat_probe_kind;
emat_status emat_tree_probe_ancestors(emat_backend* h, const emat_pop_model* pop_model, int32_t num_marked, const int32_t* marked_nodes /* [num_marked] */,
                                      double t_start, double t_end, int32_t num_t_cells, double* p /* [(num_marked + 1) * num_t_cells], member-major */);
emat_status emat_tree_probe_site_states(emat_backend* h, const emat_pop_model* pop_model, int32_t site, double t_start, double t_end, int32_t num_t_cells,
                                        double* p /* [4 * num_t_cells], member-major */);
emat_status emat_tree_branch_counts(emat_backend* h, int32_t kind, int32_t num_marked, const int32_t* marked_nodes, int32_t site, double t_start, double t_end, int32_t num_t_cells,
                                    int32_t* num_cells, int32_t* cells_to_skip, double* x_start, double* counts /* [members * *num_cells] or NULL */, int64_t counts_capacity);
/* ---- sampled trees kept in HBM, and the maximum-clade-credibility (MCC) tree derived from them ------------------------------
 * What a front end shows of the RUN.  The reference keeps copies of the run's tree on the host (tools/delphy_ui.cpp:770-773) and
 * derives the MCC tree from them with derive_mcc_tree (core/mcc_tree.cpp:58-156; tools/delphy_ui.cpp:784, tools/delphy_mcc.cpp).
 * All that needs of a sample is its topology and node times, 20 bytes a node, which the resident tree already has in HBM: a
 * sample is a device-to-device snapshot of those into a slot of a store, and every step of the derivation runs over
 * (samples x nodes) on the device.
 *
 * When: emat_tree_sample_push reads the resident tree as the probers do -- after emat_tree_upload or emat_tree_reassemble, with
 * the run driver between emat_run_reassemble and the next emat_run_repartition; while the parts are out on their slabs it fails
 * with EMAT_ERR_STATE.  It is queued on the engine's stream and returns at once.  Everything else here touches only the store
 * and may be called at any time, also while the parts are out (their launches queue behind the moves on the same stream).
 * The store belongs to ONE node count: after emat_tree_upload of a tree with another node count every push fails with
 * EMAT_ERR_STATE until emat_tree_samples_clear, which re-binds the store to the new count.  Samples must have the SAME nodes as
 * tips (the reference assumes tips keep their indices across base trees, mcc_tree.cpp:118-124; the engine's moves keep them).
 * With several processes every rank holds the whole tree after a reassemble; rank 0 keeps the store alone, as with the probers.
 * A handle without a device gets EMAT_ERR_NO_DEVICE: there is no CPU path.
 *
 *   emat_tree_samples_reserve   room for `capacity` samples of the resident tree's node count n: capacity x n x 20 bytes, and it
 *                               checks that the 21 bytes per sample and node a derivation over all of them works in are there
 *                               too.  More than the device has free is EMAT_ERR_CAPACITY with the sizes in emat_last_error.
 *                               A store that holds samples is not resized (EMAT_ERR_STATE): clear it first.
 *   emat_tree_sample_push       tree_snapshots.push_back(tree) (delphy_ui.cpp:770): parent, children, times and root of the
 *                               resident tree into the next slot; *index (may be NULL) receives the slot.  A full store is
 *                               EMAT_ERR_CAPACITY: nothing is evicted.
 *   emat_tree_sample_push_flat  the same from host arrays of num_nodes nodes (trees read from a file, as tools/delphy_mcc.cpp does).
 *                               EMAT_ERR_INVALID_ARGUMENT unless num_nodes is the store's, the tree is binary with one root and
 *                               consistent links, every node is below the root, and the tips are sample 0's tips.
 *   emat_tree_samples_count     slots in use, slots, nodes per sample (any may be NULL)
 *   emat_tree_samples_clear     forgets every sample (and the last derivation's correspondence table); keeps the room
 *   emat_tree_sample_get        one slot back to the host (any array may be NULL)
 *   emat_mcc_derive             derive_mcc_tree over the M = count samples first, first + stride, ... (burn-in and thinning are
 *                               the caller's: delphy_ui.cpp:770-784).  Tip fingerprints are 64 bits of a counter-based generator of
 *                               (seed, node) where the reference draws 64 bits from its bit generator (mcc_tree.cpp:70-76): two
 *                               different clades share one with probability ~ (M n)^2 / 2^65 (3e-4 at M = 1000, n = 1e5), as
 *                               there.  log_cc[k] is the sum of hist[c] (log c - log M) over c ascending, hist[c] = number of inner
 *                               nodes of sample k whose clade is in c samples (:78-103 sums the same terms in node order); the
 *                               master is the first maximum (:105-108).  support / t / t_mrca are the sums over the samples in
 *                               sample order of Mcc_tree::calculate_derived_quantities (:158-179): the same doubles.  Nothing
 *                               but the fingerprints depends on `seed`, and the same arguments give the same bits.
 *                               EMAT_ERR_INVALID_ARGUMENT: count < 1, stride < 1, a sample outside the store.
 *   emat_mcc_get_correspondence corresponding_node_to (mcc_tree.h:91-98): for the k-th chosen sample of the last derivation and
 *                               every MCC node, the MRCA in that sample of the tips below the MCC node (mcc_tree.cpp:118-147), and
 *                               whether it is exactly that clade.  The (M x n) table stays in HBM until the next derive / clear. */
typedef struct emat_mcc_result {
  int32_t master_position;   /* out: which of the `count` chosen samples is the master ... */
  int32_t master_index;      /* out: ... and its slot, first + master_position * stride */
  double* log_cc;            /* [count] log clade credibility of every chosen sample, or NULL */
  int32_t* parent;           /* [n] the MCC tree's topology = the master's; any of these may be NULL */
  int32_t* child0;           /* [n] */
  int32_t* child1;           /* [n] */
  int32_t root;              /* out */
  double* support;           /* [n] posterior_support = num_exact / count */
  double* t;                 /* [n] mean time of the corresponding nodes that match exactly */
  double* t_mrca;            /* [n] mean time of all corresponding nodes */
  int32_t* num_exact;        /* [n] in how many chosen samples the MCC node's clade occurs */
  int32_t num_distinct_clades;   /* out: keys in the table of clade counts (tips included) */
  int32_t table_regrows;     /* out: how often that table was quadrupled and refilled */
  int64_t table_slots;       /* out: its final size */
} emat_mcc_result;
emat_status emat_tree_samples_reserve(emat_backend* h, int32_t capacity);
emat_status emat_tree_sample_push(emat_backend* h, int32_t* index);
emat_status emat_tree_sample_push_flat(emat_backend* h, int32_t num_nodes, const int32_t* parent, const int32_t* child0, const int32_t* child1, const double* t, int32_t root, int32_t* index);
emat_status emat_tree_samples_count(emat_backend* h, int32_t* count, int32_t* capacity, int32_t* num_nodes);
emat_status emat_tree_samples_clear(emat_backend* h);
emat_status emat_tree_sample_get(emat_backend* h, int32_t index, int32_t* parent, int32_t* child0, int32_t* child1, double* t, int32_t* root);
emat_status emat_mcc_derive(emat_backend* h, int32_t first, int32_t count, int32_t stride, uint64_t seed, emat_mcc_result* out);
emat_status emat_mcc_get_correspondence(emat_backend* h, int32_t k, int32_t* node_in_sample /* [n] */, uint8_t* is_exact /* [n] */);
/* ---- the ancestral prober over all kept samples in one call, with the spread of its answers --------------------------------
 * A front end draws a lineage-prevalence curve with its uncertainty band by running probe_ancestors_on_tree on EVERY base tree of
 * the MCC tree, the marked nodes of a base tree being the nodes that correspond to the MCC nodes picked
 * (tools/delphy_wasm.cpp:1828-1849: "iterating over all base trees in an MCC, and some node in the MCC isn't linked to any node in
 * some base tree -> -1").  A sample of the store holds what that prober reads, so the two calls below run it over the chosen
 * samples on the device -- every step over (samples x nodes) or (samples x members x cells), the number of launches independent
 * of the number of samples -- and return the per-sample probabilities, or only their mean and order statistics over the samples.
 * Sample k of a call is slot first + k * stride, as in emat_mcc_derive.  For it:
 *   p[k]            is what emat_tree_probe_ancestors returns for that sample's tree, its marks and its population model, BIT FOR
 *                   BIT: member num_marked is "none of them", a mark of -1 marks nothing, of a node marked twice the first entry
 *                   wins; the grid extension of ancestral_tree_prober.cpp:52-61 is made per sample against that sample's own root
 *                   time (cells_to_skip[k]) with the same subtractions on the host, and the fixed-point quantum is the one of the
 *                   store's node count.
 *   mean            ((p_0 + p_1) + ... + p_{count-1}) / count, added in sample order and divided once
 *   order_stats[j]  for every (member, cell) the ranks[j]-th smallest of the count values (an exact sort on the device).  At most
 *                   4 096 samples when order statistics are asked for (the sort's workgroup holds them in LDS): more is
 *                   EMAT_ERR_CAPACITY.
 * Only what is asked for crosses to the host.  Both calls touch only the store: like emat_mcc_derive they may be called while the
 * parts are out, and their launches queue on the engine's stream; with several processes rank 0 answers alone.  The site-state
 * form is the next section: it needs samples that kept their mutations.  The samples are worked on in chunks sized from the free device memory (per
 * sample about 12 bytes a node and 28 bytes per member and cell); the results are the same bits for every chunk size, and option
 * "samples_probe_chunk" (0 = automatic; may be set at any time) forces one for tests.
 *
 *   emat_tree_samples_probe_ancestors  pop_models: one for all (num_pop_models = 1) or one per chosen sample (= count);
 *                                      marked_nodes: [num_marked] for all (marks_per_sample = 0) or [count][num_marked] (= 1).
 *   emat_mcc_probe_ancestors           probes the samples of the LAST emat_mcc_derive (its first / count / stride); the mark of
 *                                      sample k for entry i is the node corresponding to mcc_nodes[i] in that sample, read on the
 *                                      device from the table emat_mcc_get_correspondence serves, exact match or not.
 *   emat_mcc_get_derivation            first / count / stride of the last derivation, which size emat_mcc_probe_ancestors' outputs
 *                                      (any may be NULL); count = 0 when there is no valid one.  An emat_mcc_derive refused for its
 *                                      arguments leaves the derivation before it in place, as it does for emat_mcc_get_correspondence.
 * EMAT_ERR_INVALID_ARGUMENT (text in emat_last_error): what emat_tree_probe_ancestors refuses, with its messages; count < 1,
 * stride < 1, a sample outside the store; num_pop_models neither 1 nor count; a population model its constructor refuses (the
 * text says which); a per-sample mark outside [-1, n) (the text names sample and entry); a rank outside [0, count); num_ranks > 0
 * without ranks or order_stats; p, mean and order_stats all NULL.  EMAT_ERR_STATE: emat_mcc_probe_ancestors without a valid
 * derivation (none yet, emat_tree_samples_clear since, or the last one failed).  EMAT_ERR_CAPACITY: a sample's grid beyond
 * emat_tree_probe_ancestors' limits; results or working room beyond the free device memory (the text gives the sizes); order
 * statistics over more than 4 096 samples.  EMAT_ERR_INTERNAL: a sample in which a node is earlier than its parent
 * (emat_tree_sample_push_flat does not check times); the text names the sample's position.  EMAT_ERR_NO_DEVICE: a handle without a
 * device.  After any refusal the next call works. */
typedef struct emat_samples_probe_result {
  double*  p;             /* [count][num_marked + 1][num_t_cells], or NULL: every chosen sample's probabilities (site-state form: [count][num_sites][4][num_t_cells], and so on below) */
  double*  mean;          /* [num_marked + 1][num_t_cells], or NULL: ((p_0 + p_1) + ... + p_{count-1}) / count, summed in sample order */
  int32_t  num_ranks;     /* 0, or how many order statistics */
  const int32_t* ranks;   /* [num_ranks], each in [0, count) */
  double*  order_stats;   /* [num_ranks][num_marked + 1][num_t_cells], or NULL: for every (member, cell) the ranks[j]-th smallest of the count values */
  int32_t* cells_to_skip; /* [count], or NULL: how many cells each sample's grid was extended by to reach its root */
} emat_samples_probe_result;
emat_status emat_tree_samples_probe_ancestors(emat_backend* h,
    const emat_pop_model* pop_models, int32_t num_pop_models /* 1: one for all; count: one per chosen sample */,
    int32_t first, int32_t count, int32_t stride,
    int32_t num_marked, const int32_t* marked_nodes, int32_t marks_per_sample /* 0: [num_marked] for all; 1: [count][num_marked] */,
    double t_start, double t_end, int32_t num_t_cells, emat_samples_probe_result* out);
emat_status emat_mcc_probe_ancestors(emat_backend* h, const emat_pop_model* pop_models, int32_t num_pop_models,
    int32_t num_marked, const int32_t* mcc_nodes,
    double t_start, double t_end, int32_t num_t_cells, emat_samples_probe_result* out);
emat_status emat_mcc_get_derivation(emat_backend* h, int32_t* first, int32_t* count, int32_t* stride);
/* ---- samples that keep their mutations, and the site-state prober over all kept samples in one call --------------------------
 * The second curve a front end draws over every base tree of an MCC tree: probe_site_states_on_tree
 * (core/site_states_tree_prober.cpp:40-92, exported at tools/delphy_wasm.cpp:1809), the prevalence of a site's four states over time,
 * with the same band over the samples.  That prober reads a tree's mutations and the sequence its root starts from, which a sample of
 * the store does not have unless the store is told to keep them.  Opt-in: a store without this room behaves exactly as before.
 *
 *   emat_tree_samples_reserve_mutations  after emat_tree_samples_reserve, on an empty store (one that holds samples is
 *                               EMAT_ERR_STATE: clear it first): room for the per-node list headers of `capacity` samples
 *                               (capacity x n x 8 bytes), the reference sequence of every slot (capacity x L bytes, L = the handle's
 *                               num_sites) and an arena of `mutation_records` records of 16 bytes shared by all slots (a Mutation,
 *                               core/mutations.h:21-29).  hipMemGetInfo is asked first: more than is free is EMAT_ERR_CAPACITY with the
 *                               three sizes in emat_last_error.  0 releases the room.  A later emat_tree_samples_reserve (or the
 *                               re-binding emat_tree_samples_clear does after the node count changed) that re-allocates the store, or
 *                               changes its slots or node count, DROPS this room: reserve it again.
 *   emat_tree_sample_push       on a store with that room also keeps the resident tree's list headers, the used part of its mutation
 *                               heap (as one segment of the arena; the headers' offsets stay as they are, relative to the segment)
 *                               and the reference sequence as it stands on the device (Base_tree_vector::push_back copies the whole
 *                               Phylo_tree, delphy_ui.cpp:770-773): device to device on the engine's stream.  An arena without room
 *                               for this tree's records is EMAT_ERR_CAPACITY (records needed and free in the text): nothing is
 *                               pushed and the count is unchanged.
 *   emat_tree_sample_push_flat_mutations  emat_tree_sample_push_flat for a tree that comes with its mutations as CSR lists
 *                               (mut_offset [n + 1]; a file's trees, tools/delphy_mcc.cpp) and its reference sequence [L].  On top of
 *                               emat_tree_sample_push_flat's checks: offsets start at 0 and never decrease, sites are in [0, L), states
 *                               in [0, 4) here and in ref_sequence.  That the states chain along the tree is NOT checked.  The root may
 *                               carry mutations.  emat_tree_sample_push_flat itself still works on such a store: its sample is marked
 *                               as having no mutations, and the site-state calls refuse a range that includes it.
 *   emat_tree_sample_get_mutations  one slot's mutations back as CSR in node order, each list in its stored order, and its reference
 *                               sequence (Phylo_tree::ref_sequence); any array may be NULL.  `capacity` (records) too small is
 *                               EMAT_ERR_CAPACITY with *num_mutations set.
 *   emat_tree_samples_mutation_info  records handed out, records of the arena (0: no room), and the L the room is bound to.
 *   emat_tree_samples_clear     hands the arena out afresh and keeps the room.
 * The store binds to ONE number of sites, as to one node count.
 *
 *   emat_tree_samples_probe_site_states  for sample k (slot first + k * stride) and entry i of `sites`:
 *     p[k][i]       [4][num_t_cells], BIT FOR BIT what emat_tree_probe_site_states returns for that sample's tree, reference sequence,
 *                   population model and sites[i]: a branch takes the first mutation of the site on its list; the root starts from the
 *                   slot's reference state with every mutation of the site on its own list applied, and that state is the chain's
 *                   initial member; grid extension per sample against its own root (site_states_tree_prober.cpp:60-69), the
 *                   fixed-point quantum of the store's node count, the same add_boxcar / add_trapezoid, intensity and exp.
 *     mean, order_stats   as for the ancestral form, over the samples, for every (site entry, state, cell)
 *     Dimensions of emat_samples_probe_result here, "members" being 4 x num_sites:  p [count][num_sites][4][num_t_cells];
 *     mean [num_sites][4][num_t_cells];  order_stats [num_ranks][num_sites][4][num_t_cells];  cells_to_skip [count].
 *     A site may be given twice.  The number of launches grows neither with count nor with num_sites: the chunks iterate over
 *     (sample, site) pairs, "samples_probe_chunk" counting samples, each with all its sites; results are the same bits for every
 *     chunk size.  Touches only the store: may be called while the parts are out; rank 0 answers alone.
 *   emat_mcc_probe_site_states           the same with the first / count / stride of the last emat_mcc_derive
 *     (emat_mcc_get_derivation sizes the outputs).  Sites are the same in every base tree: the correspondence table plays no part.
 * EMAT_ERR_INVALID_ARGUMENT: what the ancestral batched call refuses of samples, models, window, ranks and outputs, with its texts;
 * num_sites < 1 or sites NULL; a site outside [0, L) (the text names the entry).  EMAT_ERR_STATE: a store without mutation room; a
 * chosen sample pushed without mutations (the text names its position and slot); emat_mcc_probe_site_states without a valid
 * derivation.  EMAT_ERR_CAPACITY: the grid of a (sample, site) beyond emat_tree_probe_site_states' limits; results, or the working room
 * of one sample with all its sites, beyond the free device memory (sizes in the text); order statistics over more than 4 096 samples.
 * EMAT_ERR_INTERNAL: a bad link, a node earlier than its parent, or a list outside its segment in a sample (position in the text).
 * EMAT_ERR_NO_DEVICE: a handle without a device.  After any refusal the next call works. */
emat_status emat_tree_samples_reserve_mutations(emat_backend* h, int64_t mutation_records);
emat_status emat_tree_sample_push_flat_mutations(emat_backend* h, int32_t num_nodes, const int32_t* parent, const int32_t* child0, const int32_t* child1, const double* t, int32_t root,
    const int32_t* mut_offset /* [num_nodes + 1] */, const int32_t* mut_site, const uint8_t* mut_from, const uint8_t* mut_to, const double* mut_t,
    const uint8_t* ref_sequence /* [num_sites] */, int32_t* index);
emat_status emat_tree_sample_get_mutations(emat_backend* h, int32_t index, int32_t* mut_offset /* [n + 1] */, int32_t* site, uint8_t* from, uint8_t* to, double* t,
    int64_t capacity, uint8_t* ref_sequence /* [num_sites] */, int64_t* num_mutations);
emat_status emat_tree_samples_mutation_info(emat_backend* h, int64_t* records_used, int64_t* records_capacity, int32_t* num_sites);
emat_status emat_tree_samples_probe_site_states(emat_backend* h,
    const emat_pop_model* pop_models, int32_t num_pop_models /* 1: one for all; count: one per chosen sample */,
    int32_t first, int32_t count, int32_t stride, int32_t num_sites, const int32_t* sites /* [num_sites] */,
    double t_start, double t_end, int32_t num_t_cells, emat_samples_probe_result* out);
emat_status emat_mcc_probe_site_states(emat_backend* h, const emat_pop_model* pop_models, int32_t num_pop_models,
    int32_t num_sites, const int32_t* sites /* [num_sites] */,
    double t_start, double t_end, int32_t num_t_cells, emat_samples_probe_result* out);
/* ---- on the MCC tree: the spread of every node's date over the samples, and the support of the master's mutations -------------
 * A time tree is drawn with a bar on every node (the spread of that node's date over the samples) and with its mutations marked by
 * how many samples agree with them.  The reference exposes the MCC tree's base trees and, per base tree, the corresponding node
 * and whether it matches exactly (core/mcc_tree.h:91-98), and exports both (tools/delphy_wasm.cpp:1503-1523) so that a front end
 * loops over every base tree.  Here that loop would pull the (M x n) correspondence table and every sample to the host; the two
 * calls below make those numbers where the table, the samples' times and their mutation lists already lie.
 *
 * Both work on the LAST VALID DERIVATION: its first / count / stride, its master and its correspondence table, as
 * emat_mcc_probe_ancestors uses them.  M = its sample count, sample k = slot first + k * stride, n = nodes per sample; for MCC node
 * v, c(k, v) = corr[k][v] and x(k, v) = the double t[c(k, v)] of sample k as the store holds it.  Both touch only the store, may be
 * called while the parts are out, and queue on the engine's stream; with several processes rank 0 answers alone; a handle without
 * a device gets EMAT_ERR_NO_DEVICE.  No other call's behaviour or bits change.
 *
 *   emat_mcc_node_times   for each node asked for (mcc_nodes NULL: all n in node order, num_nodes is ignored; a node may be given
 *     twice, every entry is answered; tips are nodes like any other) and each of two sets of samples --
 *       mrca:   all k, m = M (the spread behind emat_mcc_derive's t_mrca);
 *       exact:  {k : exact[k][v]}, m = num_exact[v] >= 1 (the master matches itself; the spread behind t) --
 *     with s = the set's m values x(k, v) sorted ascending:
 *       quantile j   s[floor(quantiles[j] * (double)(m - 1))]: one double multiplication and one floor
 *       hpd          w = min(m, max(1, ceil(hpd_mass * (double)m))); i* = the SMALLEST i in [0, m - w] that minimises the double
 *                    s[i + w - 1] - s[i]; lo = s[i*], hi = s[i* + w - 1]: the shortest interval holding that share of the values,
 *                    the first one on ties
 *       times / is_exact   x(k, v) and exact[k][v] themselves, [num_nodes][M] in sample order: for the handful of nodes whose
 *                    histogram is drawn; num_nodes x M above 2^26 values is EMAT_ERR_CAPACITY.
 *     Every output is one of the doubles in the store: nothing is averaged or interpolated, and the results are the same for
 *     every chunk size and from call to call.  The sort is the probers' (an exact sort in LDS): a derivation over more than
 *     4 096 samples is EMAT_ERR_CAPACITY.  The nodes are worked on in chunks sized from half the free device memory (9 bytes per
 *     node and sample); option "mcc_summary_chunk" (0 = automatic; may be set at any time) forces a chunk of that many nodes for
 *     tests.  Only what is asked for crosses to the host.
 *     EMAT_ERR_STATE: no valid derivation (none yet, emat_tree_samples_clear since, or the last one failed).
 *     EMAT_ERR_INVALID_ARGUMENT: num_nodes < 1 with a list; a node outside [0, n) (the text names the entry); a quantile outside
 *     [0, 1] or NaN; hpd_mass outside [0, 1] or NaN; num_quantiles > 0 without quantiles; every output NULL; q_exact / q_mrca
 *     without quantiles, hpd_exact / hpd_mrca with hpd_mass = 0.  EMAT_ERR_INTERNAL: a node time of a chosen sample that is not
 *     finite (+inf pads the sort; the text names the sample's position), or a table entry outside the tree.
 *
 *   emat_mcc_mutation_support   records are the MASTER sample's mutations in the CSR order emat_tree_sample_get_mutations(master
 *     slot) returns them: node order, each list in stored order, the root's own list included.  For record j on node v with
 *     (site, from, to), sample k HAS it when exact[k][v] and the stored list of node c(k, v) in sample k holds a record with the
 *     same site, from and to; its time in that sample is the t of the FIRST such record in stored order.
 *       num_with[j]   how many chosen samples have it (>= 1: the master has it)
 *       mean_t[j]     the sum of those times IN SAMPLE ORDER, divided once by num_with[j]
 *       t_min / t_max the smallest and largest of those times
 *     *num_mutations (may be NULL) receives the number of records; with every array NULL that is all the call does.
 *     EMAT_ERR_STATE: no valid derivation; a store without mutation room; a chosen sample pushed without mutations (the text names
 *     its position and slot).  EMAT_ERR_CAPACITY, with *num_mutations set: `capacity` (records) too small.  EMAT_ERR_INTERNAL: a list
 *     outside its segment.
 * After any refusal the next call works. */
typedef struct emat_mcc_node_times_result {
  int32_t num_quantiles;     /* in: 0, or how many quantiles */
  const double* quantiles;   /* in: [num_quantiles], each in [0, 1] */
  double  hpd_mass;          /* in: in (0, 1]; 0: no HPD asked for */
  double* q_exact;           /* [num_quantiles][num_nodes], or NULL */
  double* q_mrca;            /* [num_quantiles][num_nodes], or NULL */
  double* hpd_exact;         /* [2][num_nodes]: lo, hi; or NULL */
  double* hpd_mrca;          /* [2][num_nodes]: lo, hi; or NULL */
  int32_t* num_exact;        /* [num_nodes], or NULL */
  double* times;             /* [num_nodes][M] in sample order, or NULL: x(k, v) itself */
  uint8_t* is_exact;         /* [num_nodes][M] in sample order, or NULL: exact[k][v] itself */
} emat_mcc_node_times_result;
emat_status emat_mcc_node_times(emat_backend* h, int32_t num_nodes, const int32_t* mcc_nodes /* NULL: all n, in node order */,
    emat_mcc_node_times_result* out);
emat_status emat_mcc_mutation_support(emat_backend* h, int64_t capacity /* records */, int64_t* num_mutations,
    int32_t* num_with /* [records] */, double* mean_t, double* t_min, double* t_max /* any may be NULL */);
/* One run over several processes, one GPU each, EVERY one with the whole tree in its HBM (the tree is a few tens of MB; what
 * is worth sharding is the moves).  Every process cuts the same partition and calls emat_tree_repartition_range with its own
 * block [part_lo, part_hi) of the parts (backend part id = part - part_lo): the sequence states at the cut points and the
 * coalescent grid are computed for the whole run by every process -- identically, no exchange -- and only the slabs of the
 * block are built.  After the moves:
 *   emat_tree_get_root_deltas     on the process that holds the root part (*num_root_deltas = -1 elsewhere); the caller
 *                                 hands the result to every process
 *   emat_tree_gather_local        every process: its own parts back into its copy of the tree (heaps rebuilt from zero)
 *   emat_tree_export_nodes        every process: what its parts own and link, as one buffer (buf = NULL: size only)
 *   emat_tree_apply_nodes         every process, once per OTHER process's buffer (an all-gather, the caller's)
 *   emat_tree_reassemble_end      every process: mirrors refreshed; every copy of the tree holds the same nodes again
 * (lists sit at different heap offsets in different processes, which nothing depends on).  `buf` of emat_tree_export_nodes /
 * emat_tree_apply_nodes may be host memory or device memory: with device buffers the exchange is one RCCL all-gather on
 * what the kernels wrote, and nothing but a 32-byte header and the per-node records (for validation) crosses PCIe.
 * Streams: the engine launches on a stream of its own.  emat_tree_export_nodes returns with its kernels finished (the buffer
 * may be handed to a collective on any stream); emat_tree_apply_nodes reads `buf` from the engine's stream as soon as it is
 * called, so the caller must have waited for whatever produced a DEVICE buffer (e.g. the all-gather on its own stream). */
emat_status emat_tree_repartition_range(emat_backend* h, int32_t num_parts, const int32_t* part_offset, const int32_t* orig, const int32_t* kid0, const int32_t* kid1,
                                        int32_t root_part, const uint64_t* seeds, const emat_pop_model* pop_model, double t_step, int32_t part_lo, int32_t part_hi);
emat_status emat_tree_get_root_deltas(emat_backend* h, int32_t* num_root_deltas, int32_t* site, uint8_t* from, uint8_t* to, int32_t capacity);
emat_status emat_tree_gather_local(emat_backend* h, int32_t num_root_deltas, const int32_t* site, const uint8_t* from, const uint8_t* to);
emat_status emat_tree_export_nodes(emat_backend* h, uint8_t* buf, uint64_t capacity, uint64_t* bytes_needed);
emat_status emat_tree_apply_nodes(emat_backend* h, const uint8_t* buf, uint64_t bytes);
emat_status emat_tree_reassemble_end(emat_backend* h);

/* Forces the from-scratch recomputation that Subrun::validate_derived_quantities() performs
 * after set_evo / set_coalescent_prior_part (reference subrun.cpp:17-26).  Called implicitly
 * by the run functions when the derived quantities are stale. */
emat_status emat_recalc_derived(emat_backend* h);

/* replaces: Subrun::check_derived_quantities (reference subrun.cpp:28-56), which debug builds run after every move and
 * --v0-paranoid forces in release builds (run.h:220-224, cmdline.cpp:177).  Every part's lambda_i, num_sites_missing, log_G
 * and augmented coalescent prior are recomputed from scratch ON THE DEVICE into scratch memory and compared with what the
 * moves maintained incrementally; the state is not touched, nothing but this library is involved.  `tol_scale` multiplies
 * the reference's own tolerances (|d lambda_i| / L < 1e-8, |d log_G| < 1e-6, |d prior| < 1e-5; missing-site counts exact).
 * Returns EMAT_OK, or EMAT_ERR_INTERNAL with emat_last_error naming the first offending part and quantity.
 * `*worst_part` / `worst4` (either may be NULL): that part -- or, when all is well, the part closest to a tolerance -- and
 * its four deviations {lambda per site, log_G, prior, nodes with a wrong missing-site count}. */
emat_status emat_check_derived(emat_backend* h, double tol_scale, int32_t* worst_part, double* worst4);

/* ---- results ---------------------------------------------------------------------------- */
/* replaces: sum of subrun.log_G() / subrun.log_augmented_coalescent_prior()
 * (reference run.cpp:340-348) */
emat_status emat_get_totals(emat_backend* h, double* log_G, double* log_augmented_coalescent_prior);

/* ---- sufficient statistics of the global moves ---------------------------- */
/* replaces: Run::calc_cur_Ttwiddle_beta_a / calc_cur_num_muts / calc_cur_num_muts_ab (reference run.cpp:445-453), i.e.
 * calc_Ttwiddle_beta_a (phylo_tree_calc.cpp:288-369), calc_num_muts_beta_ab (:599-610), calc_num_muts (:577-585), which
 * the host-side global moves (mu, HKY kappa / pi; run.cpp:781-1010) consume.  Computed on the device over the parts of
 * this handle and summed in part order, so that the trees need not be downloaded for them: every branch of the whole
 * tree is a non-root branch of exactly one part.  With parts spread over several handles (GPUs) the caller adds the
 * per-handle results.  Ttwiddle_beta_a[beta][a] = sum over sites l of partition beta of nu_l x (time site l spends in
 * state a over all branches, missing stretches excluded); num_muts_beta_ab[beta][a][b] counts mutations a -> b.
 * num_partitions must equal the value given to emat_set_evo and be <= 4 (EMAT_ERR_CAPACITY otherwise). */
emat_status emat_get_global_stats(emat_backend* h, int32_t num_partitions, double* Ttwiddle_beta_a /*[P][4]*/,
                                  int64_t* num_muts_beta_ab /*[P][4][4]*/, int64_t* num_muts /* may be NULL */);

/* replaces: calc_num_muts_l (reference phylo_tree_calc.cpp:612-622), consumed with calc_Ttwiddle_l by the site-rate
 * (alpha / nu_l) moves (run.cpp:1109-1110, 1184-1185): mutations per site over all branches of all parts of this handle
 * (the deltas above a part's root are not mutations).  With parts on several handles the caller adds the vectors. */
emat_status emat_get_num_muts_l(emat_backend* h, int32_t* num_muts_l /*[num_sites]*/);

/* replaces: calc_Ttwiddle_l (reference phylo_tree_calc.cpp:176-222; with calc_num_muts_l the input of the site-rate moves,
 * run.cpp:1109, 1184): Ttwiddle^(l) = sum_a q^(l)_a T^(l)_a, the escape-rate-weighted time site l spends in each state.
 * The reference corrects q_ref T_total per mutation / missation by the branch length BELOW that point, which crosses
 * part boundaries, so the computation is staged (the run driver, who knows the tree of parts, wraps it:
 * emat_run_get_Ttwiddle_l):
 *   emat_get_part_tree_lengths   sum of the branch lengths inside each part;
 *   emat_Ttwiddle_l_partial      given, for every part, the tips that are cut nodes of parts below and the whole-tree
 *                                branch length hanging at each (CSR: ext_offset[num_parts + 1], ext_node, ext_length), the
 *                                per-site sums S and R over this handle's parts and, on the handle holding the run's root,
 *                                the total tree length;
 *   emat_Ttwiddle_l_finish       Ttwiddle_l = q_ref (T_total - R) + S from the sums over ALL handles (all-reduce SUM). */
emat_status emat_get_part_tree_lengths(emat_backend* h, double* tree_length_of_part /*[num_parts]*/);
emat_status emat_Ttwiddle_l_partial(emat_backend* h, const int32_t* ext_offset, const int32_t* ext_node, const double* ext_length,
                                    double* S /*[num_sites]*/, double* R /*[num_sites]*/, double* tree_length_below_root /* may be NULL */);
emat_status emat_Ttwiddle_l_finish(emat_backend* h, const double* S_sum, const double* R_sum, double tree_length, double* Ttwiddle_l /*[num_sites]*/);

/* ---- the site-rate moves: steps on alpha, then a Gibbs draw of every nu_l --------------------------------------------------
 * replaces: Run::alpha_moves and Run::gibbs_sample_all_nus (reference run.cpp:1105-1235), the one group of global moves whose work
 * grows with the number of sites: `num_alpha_steps` scaling Metropolis steps on the shape alpha of the site-rate prior (scale
 * uniform in [0.9, 1/0.9), exponential prior of mean 1, target calc_log_p_alpha, :1157-1215), the increment of the alpha prior
 * from the rates as they were (:1218-1231), and nu_l ~ Gamma(M_l + alpha, rate mu_l Ttwiddle_l + alpha) for every site, floored
 * at 1e-50 (:1114-1151), with the increments of log G and of the nu prior.  All on the device, in three launches.
 *
 * Inputs are the statistics of the WHOLE run, as SUMS over all handles: Ttwiddle_l from emat_Ttwiddle_l_finish and the summed
 * vectors of emat_get_num_muts_l (a sharded caller all-reduces both as it already does for Ttwiddle_l).  Random numbers come from
 * streams named by (key, site) -- block j of site l is Philox4x32-10 of counter (l << 32) | j under `key`; the alpha steps use the
 * pseudo-site 0xFFFFFFFF, step s taking block s: word 0 the scale, word 1 the acceptance uniform, drawn whether needed or not --
 * and every sum is added in a fixed order: with the same evolution model, the same arguments give the same nu_l and the same
 * result BIT FOR BIT on every handle and in every call.
 *
 * The call first finishes a pending pass (which reads the rates).  Afterwards the handle's nu_l are the new ones, as if given to
 * emat_set_evo: the parts' derived quantities are stale and are recomputed by the next run or by emat_recalc_derived.
 * `out->trace` (may be NULL) receives one record per step; `trace_capacity` is its room.
 * EMAT_ERR_INVALID_ARGUMENT (text in emat_last_error, naming the first offending site where there is one): a null pointer, alpha
 * not finite or <= 0, num_alpha_steps < 0, trace_capacity < num_alpha_steps with a trace, a Ttwiddle_l that is negative or not
 * finite, a negative count -- all answered before the device is asked for.  EMAT_ERR_NO_DEVICE: a handle without a device (there
 * is no CPU path).  EMAT_ERR_STATE: before emat_set_evo.  After any refusal nu_l is untouched and the next call works.
 *
 *   emat_get_nu_l             the handle's relative site rates: what emat_set_evo was given, or the last move's draws
 *   emat_debug_sample_gamma   test hook: n draws of the moves' sampler (Marsaglia-Tsang; a shape below 1 drawn at shape + 1 and
 *                             multiplied by u^(1 / shape); no floor), draw i from the stream (key, i) */
typedef struct emat_site_rate_step { double proposed_alpha, log_p_proposed, log_metropolis, u; int32_t accepted, pad_; } emat_site_rate_step;
typedef struct emat_site_rate_result {
  double alpha;                    /* out: alpha after the steps */
  double log_p_alpha_start;        /* out: log p(alpha) at the alpha passed in */
  int32_t num_accepted, num_floored;
  double delta_log_G;              /* run.cpp:1144 summed over the sites */
  double delta_log_prior_alpha;    /* run.cpp:1226-1231 */
  double delta_log_prior_nu;       /* run.cpp:1148 + 1151 */
  double sum_nu_old, sum_nu_new;
  emat_site_rate_step* trace; int32_t trace_capacity;   /* may be NULL / 0 */
} emat_site_rate_result;
emat_status emat_site_rate_moves(emat_backend* h, const double* Ttwiddle_l /*[L]*/, const int32_t* num_muts_l /*[L]*/,
                                 double alpha, int32_t num_alpha_steps /* 10 in the reference; 0 = gibbs_sample_all_nus alone */,
                                 uint64_t key, emat_site_rate_result* out);
emat_status emat_get_nu_l(emat_backend* h, double* nu_l /*[L]*/);
emat_status emat_debug_sample_gamma(emat_backend* h, uint64_t key, int32_t n, double shape, double rate, double* out /*[n]*/);  /* draw i uses stream (key, i) */

/* ---- the Skygrid population moves: tau, the zero mode and the HMC on the gammas ----------------------------------------------
 * replaces: the Skygrid branch of Run::run_global_moves (reference run.cpp:766-778): skygrid_tau_move (:1321-1358),
 * skygrid_gammas_zero_mode_gibbs_move (:2016-2189) and skygrid_gammas_hmc_move (:1360-2014), in that order, on the device in two
 * launches (csrc/emat_skygrid_kernels.hpp): the inner nodes' statistics per knot, then ONE workgroup for the three moves and every
 * leapfrog step.
 *
 * Inputs are the statistics of the WHOLE run as host arrays: the lineage grid of Scalable_coalescent_prior
 * (scalable_coalescent.cpp:88-138), k_bar[c] for the cells j = first_cell .. first_cell + num_cells - 1, cell j = [t_ref + j t_step,
 * t_ref + (j + 1) t_step) as emat_scalable_coalescent_partial numbers them (1 lineage before the root inside the root's cell), and
 * the times of the inner nodes (any order; the sums over them are added in the order given).  A sharded caller adds the grids
 * and concatenates the times.  `pop_model` is the Skygrid curve the moves start from.
 *
 * Random numbers: the (key, id) streams of the site-rate moves.  Knot k's initial momentum is sqrt(m_k) x one Box-Muller normal,
 * the first two words of stream (key, k).  Five pseudo-ids at the top of the range, each drawn from its stream's start and drawn
 * whether needed or not:
 *   0xFFFFFFFE  the tau draw (Marsaglia-Tsang, as emat_debug_sample_gamma)    0xFFFFFFFD  the zero mode's I_bar draw (same sampler)
 *   0xFFFFFFFC  the zero mode's acceptance uniform, [0, 1)                     0xFFFFFFFB  dt = -hmc_mean_dt log(u), u in (0, 1]
 *   0xFFFFFFFA  the HMC's acceptance uniform, [0, 1)
 * Every sum is added in a fixed order and there are no atomics: the same arguments give the same result BIT FOR BIT on every handle and
 * in every call.  The sum over inner nodes of log N(t_i) is formed as sum_k W_k gamma_k, W_k = sum_i d log N(t_i) / d gamma_k (log N is
 * linear in the gammas for both Skygrid types), so the nodes are read once per call.
 *
 * The call first finishes a pending pass.  It changes nothing in the handle: the caller hands the new curve to the next
 * emat_tree_repartition / emat_build_coalescent_parts.
 * EMAT_ERR_INVALID_ARGUMENT (text in emat_last_error naming the first offender), all answered before the device is asked for: a null
 * pointer; a model that is not a Skygrid or that the model check refuses; t_ref not finite or t_step not finite and positive; tau not
 * finite or <= 0; a barrier scale <= 0 (or not finite) with the barrier on; hmc_steps < 0; hmc_mean_dt not finite or <= 0; num_cells < 1;
 * num_inner < 1; a k_bar that is negative or not finite; an inner_t that is not finite or lies outside the grid's cells; a trace
 * with trace_capacity < hmc_steps.  EMAT_ERR_CAPACITY: more than 1 024 knots or 2^22 cells, or cell numbers outside [-2^30, 2^30).  EMAT_ERR_NO_DEVICE: a handle without
 * a device, after the argument checks (there is no CPU path).
 *
 *   emat_debug_pop_gradient   test hook: the device's gradient of the Skygrid curve, point by point (reference pop_model.cpp:206-225,
 *                             333-523).  op 3: out[i] = d log(integral of N over [a[i], b[i]]) / d gamma_k; op 4: out[i] =
 *                             d log N(a[i]) / d gamma_k.  (emat_debug_pop's ops 0-2 and signature are as they were.) */
typedef struct emat_skygrid_spec {          /* Run's setters, reference run.h:85-91 and neighbours */
  double tau;                                /* in: skygrid_tau_ */
  int32_t tau_move_enabled, low_gamma_barrier_enabled;
  double tau_prior_alpha, tau_prior_beta;
  double low_gamma_barrier_loc, low_gamma_barrier_scale;
  double inv_nbar_prior_alpha, inv_nbar_prior_beta;
  int32_t do_tau, do_zero_mode, do_hmc;      /* which of the three to run, in the reference's order (tau also needs tau_move_enabled) */
  int32_t hmc_steps;                         /* 25 in the reference */
  double hmc_mean_dt;                        /* 2 pi / 100 in the reference */
} emat_skygrid_spec;
typedef struct emat_skygrid_result {
  double* gamma;                             /* out [num_knots], the caller's array: the curve after the three moves */
  double tau;                                /* after the tau move (the tau passed in when it did not run) */
  double log_coalescent_prior_start;         /* calc_log_prior, scalable_coalescent.cpp:163-187, under the model passed in */
  double log_coalescent_prior_end;           /* ... under the model returned (run.cpp:2170, :2004) */
  double delta_log_other_priors;             /* run.cpp:1355-1357 + :2186-2187 + :2005, of the moves that ran and were accepted */
  /* skygrid_tau_move */
  double tau_post_alpha, tau_post_beta;      /* run.cpp:1343-1344 */
  double tau_draw;                           /* :1352; drawn also when the move does not run */
  double tau_delta_log_prior;                /* :1355-1357; 0 when it did not run */
  /* skygrid_gammas_zero_mode_gibbs_move */
  double zero_B;                             /* run.cpp:2108-2112 */
  double zero_shape, zero_rate;              /* :2115-2117 */
  double zero_I_bar;                         /* :2120, the draw */
  double zero_delta_gamma_bar;               /* :2121 */
  double zero_log_metropolis, zero_u;        /* :2164-2165; u in [0, 1) */
  int32_t zero_accepted;
  /* skygrid_gammas_hmc_move */
  int32_t hmc_accepted;                      /* run.cpp:1994 */
  double hmc_dt;                             /* :1885 */
  double hmc_K_old, hmc_K_new;               /* :1855, :1973 (new = old when the move ended early or did not run) */
  double hmc_U_prior_old, hmc_U_prior_new;   /* :1856, :1974 */
  double hmc_U_coal_old, hmc_U_coal_new;     /* :1857, :1975 */
  double hmc_log_metropolis, hmc_u;          /* :1978, :1994; u in [0, 1) */
  int32_t hmc_K_exit_step;                   /* the K > 100 (M + 1) rule: -1 = it never ended the move, 0 = the initial momenta (:1868), s >= 1 = after
                                                the momentum update of leapfrog step s, counted from 1 (:1940) */
  int32_t hmc_nan;                           /* :1981-1989 ended it */
  int32_t hmc_steps_done;                    /* force evaluations made */
  int32_t trace_capacity;                    /* in: leapfrog steps `trace` has room for (>= hmc_steps) */
  /* may be NULL: [5 + 4 * trace_capacity][num_knots] doubles.  Rows 0-4: c_k (run.cpp:1695-1702), W_k, m_k (:1708), gamma at the start of
   * the HMC, the initial p_k (:1852).  Then four rows per leapfrog step made: gamma after the first half step (:1893-1895), f_k (:1900),
   * p_k after the momentum step (:1931-1933), gamma after the second half step (:1950-1952; the half-step gamma again where the K rule
   * ended the move at this step). */
  double* trace;
} emat_skygrid_result;
emat_status emat_skygrid_moves(emat_backend* h, const emat_pop_model* pop_model, const emat_skygrid_spec* spec, double t_ref, double t_step,
                               int32_t first_cell, int32_t num_cells, const double* k_bar /*[num_cells]*/,
                               int32_t num_inner, const double* inner_t /*[num_inner]*/, uint64_t key, emat_skygrid_result* out);
/* The statistics emat_skygrid_moves reads, from the tree resident in HBM as it stands after emat_tree_upload / emat_tree_reassemble (EMAT_ERR_STATE
 * while the parts are out, as the tree probers): the reference's whole-tree grid (Scalable_coalescent_prior, scalable_coalescent.cpp:88-138), k_bar[c]
 * over the cells from the root's to the latest tip's with 1 lineage before the root inside the root's cell, and the times of the inner nodes in node
 * order.  With null k_bar / inner_t only the sizes are returned; EMAT_ERR_BUFFER_TOO_SMALL when an array given is too short.  Cell c is one workgroup
 * adding the branches in a fixed order, no atomics: the same bits from call to call.  The arrays also stay in buffers of the handle, and
 * emat_tree_skygrid_moves is emat_skygrid_moves on them without their leaving HBM: bit for bit what emat_skygrid_moves returns when fed the
 * arrays this call hands out.  Its refusals are emat_skygrid_moves' own, then the tree's state. */
emat_status emat_tree_coalescent_stats(emat_backend* h, double t_ref, double t_step, int32_t* first_cell, int32_t* num_cells, double* k_bar /*[k_bar_capacity] or NULL*/,
                                       int32_t k_bar_capacity, double* inner_t /*[inner_capacity] or NULL*/, int32_t inner_capacity, int32_t* num_inner);
emat_status emat_tree_skygrid_moves(emat_backend* h, const emat_pop_model* pop_model, const emat_skygrid_spec* spec, double t_ref, double t_step, uint64_t key, emat_skygrid_result* out);
emat_status emat_debug_pop_gradient(emat_backend* h, const emat_pop_model* pop_model, int32_t op, int32_t k, int32_t n, const double* a, const double* b, double* out);

/* ---- the Exponential population moves: n0 and the growth rate ----------------------------------------------------------------
 * replaces: the Exp_pop_model branch of Run::run_global_moves (reference run.cpp:754-764): `rounds` times pop_size_move (:1237-1276)
 * then pop_growth_rate_move (:1278-1319), on the device (csrc/emat_exp_pop_kernels.hpp).  Step s = 0 .. 2 rounds - 1 is a Metropolis step,
 * even s on n0, odd s on g, and each re-evaluates Scalable_coalescent_prior::calc_log_prior (scalable_coalescent.cpp:140-187) under the
 * proposed Exp_pop_model{t0, n0, g, min_pop}, its t_c derived afresh as the constructor derives it (pop_model.cpp:32-36), node by node:
 * with the min_pop barrier log N(t) is not linear in (n0, g).
 *
 * Inputs are the statistics of the WHOLE run as emat_skygrid_moves takes them: the lineage grid k_bar[c] over the cells first_cell ..
 * first_cell + num_cells - 1 and the times of the inner nodes.  A sharded caller adds the grids and concatenates the times.
 * `pop_model` is the Exp_pop_model the steps start from.
 *
 * Each evaluation is one launch of G = min(256, ceil(max(num_inner, num_cells) / 1 024)) workgroups of 1 024 threads -- a function of the
 * sizes only -- and each launch begins with every workgroup taking the previous step's decision from the same numbers; the host queues
 * 1 + 2 rounds launches and one closing launch and synchronises once.  Every sum is added in a fixed order (thread, fixed tree over the
 * workgroup, workgroups in order) and there are no atomics: the same arguments give the same result BIT FOR BIT on every handle and in
 * every call.
 *
 * Random numbers: the (key, id) streams of the site-rate moves under the pseudo-id 0xFFFFFFF9, the next below the Skygrid's five.  Step s
 * takes block s of that stream: word 0 the proposal's uniform, word 1 the acceptance uniform, both in [0, 1) and both drawn whether
 * needed or not, so that a step's draws depend on (key, s) alone.
 *   n0 step (:1249-1275)  scale = 0.75 + (1 / 0.75 - 0.75) u0, new_n0 = scale old_n0, log_prior_ratio = -(alpha + 1) log(scale)
 *                         - beta (1 / new_n0 - 1 / old_n0), log_metropolis = (new - old log prior) + log_prior_ratio + log(old_n0 / new_n0).
 *   g step (:1289-1318)   new_g = old_g + (-w + 2 w u0), w = 1 / 365; outside [g_min, g_max] the step ends at once (no evaluation, counted
 *                         in g_out_of_bounds); log_prior_ratio = (|old_g - mu| - |new_g - mu|) / scale; no Hastings term.
 *   both                  accepted when log_metropolis > 0 || u1 < exp(log_metropolis) (a NaN rejects); delta_log_other_priors grows by
 *                         log_prior_ratio.  A disabled move's step does nothing but keeps its block.
 *
 * The call first finishes a pending pass.  It changes nothing in the handle.
 * EMAT_ERR_INVALID_ARGUMENT (text in emat_last_error naming the first offender), all answered before the device is asked for: a null
 * pointer; a model that is not EMAT_POP_EXP (the reference moves only Exp_pop_model, :1239); n0 not finite or <= 0; g or t0 not finite;
 * min_pop negative or not finite; g_min > g_max or either NaN; g outside [g_min, g_max] (:1291); g_prior_scale not finite or <= 0;
 * g_prior_mu or an inverse-gamma parameter not finite; rounds < 0; a trace with trace_capacity < 2 rounds; and emat_skygrid_moves'
 * refusals of t_ref, t_step, num_cells, num_inner, k_bar and inner_t.  EMAT_ERR_CAPACITY: more than 2^22 cells, cell numbers outside
 * [-2^30, 2^30), or rounds > 4 096.  EMAT_ERR_NO_DEVICE: a handle without a device, after the argument checks (there is no CPU path). */
typedef struct emat_exp_pop_spec {          /* Run's setters, reference run.h:64-81, :206-211 */
  int32_t n0_move_enabled, g_move_enabled;   /* final_pop_size_move_enabled_, pop_growth_rate_move_enabled_ */
  double inv_n0_prior_alpha, inv_n0_prior_beta;   /* pop_inv_n0_prior_alpha_, _beta_; reference defaults 0, 0 */
  double g_prior_mu, g_prior_scale, g_min, g_max;   /* pop_g_prior_mu_, ...; 0.001/365, 30.701135/365, -inf, +inf */
  int32_t rounds, pad_;                      /* 50 in the reference (run.cpp:757); 0 = evaluate the prior only */
} emat_exp_pop_spec;
typedef struct emat_exp_pop_step {
  double proposed;                           /* new_n0 (run.cpp:1252) or new_g (:1295); the value held when the move is disabled */
  double log_coalescent_prior_proposed;      /* :1263, :1307; 0 when not evaluated */
  double log_prior_ratio;                    /* :1255-1257, :1300-1301 */
  double log_metropolis, u;                  /* :1265-1267, :1309-1310; u in [0, 1) */
  int32_t accepted, evaluated;               /* evaluated = 0: the move is disabled or new_g left [g_min, g_max] (:1298) */
} emat_exp_pop_step;
typedef struct emat_exp_pop_result {
  double n0, g;                              /* after the round */
  double log_coalescent_prior_start;         /* calc_log_prior under the model passed in */
  double log_coalescent_prior_end;           /* ... under the model returned (run.cpp:1269, :1312) */
  double delta_log_other_priors;             /* :1270, :1313 of the steps accepted */
  int32_t n0_accepted, g_accepted, g_out_of_bounds, pad_;
  emat_exp_pop_step* trace;                  /* may be NULL: room for 2 * rounds records, step s at [s] */
  int32_t trace_capacity;                    /* in: records `trace` has room for (>= 2 * rounds) */
} emat_exp_pop_result;
emat_status emat_exp_pop_moves(emat_backend* h, const emat_pop_model* pop_model, const emat_exp_pop_spec* spec, double t_ref, double t_step,
                               int32_t first_cell, int32_t num_cells, const double* k_bar /*[num_cells]*/,
                               int32_t num_inner, const double* inner_t /*[num_inner]*/, uint64_t key, emat_exp_pop_result* out);
/* emat_exp_pop_moves on the statistics of the tree resident in HBM (emat_tree_coalescent_stats), which never leave it: bit for bit what
 * emat_exp_pop_moves returns when fed the arrays that call hands out.  Its refusals are emat_exp_pop_moves' own, then the tree's state. */
emat_status emat_tree_exp_pop_moves(emat_backend* h, const emat_pop_model* pop_model, const emat_exp_pop_spec* spec, double t_ref, double t_step, uint64_t key, emat_exp_pop_result* out);

/* ---- the substitution-model moves: mu, the HKY frequencies and kappa -----------------------------------------------------------
 * replaces: groups 1 and 2 of Run::run_global_moves (reference run.cpp:703-719): mu_move (:781-821), then `rounds` times
 * hky_frequencies_move (:953-1034) and hky_kappa_move (:1036-1103), on the device (csrc/emat_subst_kernels.hpp) in ONE launch of one
 * workgroup: the Gibbs draw of mu, then the steps s = 0 .. 2 rounds - 1, even s a frequencies step and odd s a kappa step.  The model is
 * the linked HKY model of `spec` (the reference refuses unlinked ones, :791-795); every step derives q from (kappa, pi) as
 * Hky_model::derive_site_evo_model does (evo_hky.cpp:7-50).
 *
 * Inputs are the statistics of the WHOLE run, as SUMS over all handles, exactly as emat_site_rate_moves takes its own: Ttwiddle_beta_a and
 * num_muts_beta_ab as emat_get_global_stats hands them out (num_muts is the sum of the counts off the diagonal), and
 * root_state_counts[a], the number of sites present in state a at the run's root: the reference sequence's counts less the root's
 * deltas and missations (:996-1004), summed over the site partitions.
 *
 *   mu draw (when do_mu)  mu ~ Gamma(shape = num_muts + mu_prior_alpha, rate = sum_{beta, a} q_a Ttwiddle_beta_a + mu_prior_beta), the
 *                         sampler of emat_debug_sample_gamma; delta log G = -(new - old) Ttwiddle + num_muts log(new / old), the other
 *                         priors grow by (alpha - 1) log(new / old) - beta (new - old) (:818-820).
 *   pi step (:964-1033)   d = 0.01 u0, ia = floor(4 u1), ib = (ia + 1 + floor(3 u2)) mod 4 (the law of the reference's redraw loop);
 *                         pi[ia] += d, pi[ib] -= d; a pi that leaves (0, 1) ends the step at once (:977-979, counted in pi_left_unit).
 *                         delta log G = the three sums over branch lengths, root counts and mutations; no prior ratio, no Hastings term.
 *   kappa step (:1049-1102) scale = 0.75 + (1 / 0.75 - 0.75) u0, kappa *= scale; delta log G = the two sums over branch lengths and mutations;
 *                         log_prior_ratio = log of :1064-1067 (log-normal, mean 1, sigma 1.25), Hastings term log(old / new) (:1091).
 *   both                  force_reject as :1007, :1016, :1084 (a count above 0 against a rate or frequency of 0: the step is evaluated, never
 *                         accepted, counted in forced_rejections, and reports 0 for its three sums); else accepted when log_metropolis > 0 ||
 *                         u < exp(log_metropolis) (a NaN rejects).  A disabled move's step does nothing but keeps its draws.
 * The 16 (a, b) terms of a step are formed by 16 lanes and added in the reference's order; no atomics: the same arguments give the same
 * result BIT FOR BIT on every handle and in every call.
 *
 * Random numbers: the (key, id) streams of the site-rate moves under the next two pseudo-ids below the Exponential moves' one:
 *   0xFFFFFFF8  the mu draw, from the stream's start (drawn also when do_mu is 0, provided shape and rate are positive)
 *   0xFFFFFFF7  step s takes the stream's 64-bit words 4 s .. 4 s + 3, all in [0, 1): a pi step u0, u1, u2 and the acceptance uniform; a
 *               kappa step u0 and the acceptance uniform (words 2 and 3 unused).  A step's draws depend on (key, s) alone.
 *
 * The call first finishes a pending pass.  Afterwards the handle's model is the new one, as if given to emat_set_evo: mu for every
 * partition, pi, and q derived from the returned kappa and pi on the host (hky_derive_q, csrc/emat_move_specs.hpp, the run driver's own
 * arithmetic); nu_l, the site partitions and the reference sequence are untouched and nothing L-long is uploaded.
 *
 *   emat_parts_subst_stats   the three statistics from the parts on this handle: k_global_stats' rows reduced on the device in a fixed
 *                            order (one workgroup per column, 256 threads), the root counts from the root part's root node.
 *   emat_parts_subst_moves   emat_subst_moves on those statistics without their leaving HBM: bit for bit what emat_subst_moves returns
 *                            when fed the arrays emat_parts_subst_stats hands out.
 *   emat_get_evo             the model the handle holds (*num_partitions: in the room of the arrays, out the model's P).
 *
 * EMAT_ERR_INVALID_ARGUMENT (text in emat_last_error naming the first offender), all answered before the device is asked for: a null
 * pointer; mu or kappa not finite or <= 0; a pi[a] outside (0, 1) or |sum - 1| > 1e-9; mu_prior_alpha or mu_prior_beta not finite; rounds
 * < 0; a trace with trace_capacity < 2 rounds; num_partitions other than emat_set_evo's; a Ttwiddle that is negative or not finite; a
 * negative count; shape <= 0 or rate <= 0 for the mu draw while do_mu is set.  EMAT_ERR_CAPACITY: more than 4 site partitions, or rounds
 * > 4 096.  EMAT_ERR_STATE: before emat_set_evo; for the parts calls, with no parts out or no root part on this handle.
 * EMAT_ERR_NO_DEVICE: a handle without a device, after these checks.  After any refusal the model is untouched and the next call works. */
typedef struct emat_subst_spec {
  double mu, kappa, pi[4];                   /* the linked HKY model the moves start from */
  double mu_prior_alpha, mu_prior_beta;      /* reference run.h:47-50; defaults 1 and 0 */
  int32_t do_mu, do_pi, do_kappa;            /* which of the moves run */
  int32_t rounds;                            /* 10 in the reference (run.cpp:714); 0 = the mu draw alone */
} emat_subst_spec;
typedef struct emat_subst_step {
  double kappa, pi[4];                       /* held before the step */
  double proposal;                           /* d (a pi step, run.cpp:965) or scale (a kappa step, :1050) */
  double delta_log_G;                        /* :985-1020, :1070-1088; 0 when not evaluated or force-rejected */
  double log_prior_ratio;                    /* log of :1064-1067; 0 for a pi step */
  double log_metropolis, u;                  /* :1022, :1091; u in [0, 1) */
  int32_t ia, ib;                            /* a pi step's two letters (:966-970); -1, -1 for a kappa step */
  int32_t accepted, evaluated;               /* evaluated = 0: the move is disabled or a pi left (0, 1) */
  int32_t left_unit, force_rejected;         /* :977-979; :1007, :1016, :1084 */
} emat_subst_step;
typedef struct emat_subst_result {
  double mu, kappa, pi[4];                   /* after the call */
  double mu_post_shape, mu_post_rate;        /* run.cpp:808-810 */
  double mu_draw;                            /* :813; NaN when do_mu is 0 and shape or rate is not positive */
  double delta_log_G, delta_log_other_priors;          /* of the draw and of every accepted step */
  double mu_delta_log_G, mu_delta_log_other_priors;    /* :818-820 alone; 0 when do_mu is 0 */
  int32_t pi_accepted, kappa_accepted, pi_left_unit, forced_rejections;
  emat_subst_step* trace;                    /* may be NULL: room for 2 * rounds records, step s at [s] */
  int32_t trace_capacity;                    /* in: records `trace` has room for (>= 2 * rounds) */
} emat_subst_result;
emat_status emat_subst_moves(emat_backend* h, const emat_subst_spec* spec, int32_t num_partitions, const double* Ttwiddle_beta_a /*[P][4]*/,
                             const int64_t* num_muts_beta_ab /*[P][4][4]*/, const int64_t* root_state_counts /*[4]*/, uint64_t key, emat_subst_result* out);
emat_status emat_parts_subst_stats(emat_backend* h, double* Ttwiddle_beta_a /*[P][4]*/, int64_t* num_muts_beta_ab /*[P][4][4]*/, int64_t* root_state_counts /*[4]*/);
emat_status emat_parts_subst_moves(emat_backend* h, const emat_subst_spec* spec, uint64_t key, emat_subst_result* out);
emat_status emat_get_evo(emat_backend* h, int32_t* num_partitions, double* mu /*[P]*/, double* pi /*[P][4]*/, double* q /*[P][4][4]*/);

/* ---- the APOBEC (mpox) model's moves: Gibbs rounds of mu and rho = mu* / mu ------------------------------------------------------
 * replaces: the other arm of group 1 of Run::run_global_moves (reference run.cpp:703-719): Run::mpox_hack_moves (:823-951), on the device
 * (csrc/emat_mpox_kernels.hpp) in ONE launch of one wavefront.  The model has two site partitions (Run::set_mpox_hack_enabled, :359-398):
 * 0 = sites without APOBEC context, 1 = sites with it; Jukes-Cantor rates everywhere and on partition 1 the extra rate 2 rho of TC>TT and
 * GA>AA (Run::derive_evo, :400-435; mpox_derive_q of csrc/emat_move_specs.hpp); pi = 0.25 and the same mu in both.
 *
 * Inputs are the statistics of the WHOLE run as emat_get_global_stats hands them out, for the 2 partitions.  From them (:854-905):
 *   M = the sum of the counts off the diagonal       M* = M[1][C][T] + M[1][G][A]
 *   Ttwiddle = the sum of all eight Ttwiddle_beta_a, beta outer and a inner       Ttwiddle* = T[1][C] + T[1][G]
 * Round i = 0 .. rounds - 1 (:908-947):
 *   rho = mu* / mu and Ttwiddle_eff = Ttwiddle + 2 rho Ttwiddle*, at the top of the round
 *   mu draw (when do_mu)   mu ~ Gamma(shape = M + mu_prior_alpha - 1, rate = Ttwiddle_eff + mu_prior_beta), the sampler of
 *                          emat_debug_sample_gamma; delta log G = -(new - old) Ttwiddle_eff + M log(new / old), the other priors grow by
 *                          (alpha - 1) log(new / old) - beta (new - old) (:924-926)
 *   rho draw (when Ttwiddle* > 0; else counted in rho_skipped)   k = 1 + 6 rho from Gamma(alpha = M* + 1, beta = mu Ttwiddle* / 3), with
 *                          the NEW mu, truncated to [1, inf) by inverse transform (safe_sample_truncated_gamma, safe_gamma_math.h:110-139):
 *                          Q_hi = Q(alpha, beta), Q_lo = 0, rand_Q = Q_lo + (Q_hi - Q_lo) u with u in (0, 1], y = Q^-1(alpha, rand_Q),
 *                          k = max(1, y / beta), new_rho = (k - 1) / 6, mu* = mu new_rho;
 *                          delta log G = -2 mu (new_rho - rho) Ttwiddle* + M* log((1 + 6 new_rho) / (1 + 6 rho)), rho the value from the
 *                          top of the round (:939-944).  Where the reference aborts because Q_lo >= Q_hi (Q(alpha, beta) underflows), the
 *                          step ends with rho and mu* unchanged and is counted in rho_degenerate.
 * Q and its inverse are the device's incomplete-gamma routines (emat_debug_gamma), held to 1e-12 + 1e-10 Q and 1e-9 max(1, y) for
 * alpha <= 1 000 and beta <= 1e5.  Every lane of the wavefront runs the same scalar arithmetic; no atomics: the same arguments give the
 * same result BIT FOR BIT on every handle and in every call.
 *
 * Random numbers: the (key, id) streams of the site-rate moves under the next two pseudo-ids below the substitution-model moves':
 *   0xFFFFFFF6  round i's mu draw starts at the stream's 64-bit word 256 i (a draw takes at most 193); drawn also when do_mu is 0,
 *               provided shape and rate are positive
 *   0xFFFFFFF5  round i's rho uniform is word i, in (0, 1]
 * A round's draws depend on (key, i) alone.
 *
 * The call first finishes a pending pass.  Afterwards the handle's model is the new one, as if given to emat_set_evo: mu on both
 * partitions, pi = 0.25, q0 and q1 = mpox_derive_q(mu* / mu) made on the host; nu_l, the site partitions and the reference sequence are
 * untouched and nothing L-long is uploaded.
 *
 *   emat_parts_mpox_moves   emat_mpox_moves on the statistics of the parts on this handle (emat_parts_subst_stats' two arrays; the root
 *                           counts are not read) without their leaving HBM: bit for bit what emat_mpox_moves returns when fed them.
 *
 * EMAT_ERR_INVALID_ARGUMENT (text in emat_last_error naming the first offender), all answered before the device is asked for: a null
 * pointer; mu not finite or <= 0; mu_star not finite or < 0; mu_prior_alpha or mu_prior_beta not finite; rounds < 0; a trace with
 * trace_capacity < rounds; a model on the handle with other than 2 site partitions; a Ttwiddle that is negative or not finite; a negative
 * count; shape <= 0 or rate <= 0 for the first round's mu draw while do_mu is set (a later round's: after the launch, the model untouched).
 * EMAT_ERR_CAPACITY: rounds > 4 096.  EMAT_ERR_STATE: before emat_set_evo; for the parts call, with no parts out or no root part on this
 * handle.  EMAT_ERR_NO_DEVICE: a handle without a device, after these checks.  After any refusal the model is untouched and the next call works. */
typedef struct emat_mpox_spec {
  double mu, mu_star;                        /* the model the rounds start from (Run::mpox_mu_, mpox_mu_star_) */
  double mu_prior_alpha, mu_prior_beta;      /* reference run.h:47-50; defaults 1 and 0 */
  int32_t do_mu;                             /* Run::mu_move_enabled_ (:915) */
  int32_t rounds;                            /* 10 in the reference (:908) */
} emat_mpox_spec;
typedef struct emat_mpox_round {
  double mu, rho, Ttwiddle_eff;              /* held before the round; :911-912 */
  double mu_shape, mu_rate, mu_draw;         /* :916-921; the draw is NaN when do_mu is 0 and shape or rate is not positive */
  double mu_delta_log_G, mu_delta_log_other_priors;   /* :924-926; 0 when do_mu is 0 */
  double alpha, beta, Q_lo, Q_hi, u, rand_Q, y, k, new_rho;   /* the rho draw (safe_gamma_math.h:117-138, run.cpp:940); 0 when skipped, from y on 0 when degenerate */
  double rho_delta_log_G;                    /* :943-944 */
  int32_t mu_done, rho_done, rho_degenerate, reserved;
} emat_mpox_round;
typedef struct emat_mpox_result {
  double mu, mu_star;                        /* after the call */
  double M, M_star, Ttwiddle, Ttwiddle_star; /* :863-866, :897-905 */
  double delta_log_G, delta_log_other_priors;          /* of every draw */
  int32_t rho_skipped, rho_degenerate;       /* rounds whose rho step did not run (Ttwiddle* = 0) / ended on Q_lo >= Q_hi */
  emat_mpox_round* trace;                    /* may be NULL: room for `rounds` records, round i at [i] */
  int32_t trace_capacity;                    /* in: records `trace` has room for (>= rounds) */
} emat_mpox_result;
emat_status emat_mpox_moves(emat_backend* h, const emat_mpox_spec* spec, const double* Ttwiddle_beta_a /*[2][4]*/, const int64_t* num_muts_beta_ab /*[2][4][4]*/,
                            uint64_t key, emat_mpox_result* out);
emat_status emat_parts_mpox_moves(emat_backend* h, const emat_mpox_spec* spec, uint64_t key, emat_mpox_result* out);

/* replaces: Run::calc_cur_log_coalescent_prior (reference run.cpp:455-465), i.e. Scalable_coalescent_prior::calc_log_prior
 * (scalable_coalescent.cpp:163-187) with every node displaced to its current time (:88-138): the whole-tree grid prior
 *   - sum_cells t_step kbar (kbar - 1) / (2 Nbar)  -  sum over inner nodes of log N(t),
 * under the population model last given to emat_build_coalescent_parts / emat_coalescent_begin.  `t_ref` is the time of
 * the latest tip (calc_max_tip_time, run.cpp:40) and cell j is [t_ref + j t_step, t_ref + (j + 1) t_step), j < 0.
 * The grid is additive over nodes and therefore over parts (a cut node counts once, as the coalescence it is), the prior
 * is not linear in it: with parts on several GPUs each rank asks for its partial grid over a common cell range
 * (`first_cell_needed`, all-reduce MIN, tells how far back that must reach; call with num_cells = 0 to get it), the
 * partial grids and log sums are all-reduced (SUM) and any rank evaluates the formula.  A single handle uses the
 * one-call form. */
emat_status emat_scalable_coalescent_partial(emat_backend* h, double t_ref, double t_step, int32_t first_cell, int32_t num_cells,
                                             double* k_bar_partial /*[num_cells], overwritten*/, double* sum_neg_log_pop /* may be NULL */,
                                             int32_t* first_cell_needed /* may be NULL */);
emat_status emat_scalable_coalescent_log_prior(emat_backend* h, double t_ref, double t_step, int32_t first_cell, int32_t num_cells,
                                               const double* k_bar_partial_sum /*[num_cells]*/, double sum_neg_log_pop, double* log_prior);
emat_status emat_get_scalable_coalescent_log_prior(emat_backend* h, double t_ref, double t_step, double* log_prior);

/* Sizes needed to download a part (so that the caller can size an emat_flat_tree). */
emat_status emat_part_get_sizes(emat_backend* h, int32_t part_id, int32_t* num_nodes,
                                int32_t* num_muts, int32_t* num_intervals, int32_t* num_from_states);
/* replaces: reading subrun.tree() in Run::reassemble (reference run.cpp:200-250) */
emat_status emat_part_download(emat_backend* h, int32_t part_id, emat_flat_tree* out);

/* replaces: subrun.lambda_i(), num_sites_missing_at_every_node(), log_G(),
 * log_augmented_coalescent_prior() (reference subrun.h:43-55).  Any pointer may be NULL. */
emat_status emat_part_get_derived(emat_backend* h, int32_t part_id, double* lambda_i /*[num_nodes]*/,
                                  int32_t* num_sites_missing /*[num_nodes]*/, double* log_G,
                                  double* log_augmented_coalescent_prior);

/* replaces: subrun.state_frequencies_of_ref_sequence_per_partition() (reference subrun.h:45-46; Run reads the root part's in
 * check_global_and_local_totals_match, run.cpp:354-355, and the HKY moves use the run's own copy, run.cpp:477): how many sites of
 * every site partition carry each state in the reference sequence the part is written against
 * (calc_state_frequencies_per_partition_of, phylo_tree_calc.cpp:95-106) -- the table the kernels evaluate the root prior from
 * (calc_log_root_prior, phylo_tree_calc.cpp:467-504), refreshed whenever the reference sequence follows the root sequence.
 * `*num_partitions` is in/out (capacity in rows of four, count out); counts[beta * 4 + a]. */
emat_status emat_part_get_state_frequencies(emat_backend* h, int32_t part_id, int32_t* num_partitions, int32_t* counts /*[num_partitions][4]*/);

/* Coalescent-part arrays of one part (reference very_scalable_coalescent.h:47-56), for the
 * cross-part exchange and for tests.  `*num_cells` is in/out (capacity in, length out). */
emat_status emat_part_get_coalescent(emat_backend* h, int32_t part_id, int32_t* num_cells,
                                     double* k_bar_p, double* k_twiddle_bar_p, double* k_twiddle_bar,
                                     double* popsize_bar, int32_t* num_active_parts,
                                     double* t_ref, double* t_step);

/* Where a part's random stream stands (reference: the Subrun's own bit generator, run.cpp:112-114, 182-183): Philox4x32-10 keyed
 * by `key`; `counter` blocks consumed; the unconsumed second 64-bit half of the last block if `has_spare`.  With it, the part's
 * tree and its coalescent arrays, a checker can replay the part's chain from exactly the state the device starts from --
 * also when the parts were cut and their tables built by kernels (emat_tree_repartition).  Any pointer may be NULL. */
emat_status emat_part_get_rng(emat_backend* h, int32_t part_id, uint64_t* key, uint64_t* counter, uint64_t* spare, int32_t* has_spare);

/* Per-part status and move counters. */
typedef struct emat_part_stats {
  int32_t status;                /* 0 = OK; otherwise an emat_status raised inside the kernel */
  int32_t num_nodes;
  int64_t moves_done;
  int64_t proposed[5];           /* inner_displace, tip_displace, branch_reform, subtree_slide, spr1 */
  int64_t accepted[5];
  int64_t algorithmic_bytes;     /* bytes the moves touched, counted with SURVEY section 8(d)'s per-record sizes */
  int64_t rng_draws;
  int64_t device_ticks;          /* 100 MHz wall-clock ticks this part's wavefront spent running moves (cumulative) */
  int64_t algorithmic_write_bytes; /* the part of algorithmic_bytes that is written: coalescent cells, re-timed mutation lists, region records, re-linked nodes */
} emat_part_stats;
emat_status emat_part_get_stats(emat_backend* h, int32_t part_id, emat_part_stats* out);

/* Trace of the first `cfg.trace_moves` moves of a part (tests): 4 doubles per move =
 * {move kind (0..4, -1 = no-op), node X, accepted (0/1), log_mh (NaN when the move exited early)}. */
emat_status emat_part_get_trace(emat_backend* h, int32_t part_id, int32_t* num_moves /*in/out*/,
                                double* trace /*[4*num_moves]*/);

/* Duration of the last emat_run_* launch measured with HIP events on the engine's own stream (milliseconds): the launch of the
 * main size class.  The few parts of the side classes run beside it on streams of their own and are waited for by whatever next
 * reads or changes the parts (emat_synchronize, emat_tree_reassemble, the getters), not by the next emat_run_* call. */
emat_status emat_last_run_ms(emat_backend* h, double* ms);
/* Duration of the dominant kernel (k_run_moves, the bulk size class) inside the last pass, and how many parts it ran. */
emat_status emat_last_kernel_ms(emat_backend* h, double* ms, int32_t* num_parts_in_kernel);

/* ---- test hooks (not part of the boundary) ------------------------------------------------- */
/* Evaluates, on the device and point by point, the engine's own implementations of the regularised upper incomplete gamma
 * function: mode 0: out[i] = Q(a[i], x_or_q[i]); mode 1: out[i] = the x with Q(a[i], x) = x_or_q[i].  They stand in for
 * boost::math::gamma_q / gamma_q_inv (Boost 1.84, reference safe_gamma_math.h:46,68; reached from spr_study.cpp:368,463,544),
 * whose source is not part of the reference tree; tests/test_parity_gpu.py sweeps them over tests/golden/gamma_q.json. */
emat_status emat_debug_gamma(emat_backend* h, int32_t mode, int32_t n, const double* a, const double* x_or_q, double* out);
/* The device's population-model routines, point by point (reference pop_model.cpp:18-145, 247-330): op 0: out[i] = N(a[i])
 * (pop_at_time); op 1: out[i] = integral of N over [a[i], b[i]] (pop_integral); op 2: integral of 1 / N over [a[i], b[i]]
 * (intensity_integral, what the tree probers use).  tests/ sweeps them over the reference's own expectations
 * (tests/golden/reference_expectations.json). */
emat_status emat_debug_pop(emat_backend* h, const emat_pop_model* pop_model, int32_t op, int32_t n, const double* a, const double* b, double* out);
/* The moves' own tree queries on one resident part, query by query (reference phylo_tree.cpp:204-280, 292-299): op 0: out[i] =
 * find_MRCA_of(a[i], b[i]); op 1: out[i] = descends_from(a[i], b[i]) (0 / 1); -1 stands for k_no_node.  tests/ runs them over the
 * reference's own table of cases (phylo_tree_tests.cpp:365-525). */
emat_status emat_debug_tree_query(emat_backend* h, int32_t part_id, int32_t op, int32_t n, const int32_t* a, const int32_t* b, int32_t* out);
/* The moves' own SPR graft machinery on one resident part, with what it found written out as numbers (reference Spr_move,
 * spr_move.h:86-150, spr_move.cpp:9-1156).  `mu_proposal` is the JC69 rate of the proposal (the reference's mu_JC); whether the root
 * sequence may change is the part's includes_run_root flag (the reference's can_change_root).
 *   mode 0: analyze_graft(X);  1: ... + peel_graft;  2: ... + apply_graft of the same graft (a round trip);
 *   mode 3: analyze_graft(X), peel_graft, Spr_move::move(X, new_sibling, new_t_P), propose_new_graft(X) from the part's random
 *           stream, apply_graft, and the part's log G updated by the two delta_log_G as an accepted move does (what the reference's
 *           run_full_spr_move_test steps through, tests/spr_move_tests.cpp:1518-1641).
 * out (doubles): [0] part status afterwards (0 = fine), [1] number of grafts that follow (1; 2 in mode 3: old, then new), each graft as
 *   nbi, delta_log_G, log_alpha_mut, X, S, t_P, then per branch info: A, B, is_open, T_to_X, partial_lambda_at_A, partial_lambda_at_X,
 *   n_warm, (start, end) x n_warm, n_hot, (start, end) x n_hot, n_hot_muts, (site, from, to, t) x n, n_hot_deltas, (site, from, to) x n;
 *   after the first graft, for mode >= 1: count_min_mutations, count_closed_mutations, n, (site, from, to) x n of summarize_closed_mutations.
 * *out_len = doubles needed (EMAT_ERR_CAPACITY when more than out_cap).  tests/ runs it over the reference's own fixtures and expected
 * values (tests/spr_move_tests.cpp:142-1516, as data in tests/golden/reference_expectations.json). */
emat_status emat_debug_graft(emat_backend* h, int32_t part_id, int32_t X, double mu_proposal, int32_t mode, int32_t new_sibling, double new_t_P,
                             double* out, int32_t out_cap, int32_t* out_len);
/* The proposal's JC69 mutational-history sampler on one resident part, history by history (reference sample_mutational_history +
 * adjust_mutational_history, spr_move.cpp:1164-1370, 1409-1439), driven as the reference's own statistical test drives it
 * (tests/spr_move_tests.cpp:1795-1961): history i ends at the point (branch[i], t_end[i]) of the tree and starts T earlier from `start_seq`
 * (num_sites states); its site deltas are where start_seq differs from the tree's sequence at that point.  counts[i] = its number of
 * mutations; muts = (site, from, to, t) per mutation, histories back to back; *num_muts = their total (EMAT_ERR_CAPACITY above muts_cap).
 * Random numbers come from the part's stream. */
emat_status emat_debug_sample_history(emat_backend* h, int32_t part_id, int32_t n, const int32_t* branch, const double* t_end, const uint8_t* start_seq, double T, double mu,
                                      int32_t* counts, double* muts, int32_t muts_cap, int32_t* num_muts);
/* One tree-editing session of the moves' own device code on node X of a resident part (reference Tree_editing_session,
 * tree_editing.cpp:7-302; what Spr_move::move is built from): the constructor, then step i of n_ops: op_kind[i] = 0
 * slide_P_along_branch(op_t[i]), 1 hop_up(), 2 flip(), 3 hop_down(op_node[i]); then end().  lambda_i and the missing-site counts of
 * the nodes are kept up to date by the steps, as in a move (emat_check_derived verifies them afterwards).  tests/ runs the ten
 * cases of the reference's tests/tree_editing_tests.cpp through it. */
emat_status emat_debug_edit(emat_backend* h, int32_t part_id, int32_t X, int32_t n_ops, const int32_t* op_kind, const int32_t* op_node, const double* op_t);
/* Every resident part's remembered missation rate changes -- one number per node, kept beside the node records and put back to "not
 * known" by whatever writes the node's missation lists -- against a fresh evaluation on the lists as they stand: out_2n[2 p] = nodes of
 * part p whose remembered value is known and differs from it in bits (0 unless an invalidation is missing), out_2n[2 p + 1] = nodes whose
 * value is known.  Nothing is recalculated first. */
emat_status emat_debug_miss_dl_check(emat_backend* h, int32_t* out_2n);
/* The device's interval-set algebra on two valid sets given as (start, end) pairs (reference interval_set.h:130-138, 238-500):
 * op 1 merge, 2 intersect, 3 subtract -> pairs in `out` (room for na + nb + 1 pairs), *n_out = their number; op 5 contains
 * (site b[0]), 6 sets intersect -> *n_out = 0 / 1; op 7 / 8: the graft analysis's one-walk split of a by b, its difference (= op 3) /
 * what is left of a (= a minus that difference, entry for entry) -> pairs in `out`. */
emat_status emat_debug_interval_op(emat_backend* h, int32_t op, const int32_t* a, int32_t na, const int32_t* b, int32_t nb, int32_t* out, int32_t* n_out);
/* How often the cut-state pools (out3[0]) and the list heaps (out3[1]) of the HBM-resident tree had to grow (with
 * EMAT_TREE_TIGHT set in the environment they start without any room, so that tests reach those paths), and how many
 * cut-point states needed the large variant of k_gt_measure (out3[2]). */
emat_status emat_debug_tree_counters(emat_backend* h, int32_t* out3);

/* ---- initial-tree construction ------------------------------------------------------------------------
 * replaces: build_usher_like_tree (reference core/phylo_tree.cpp:796-1049; --v0-init-method old_usher_like through
 * build_rough_initial_tree_from_maple, cmdline.cpp:88-121) with its closing passes fix_up_missations (:414-507), pseudo_date
 * (dates.cpp:63-82) and randomize_mutation_times (:567-644).
 * Tip descriptors (reference Tip_desc, phylo_tree.h:137-143, as io.cpp's MAPLE reader fills them): per tip its date range, its
 * differences from the reference sequence of emat_set_ref_sequence (ascending sites; `from` is the reference state) and its
 * missing intervals (sorted, disjoint, non-adjacent).  Tips become nodes 0 .. num_tips-1 in this order, the inner node created
 * for tip X is X + num_tips - 1.  The O(tips x nodes) graft loop runs on the device; the tree is a function of (descriptors,
 * seed).  Input that the reference rejects (site out of range, delta onto the reference state, a site both missing and changed,
 * t_min > t_max, fewer than two tips) is EMAT_ERR_INVALID_ARGUMENT with emat_last_error saying which tip. */
typedef struct emat_tip_descs {
  int32_t num_tips;
  const float*   t_min;          /* [num_tips] */
  const float*   t_max;          /* [num_tips] */
  const int32_t* delta_offset;   /* [num_tips+1] CSR into delta_site / delta_to */
  const int32_t* delta_site;
  const uint8_t* delta_to;
  const int32_t* miss_offset;    /* [num_tips+1] CSR into miss_start / miss_end */
  const int32_t* miss_start;
  const int32_t* miss_end;
} emat_tip_descs;
emat_status emat_tree_build_usher_like(emat_backend* h, const emat_tip_descs* tips, uint64_t seed);
/* The tree it made, as a flat tree (for emat_run_create / emat_tree_upload): sizes, then the arrays. */
emat_status emat_tree_built_sizes(emat_backend* h, int32_t* num_nodes, int32_t* num_muts, int32_t* num_intervals, int32_t* num_from_states);
emat_status emat_tree_built_get(emat_backend* h, emat_flat_tree* out);
/* replaces: build_initial_phylo_tree (reference core/utree.cpp:1892-1925), the reference's DEFAULT initial tree (--v0-init-method
 * mp_plus_timing, cmdline.cpp:113-115, 437): maximum-parsimony guide tree by branch-and-bound insertion (utree.cpp:190-755), up to five
 * rebuilds in nearest-first order (:761-914), SPR refinement of tips and subtrees (:920-1081), rooting by the least-squares regression
 * of divergence on sampling date with the midpoint fall-back (:1085-1464), dating from the fitted rate (:1750-1890), then
 * fix_up_missations and randomize_mutation_times.  Host code, as in the reference (no device needed: works on a device = -1 handle);
 * same descriptors + same seed => the same tree.  The tree is written against the ROOT's sequence, as the reference's is after
 * rereference_to_root_sequence (phylo_tree.cpp:309-322): fetch that sequence with emat_tree_built_ref and hand it on wherever the tree
 * goes (emat_run_create, emat_set_ref_sequence + emat_tree_upload).  report (may be NULL): [0..2] site deltas in the guide tree, after
 * the rebuilds, after SPR refinement; [3] 0 = rooted by regression, 1 = by the midpoint fall-back. */
emat_status emat_tree_build_default(emat_backend* h, const emat_tip_descs* tips, uint64_t seed, int32_t* report /*[4]*/);
emat_status emat_tree_built_ref(emat_backend* h, uint8_t* ref_sequence /*[num_sites]*/);

/* ---- aligned sequences in: consensus, tip deltas and missing runs on the device ----------------------------------------------
 * replaces: what the reference does with the rows of an aligned FASTA once read_fasta (core/io.cpp:14-97) has framed them -- coding each
 * character (to_seq_letter / is_valid_seq_letter, core/sequence.h:77-153), deduce_consensus_sequence (core/sequence_utils.h:44-80) and, per
 * tip, calculate_delta_from_reference (core/sequence_utils.cpp:30-64), in the order of fasta_to_maple (core/cmdline.cpp:26-85).  The framing
 * itself and the dates in the ids are the host's (include/emat_host.h: emat_fasta_load, emat_seq_id_date_range).
 * A store on the handle keeps the rows as 4-bit codes (Seq_letters' bit sets, core/sequence.h:21-29), two sites a byte, each row starting on
 * a byte, beside int32 counts[L][4] of the unambiguous states seen at every site.  L is the handle's num_sites.  Everything is queued on
 * the engine's stream; all arithmetic is on integers, so the results do not depend on how the rows were cut into calls.
 * A handle without a device gets EMAT_ERR_NO_DEVICE: there is no CPU path.
 *
 *   emat_align_begin       binds the store to `max_rows` rows: max_rows x ceil(L/2) bytes, 8 bytes a row of status, and the counts.  What it held
 *                          is released first.  hipMemGetInfo is asked: more than is free is EMAT_ERR_CAPACITY with the sizes in emat_last_error.
 *                          max_rows = 0 releases the room (and is no error on a store never bound).
 *   emat_align_row_buffer  one of two page-locked buffers of the handle (which = 0 / 1) of at least `bytes` bytes, for rows on their way to
 *                          emat_align_push_rows: a push from inside one returns while the copy is in flight, and asking for the same buffer
 *                          again waits for that copy.  Rows pushed from any other memory are read before the push returns.
 *   emat_align_push_rows   num_rows rows of L ASCII characters, row r at chars + r x row_stride, as a FASTA reader holds them after dropping
 *                          line ends.  Every character is coded (case-insensitive, U = T, N - ? . all N) and packed; a row with a character
 *                          that is no sequence letter is INVALID, and the smallest such site and its byte are kept.  The chunk's valid rows
 *                          are added to the counts.  More rows than reserved is EMAT_ERR_CAPACITY: nothing is pushed.
 *   emat_align_finish      the reference sequence is given_ref ([L] of 0..3), or with NULL the consensus: per site the state with the largest
 *                          count, ties to A, then C, then G, then T, an all-zero site A.  Undated rows DO count towards it, invalid rows
 *                          do not (read_fasta drops the invalid rows, fasta_to_maple forms the consensus and only then drops the undated).
 *                          The tips are the rows that are valid and dated (row_dated[r] != 0; NULL: every row is dated), in input order.
 *                          For every tip against the reference sequence: (site, to) at every unambiguous site whose state differs, sites
 *                          ascending; the maximal runs of ambiguous codes as [start, end) -- sorted, disjoint, non-adjacent, as emat_tip_descs
 *                          wants them; `R` next to `N` is ONE run -- and how many ambiguous codes were not N (the reference's
 *                          Ambiguity_precision_loss warnings, counted).  More than INT32_MAX deltas or intervals in all is EMAT_ERR_CAPACITY
 *                          (the CSR offsets of emat_tip_descs are int32).  Fewer than two tips is no error here: the builders refuse that.
 *                          More rows may be pushed afterwards and finish called again.  `out` may be NULL.
 *   emat_align_sizes       the last finish's report
 *   emat_align_get         its arrays; any pointer may be NULL.  The descriptor arrays also stay in HBM: a later change may hand them to
 *                          emat_tree_build_usher_like without the round trip through the host.
 *   emat_align_attach      ties a record of the caller's to the store (the FASTA loader's names and dates): `destroy` is called on it when
 *                          another is attached, at the next emat_align_begin and when the handle goes.  Works without a device, as do
 *                          emat_align_num_sites (the handle's L) and emat_align_refuse, with which a layer above the boundary leaves its
 *                          own refusal in emat_last_error (it returns `status`).
 *
 * EMAT_ERR_STATE: push or finish before emat_align_begin; emat_align_sizes / emat_align_get before a finish that succeeded (or after a
 * push since).  EMAT_ERR_INVALID_ARGUMENT (text in emat_last_error): max_rows < 0, num_rows < 0, row_stride < L, chars NULL with rows
 * to push, a given_ref entry above 3 (the text names the site).  EMAT_ERR_CAPACITY besides the above: so many rows in one push that the
 * launch would exceed 2^31 workgroups.  After any refusal the next call works. */
typedef struct emat_align_report {
  int64_t num_rows;             /* rows pushed */
  int32_t num_tips;             /* valid and dated */
  int32_t num_invalid;          /* rows holding a character that is no sequence letter */
  int32_t num_undated;          /* valid rows with row_dated[r] == 0 */
  int64_t num_deltas;           /* over all tips */
  int64_t num_intervals;
  int64_t num_precision_loss;   /* ambiguous codes other than N, over all tips */
} emat_align_report;
typedef struct emat_align_arrays {
  int32_t* delta_offset;        /* [num_tips + 1]: these six are the arrays of an emat_tip_descs (t_min / t_max are the host's) */
  int32_t* delta_site;          /* [num_deltas] */
  uint8_t* delta_to;            /* [num_deltas] */
  int32_t* miss_offset;         /* [num_tips + 1] */
  int32_t* miss_start;          /* [num_intervals] */
  int32_t* miss_end;            /* [num_intervals] */
  uint8_t* ref_sequence;        /* [L] given_ref, or the consensus */
  int32_t* counts;              /* [L][4] */
  int32_t* row_status;          /* [num_rows] tip index, or -1 undated, or -2 invalid */
  int32_t* row_bad_site;        /* [num_rows] the first site that holds no sequence letter, -1 in a valid row */
  uint8_t* row_bad_byte;        /* [num_rows] ... and the byte found there */
  int32_t* row_precision_loss;  /* [num_rows] ambiguous codes other than N (0 in a row that is no tip: the reference looks at tips only) */
} emat_align_arrays;
emat_status emat_align_begin(emat_backend* h, int64_t max_rows);
emat_status emat_align_row_buffer(emat_backend* h, int32_t which, int64_t bytes, uint8_t** buffer);
emat_status emat_align_push_rows(emat_backend* h, int32_t num_rows, const uint8_t* chars, int64_t row_stride);
emat_status emat_align_finish(emat_backend* h, const uint8_t* given_ref /* [L] of 0..3, or NULL */, const uint8_t* row_dated /* [rows], or NULL = all */, emat_align_report* out);
emat_status emat_align_sizes(emat_backend* h, emat_align_report* out);
emat_status emat_align_get(emat_backend* h, const emat_align_arrays* out);
emat_status emat_align_attach(emat_backend* h, void* record, void (*destroy)(void*));
void* emat_align_attached(const emat_backend* h);
int32_t emat_align_num_sites(const emat_backend* h);
emat_status emat_align_refuse(emat_backend* h, emat_status status, const char* text);

/* Byte breakdown of one part's slab as the backend lays it out (works on host-only handles too): header, node records, coalescent
 * cell table, trace ring, list-heap content, list-heap capacity, scratch, and the number of cells kept. */
emat_status emat_debug_slab_layout(emat_backend* h, int32_t part_id, uint32_t* out8);

#ifdef __cplusplus
}
#endif
#endif /* EMAT_BACKEND_H_ */
