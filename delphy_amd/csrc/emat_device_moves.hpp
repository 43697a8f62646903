// emat_device_moves.hpp -- the five local moves of reference core/subrun.cpp:98-742 on a part slab.
// NO include guard (see emat_device_core.hpp).

#include "emat_device_spr.hpp"

namespace emat {
namespace EMAT_DEV_NS {

#ifndef EMAT_HOT_BYTES
#define EMAT_HOT_BYTES 1536   // LDS block an SPR1 move sets aside for its candidate scans (sets searched per region, scan items, regions)
#endif
enum { k_inner_node_displace = 0, k_tip_displace = 1, k_branch_reform = 2, k_subtree_slide = 3, k_spr1 = 4 };

// What a move leaves for its trace row (Ctx::tr_*): begin_move says which move it is and that it has neither picked a node nor been
// noted; the move stores the node it picked, once, right after the pick -- a move that returns early leaves the row at that --; and
// note_move adds the verdict to it.
EMAT_D void trace_nothing(Ctx& c, int kind) { c.tr_node = -1; c.tr_kind = (int16_t)kind; c.tr_acc = -1; }
EMAT_D void begin_move(Ctx& c, int kind) { hdr_of(c)->proposed[kind]++; trace_nothing(c, kind); }
EMAT_D void note_move(Ctx& c, double log_mh, bool acc, int kind) { c.tr_log_mh = log_mh; c.tr_acc = acc ? 1 : 0; if (acc) hdr_of(c)->accepted[kind]++; }
EMAT_D bool mh_accept(Ctx& c, double log_mh) { return log_mh >= 0.0 || uniform_co(c, 0.0, 1.0) < m_exp(log_mh); }

// distributions.h:38-69
EMAT_DF double bounded_exponential(Ctx& c, double lambda, double a, double b) {
  double u = u01_oo(c);
  double ltr = lambda * (b - a);
  double x;
  if (lambda == 0.0) x = a + u * (b - a);
  else if (lambda > 0 && ltr > 100) x = b + m_log(u) / lambda;
  else if (lambda < 0 && ltr < -100) x = a + m_log(u) / lambda;
  else x = a + m_log1p(u * (m_exp(ltr) - 1)) / lambda;
  return x < a ? a : (b < x ? b : x);
}
EMAT_DF int pick_random_node(Ctx& c) { return uniform_int(c, hdr_of(c)->n_nodes); }

// subrun.cpp:683-742.  What the move keeps across its calls (the two grafts, the nodes and times it started from) lives in a
// frame of the scratch arena, read back through the context after every call -- like an SPR1 move's Spr1Frame -- instead of
// in registers that every call would make the compiler spill to private memory: with one lane active every private dword
// dirties a 64-byte line of its own.
struct CoreFrame {
  int X, new_branch, P, old_S;
  double new_t, alpha_ratio, old_t_P, d_prior, log_mh;
  Graft old_graft, new_graft;
};
#ifndef EMAT_CF
#define EMAT_CF(c) (*(CoreFrame*)(c).frame)
#endif
EMAT_NOTAIL EMAT_DN void spr_move_core(Ctx& c, int X, int new_branch, double new_t, double alpha_ratio) { EMAT_TIMED(2);
  if (X == hdr_of(c)->root) return;
  if (!c.includes_run_root) if (nodes_of(c)[X].parent == hdr_of(c)->root || new_branch == hdr_of(c)->root) return;
  {
    const double t_X = nodes_of(c)[X].t;
    const int P = nodes_of(c)[X].parent;
    const double new_t_P = new_t;
    if (new_t_P == t_X || new_t_P == nodes_of(c)[new_branch].t || (P != hdr_of(c)->root && new_t_P == nodes_of(c)[nodes_of(c)[P].parent].t)) return;
    if (coal_needs_cells(c, new_t_P)) { stop_for_cells(c, c.tr_kind); return; }   // before the graft is peeled: nothing has changed yet
    CoreFrame* f = (CoreFrame*)sc_alloc(c, (uint32_t)sizeof(CoreFrame));
    if (c.failed) return;
    c.frame = (uint8_t*)f;
    f->X = X; f->new_branch = new_branch; f->P = P; f->old_S = sibling_of(c, P, X);
    f->new_t = new_t; f->alpha_ratio = alpha_ratio; f->old_t_P = nodes_of(c)[P].t;
  }
  c.mu_prop = nodes_of(c)[hdr_of(c)->root].lambda / (c.L - nodes_of(c)[hdr_of(c)->root].n_missing);
  EMAT_PHASE_BEGIN();
  analyze_graft(c, EMAT_CF(c).X, EMAT_CF(c).old_graft);
  peel_graft(c, EMAT_CF(c).old_graft);
  EMAT_PHASE(c, 0);
  spr_move_topology(c, EMAT_CF(c).X, EMAT_CF(c).new_branch, EMAT_CF(c).new_t);
  EMAT_PHASE(c, 1);
  propose_new_graft(c, EMAT_CF(c).X, EMAT_CF(c).new_graft);
  EMAT_PHASE(c, 2);
  if (c.failed) return;
  EMAT_CF(c).d_prior = coal_delta_displace_coalescence(c, EMAT_CF(c).old_t_P, EMAT_CF(c).new_t);
  {
    const CoreFrame& f = EMAT_CF(c);
    EMAT_CF(c).log_mh = (f.new_graft.delta_log_G - f.new_graft.log_alpha_mut) - (f.old_graft.delta_log_G - f.old_graft.log_alpha_mut) + m_log(f.alpha_ratio) + f.d_prior;
  }
  if (c.failed) return;
  const bool acc = mh_accept(c, EMAT_CF(c).log_mh);
  if (c.tr_kind == k_subtree_slide) note_move(c, EMAT_CF(c).log_mh, acc, k_subtree_slide);
  if (acc) {
    apply_graft(c, EMAT_CF(c).new_graft);
    hdr_of(c)->log_G -= EMAT_CF(c).old_graft.delta_log_G; hdr_of(c)->log_G += EMAT_CF(c).new_graft.delta_log_G;
    hdr_of(c)->log_aug_prior += EMAT_CF(c).d_prior;
    coal_coalescence_displaced(c, EMAT_CF(c).old_t_P, EMAT_CF(c).new_t);
  } else {
    spr_move_topology(c, EMAT_CF(c).X, EMAT_CF(c).old_S, EMAT_CF(c).old_t_P);
    apply_graft(c, EMAT_CF(c).old_graft);
  }
  EMAT_PHASE(c, 4);
}

// The three simple moves are compiled twice: kRoot = true for the part that holds the run's root (its root node may be
// displaced, its coalescent grid may grow, branch reforms next to the root go through spr_move_core) and kRoot = false for
// every other part, where none of that can happen: those versions contain no root-only code, and their only calls are the
// out-of-line transcendentals (m_log, m_exp, ...) and the cold halves of the Skygrid ratio and of a node's remembered rate change.
// The kRoot = false versions walk the coalescent cells of a displacement once (coal_delta_displace, kOneWalk); the root part's keep the
// reference's walk per direction: with one walk the HBM variant's run_chain<true> spills one register more across its calls, its frame
// goes from 32 to 48 bytes, and the kernels' ScratchSize from 320 to 336 -- for one part of a run.
// Each is a body that counts its algorithmic bytes into `n`, whichever way it leaves, and a frame that adds them to the context once.
template <bool kRoot> EMAT_DF void inner_node_displace_body(Ctx& c, ByteCount& n) {   // subrun.cpp:148-232
  begin_move(c, k_inner_node_displace);
  int node;
  { EMAT_TIMED(2);   /* inner_displace: pick an inner node */
    int guard = 0; do { node = pick_random_node(c); } while (is_tip(c, node) && guard++ < (1 << 26)); }
  c.tr_node = node;
  const int root = hdr_of(c)->root;
  if (!kRoot && node == root) return;   // node == root && !includes_run_root
  const NodeRec nd = nodes_of(c)[node];
  double t_min = -k_inf;
  if (!kRoot || node != root) {
    t_min = nodes_of(c)[nd.parent].t;
    const MutRec* m = muts_of(c, node);
    for (int i = 0; i < (int)nd.muts.cnt; ++i) t_min = t_min > m[i].t ? t_min : m[i].t;
  }
  double t_max = k_inf;
  const int ch[2] = {nd.child0, nd.child1};
  const double lambda_at_node = nd.lambda;
  double d_logG_dt = 0.0;
  if (!kRoot || node != root) d_logG_dt += -lambda_at_node;
  for (int k = 0; k < 2; ++k) {
    const int cc = ch[k];
    t_max = t_max < nodes_of(c)[cc].t ? t_max : nodes_of(c)[cc].t;
    const MutRec* m = muts_of(c, cc);
    const int nm = nmuts(c, cc);
    for (int i = 0; i < nm; ++i) t_max = t_max < m[i].t ? t_max : m[i].t;
    n.all += 64 + 16 * nm + 24 * (int)nodes_of(c)[cc].miss.cnt;
  }
  { EMAT_TIMED(2);   /* inner_displace: delta_lambda_across_node_missations of both children */
  for (int k = 0; k < 2; ++k) {
    double lambda_just_below = lambda_at_node + delta_lambda_across_node_missations(c, ch[k]);
    d_logG_dt -= -lambda_just_below;
  } }
  n.all += 2 * 64 + 16 * (int)nd.muts.cnt;
  const double old_t = nd.t;
  double log_alpha_ratio = 0.0, new_t = old_t;
  if (kRoot && node == root) {
    double tree_span = c.t_max_tip - t_max;
    EMAT_CHECK(c, tree_span >= 0.0);
    double ds = (1 / nd.lambda) / 2;
    double delta_scale;   // std::min(ds, tree_span)
    if (tree_span < ds) delta_scale = tree_span; else delta_scale = ds;
    new_t = old_t + gaussian(c, 0.0, delta_scale);
    if (new_t < t_min || new_t > t_max) return;
    log_alpha_ratio = 0.0;
  } else {
    EMAT_TIMED(2);   /* inner_displace: bounded_exponential */
    new_t = bounded_exponential(c, d_logG_dt, t_min, t_max);
    log_alpha_ratio = d_logG_dt * (new_t - old_t);
  }
  if (new_t == t_min || new_t == t_max) return;
  if (kRoot) { if (coal_needs_cells(c, new_t)) { stop_for_cells(c, k_inner_node_displace); return; } }   // nothing has changed yet
  double delta_log_G = d_logG_dt * (new_t - old_t);
  double delta_log_prior = coal_delta_displace_coalescence<kRoot, !kRoot>(c, old_t, new_t, n);
  if (c.failed) return;
  double log_mh = delta_log_G + delta_log_prior - log_alpha_ratio;
  bool acc;
  { EMAT_TIMED(2);   /* inner_displace: mh_accept + note_move */
  acc = mh_accept(c, log_mh);
  note_move(c, log_mh, acc, k_inner_node_displace); }
  if (acc) {
    EMAT_TIMED(2);   /* inner_displace: accepted: coal_coalescence_displaced + updates */
    coal_coalescence_displaced<kRoot>(c, old_t, new_t, n);
    nodes_of(c)[node].t = new_t;
    hdr_of(c)->log_G += d_logG_dt * (new_t - old_t);
    hdr_of(c)->log_aug_prior += delta_log_prior;
  }
}
template <bool kRoot> EMAT_NOTAIL EMAT_DN void inner_node_displace_move(Ctx& c) { EMAT_TIMED(2); ByteCount n; inner_node_displace_body<kRoot>(c, n); count_bytes(c, n); }

// The tip displacement and the branch reform each have two entries.  The first draws the move's node and forwards; the second takes a
// node the chain's frame has drawn already (settle_moves, below) and draws nothing for the pick, so every later draw stands where it
// stood in the stream.  The bodies exist once.
EMAT_DF int pick_random_tip(Ctx& c) { int node; int guard = 0; do { node = pick_random_node(c); } while (!is_tip(c, node) && guard++ < (1 << 26)); return node; }
template <bool kRoot> EMAT_DF void tip_displace_body(Ctx& c, ByteCount& n, int node) {   // subrun.cpp:234-285
  c.tr_node = node;
  const NodeRec nd = nodes_of(c)[node];
  if (nd.t_min == nd.t_max) return;
  double t_min;   // std::max(a, b) = a < b ? b : a
  if ((double)nd.t_min < nodes_of(c)[nd.parent].t) t_min = nodes_of(c)[nd.parent].t; else t_min = (double)nd.t_min;
  const MutRec* m = muts_of(c, node);
  for (int i = 0; i < (int)nd.muts.cnt; ++i) t_min = t_min > m[i].t ? t_min : m[i].t;
  const double t_max = (double)nd.t_max;
  const double d_logG_dt = -nd.lambda;
  const double old_t = nd.t;
  n.all += 2 * 64 + 16 * (int)nd.muts.cnt;
  double new_t = bounded_exponential(c, d_logG_dt, t_min, t_max);
  double log_alpha_ratio = d_logG_dt * (new_t - old_t);
  if (new_t == t_min || new_t == t_max) return;
  double delta_log_G = d_logG_dt * (new_t - old_t);
  double delta_log_prior = coal_delta_displace_tip<kRoot, !kRoot>(c, old_t, new_t, n);
  if (c.failed) return;
  double log_mh = delta_log_G + delta_log_prior - log_alpha_ratio;
  bool acc = mh_accept(c, log_mh);
  note_move(c, log_mh, acc, k_tip_displace);
  if (acc) {
    coal_tip_displaced<kRoot>(c, old_t, new_t, n);
    nodes_of(c)[node].t = new_t;
    hdr_of(c)->log_G += d_logG_dt * (new_t - old_t);
    hdr_of(c)->log_aug_prior += delta_log_prior;
  }
}
template <bool kRoot> EMAT_NOTAIL EMAT_DN void tip_displace_move(Ctx& c) { EMAT_TIMED(2); ByteCount n; begin_move(c, k_tip_displace); tip_displace_body<kRoot>(c, n, pick_random_tip(c)); count_bytes(c, n); }
template <bool kRoot> EMAT_NOTAIL EMAT_DN void tip_displace_move_picked(Ctx& c, int node) { EMAT_TIMED(2); ByteCount n; begin_move(c, k_tip_displace); tip_displace_body<kRoot>(c, n, node); count_bytes(c, n); }

// phylo_tree.cpp:579-644; result in scratch
EMAT_DF SVec<MutRec> randomize_branch_mutation_times(Ctx& c, int X) { EMAT_TIMED(2);
  const int n = nmuts(c, X);
  SVec<MutRec> out = sc_vec<MutRec>(c, n);
  if (c.failed) return out;
  const MutRec* old = muts_of(c, X);
  if (X == hdr_of(c)->root) { for (int i = 0; i < n; ++i) push(c, out, old[i]); return out; }
  const double t_X = nodes_of(c)[X].t, t_P = nodes_of(c)[nodes_of(c)[X].parent].t;
  bool complicated = false;
  for (int i = 0; i < n && !complicated; ++i) for (int j = i + 1; j < n; ++j) if (old[i].site == old[j].site) { complicated = true; break; }
  if (!complicated) {
    for (int i = 0; i < n; ++i) { MutRec r = make_mut(old[i].from, old[i].site, old[i].to, uniform_oc(c, t_P, t_X)); r.pad = (uint16_t)i; push(c, out, r); }   // pad: where it came from (reform_factors)
  } else {
    // distinct sites in ascending order; per site, fresh sorted times assigned in the old order
    int prev_site = -1;
    while (true) {
      int l = 0x7fffffff;
      for (int i = 0; i < n; ++i) if (old[i].site > prev_site && old[i].site < l) l = old[i].site;
      if (l == 0x7fffffff) break;
      prev_site = l;
      int first = out.n, k = 0;
      for (int i = 0; i < n; ++i) if (old[i].site == l) { MutRec r = make_mut(old[i].from, old[i].site, old[i].to, uniform_oc(c, t_P, t_X)); r.pad = (uint16_t)i; push(c, out, r); ++k; }
      // sort just the times of this site's block
      for (int a = first + 1; a < first + k && a < out.n; ++a) { double x = out.p[a].t; int b = a - 1; while (b >= first && out.p[b].t > x) { out.p[b + 1].t = out.p[b].t; --b; } out.p[b + 1].t = x; }
    }
  }
  sort_muts(out.p, out.n);
  return out;
}

// What a mutation contributes to a branch's log G besides its time (phylo_tree_calc.h:185-206): A = mu nu (q_from - q_to), the
// factor of (t - t_P), and B = log(mu nu q_from,to).  A branch reform evaluates the reference's sum twice -- over the branch's
// mutations as they are and as re-timed -- and both lists hold the SAME mutations (randomize_branch_mutation_times only draws
// new times): the factors are gathered once, all per-site loads of the branch in one round trip (they used to be one L2 round trip
// and one logarithm per mutation and list, in sequence), and each sum then runs in its own order over the same operands -- bit
// for bit the reference's two numbers.  A re-timed mutation carries the index of the one it came from in its `pad` field.
struct ReformFactors { double* A; double* B; };
// The two factors of one mutation from -> to at a site of partition `pa` and relative rate `nu` (site_part, site_nu): the only spelling
// of these expressions, for reform_factors and branch_reform_small alike.  True when B holds the ARGUMENT of its logarithm and the caller
// still has to take m_log of it (reform_factors takes its logarithms after all loads); false when B came from the staged table.
EMAT_DF bool mut_factors(const Ctx& c, int pa, double nu, int from, int to, double& A, double& B) {
  const double mn = mu_of(c)[pa] * nu;
  const double* q = q_of(c) + pa * 16;
  A = mn * (-q[from * 5] - -q[to * 5]);      // mu nu (q_a(from) - q_a(to)), q_a = -q_aa
  if (c.have_logq && nu == 1.0) { B = emat_lds_logq[pa * 16 + from * 4 + to]; return false; }
  B = mn * q[from * 4 + to];
  return true;
}
EMAT_DF ReformFactors reform_factors(Ctx& c, const MutRec* m, int n) { EMAT_TIMED(2);
  ReformFactors f; f.A = (double*)sc_alloc(c, (uint32_t)n * 16u); f.B = f.A + n;
  if (c.failed) return f;
  uint32_t need_log = 0u; bool all_logs = false;   // which entries still hold the logarithm's argument (bit j for j < 32; beyond: decided again per entry)
  for (int j0 = 0; j0 < n; j0 += 4) {
    int l[4]; int pa[4]; double nu[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) l[k] = m[j0 + k < n ? j0 + k : n - 1].site;
#pragma unroll
    for (int k = 0; k < 4; ++k) { pa[k] = site_part(c, l[k]); nu[k] = site_nu(c, l[k]); }     // eight independent loads in flight
#pragma unroll
    for (int k = 0; k < 4; ++k) if (j0 + k < n) {
      const MutRec& mm = m[j0 + k];
      if (mut_factors(c, pa[k], nu[k], (int)mm.from, (int)mm.to, f.A[j0 + k], f.B[j0 + k])) { need_log |= 1u << ((j0 + k) & 31); if (j0 + k >= 32) all_logs = true; }   // the logarithm is taken below
    }
  }
  if (all_logs) { for (int j = 0; j < n; ++j) if (!(c.have_logq && site_nu(c, m[j].site) == 1.0)) f.B[j] = m_log(f.B[j]); }
  else if (need_log != 0u) { const int n32 = n < 32 ? n : 32; for (int j = 0; j < n32; ++j) if ((need_log >> j) & 1u) f.B[j] = m_log(f.B[j]); }   // entries from 32 on need none (all_logs would be set): never shift by >= 32
  return f;
}
// A branch reform of N = 1..4 mutations at N different sites, in registers: what reform_factors, randomize_branch_mutation_times and
// branch_reform_body's two loops do for such a branch -- the same factors (mut_factors), the same draws at the same stream positions
// in index order, the same stable insertion sort (sort_muts_small), the same two sums over the same operands in the same order
// (reform_delta_small), the same verdict -- without the arena, an SVec or a pointer that may lead to LDS or to HBM: the old records
// are read once, 16 bytes each, and an accepted move stores the N new ones over them (the list's count and capacity stay; the heap,
// its top mark and the node's remembered rate change are not touched).  Out of line, so that the frame of branch_reform_move, which
// three reforms in four leave through the n == 0 path, pays nothing for it.
// Returns the bytes an accepted move stored (16 N, else 0) -- or -1, with nothing drawn and nothing changed, when two of the mutations
// share a site: the caller then takes the general path, as it does for every longer list.
// One difference, in a case no run reaches: the general path stops the part with k_part_overflow when neither the arena nor the part's
// scratch region can hold 48 n bytes; this path needs no such room and goes on.
template <int N> EMAT_DN int branch_reform_small(Ctx& c, int X, double lam, double t_X, double t_P) { EMAT_TIMED(2);
  static_assert(N >= 1 && N <= 4, "the pairwise site test and the unrolled sort are meant for short lists");
  MutRec* const list = (MutRec*)__builtin_assume_aligned(muts_of(c, X), 16);   // heap_alloc hands out multiples of 16 bytes
  ReformMut old[N];
#pragma unroll
  for (int i = 0; i < N; ++i) __builtin_memcpy(&old[i].m, list + i, 16);
  bool twice = false;
#pragma unroll
  for (int i = 0; i < N; ++i) {
#pragma unroll
    for (int j = i + 1; j < N; ++j) twice = twice || old[i].m.site == old[j].m.site;
  }
  if (twice) return -1;
  int pa[N]; double nu[N];
#pragma unroll
  for (int i = 0; i < N; ++i) { pa[i] = site_part(c, old[i].m.site); nu[i] = site_nu(c, old[i].m.site); }   // all loads in flight together
  bool need_log[N];
#pragma unroll
  for (int i = 0; i < N; ++i) need_log[i] = mut_factors(c, pa[i], nu[i], (int)old[i].m.from, (int)old[i].m.to, old[i].A, old[i].B);
#pragma unroll
  for (int i = 0; i < N; ++i) if (need_log[i]) old[i].B = m_log(old[i].B);
  ReformMut nw[N];
#pragma unroll
  for (int i = 0; i < N; ++i) { nw[i] = old[i]; nw[i].m.t = uniform_oc(c, t_P, t_X); nw[i].m.pad = (uint16_t)i; }   // pad: where it came from, as on the general path
  sort_muts_small<N>(nw);
  const double delta_log_G = reform_delta_small<N>(old, nw, lam, t_X, t_P);
  const bool acc = mh_accept(c, delta_log_G);
  note_move(c, delta_log_G, acc, k_branch_reform);
  if (!acc) return 0;
#pragma unroll
  for (int i = 0; i < N; ++i) { nw[i].m.pad = 0; __builtin_memcpy(list + i, &nw[i].m, 16); }
  hdr_of(c)->log_G += delta_log_G;
  return 16 * N;
}
// The longest list branch_reform_small is built for (0: every list with mutations takes the general path).
#ifndef EMAT_REFORM_SMALL_MAX
#define EMAT_REFORM_SMALL_MAX 4
#endif
template <bool kRoot> EMAT_DF void branch_reform_body(Ctx& c, ByteCount& n_bytes, int X) {   // subrun.cpp:287-320, from the pick on
  c.tr_node = X;
  if (X == hdr_of(c)->root) return;
  const int P = nodes_of(c)[X].parent;
  const int S = sibling_of(c, P, X);
  const double t_X = nodes_of(c)[X].t, t_P = nodes_of(c)[P].t;
  // in a part without the run's root, spr_move_core returns at once for a branch next to the subroot (subrun.cpp:689-697)
  if (kRoot) { if (P == hdr_of(c)->root) { spr_move_core(c, X, S, t_P, 1.0); if (c.failed) return; } }
  const double lam = nodes_of(c)[X].lambda;
  const int n = nmuts(c, X);
  if (n == 0) {
    // nothing to re-time (three branches in four at C4): the reference's two branch_log_G are one and the same number, no random
    // number is drawn, and the empty list replaces itself
    const double g = -lam * (t_X - t_P), delta_log_G = g - g;
    n_bytes.all += 2 * 64;
    const bool acc = mh_accept(c, delta_log_G);
    note_move(c, delta_log_G, acc, k_branch_reform);
    if (acc) hdr_of(c)->log_G += delta_log_G;
    return;
  }
  if (n <= EMAT_REFORM_SMALL_MAX) {
    // of the branches with mutations at C4, 55 % carry one, 76 % at most two, 91.5 % at most four, none of them a site twice
    int stored = -1;
    switch (n) {
#if EMAT_REFORM_SMALL_MAX >= 1
      case 1: stored = branch_reform_small<1>(c, X, lam, t_X, t_P); break;
#endif
#if EMAT_REFORM_SMALL_MAX >= 2
      case 2: stored = branch_reform_small<2>(c, X, lam, t_X, t_P); break;
#endif
#if EMAT_REFORM_SMALL_MAX >= 3
      case 3: stored = branch_reform_small<3>(c, X, lam, t_X, t_P); break;
#endif
#if EMAT_REFORM_SMALL_MAX >= 4
      case 4: stored = branch_reform_small<4>(c, X, lam, t_X, t_P); break;
#endif
      default: break;
    }
    if (stored >= 0) { n_bytes.all += 2 * 64 + 2 * 16 * n + stored; n_bytes.written += stored; return; }
  }
  // five mutations or more, or a site twice on the branch
  const ReformFactors f = reform_factors(c, muts_of(c, X), n);
  SVec<MutRec> nm = randomize_branch_mutation_times(c, X);
  if (c.failed) return;
  double g_new = -lam * (t_X - t_P), g_old = g_new;
  { const MutRec* m = nm.p; for (int i = nm.n - 1; i >= 0; --i) { const int j = (int)m[i].pad; g_new -= f.A[j] * (m[i].t - t_P); g_new += f.B[j]; } }
  { const MutRec* m = muts_of(c, X); for (int i = n - 1; i >= 0; --i) { g_old -= f.A[i] * (m[i].t - t_P); g_old += f.B[i]; } }
  const double delta_log_G = g_new - g_old;
  n_bytes.all += 2 * 64 + 2 * 16 * nm.n;
  double log_mh = delta_log_G;
  bool acc = mh_accept(c, log_mh);
  note_move(c, log_mh, acc, k_branch_reform);
  if (acc) {
    for (int i = 0; i < nm.n; ++i) nm.p[i].pad = 0;
    list_assign<MutRec>(c, nodes_of(c)[X].muts, nm.p, nm.n); hdr_of(c)->log_G += delta_log_G; n_bytes.all += 16 * nm.n; n_bytes.written += 16 * nm.n;
  }
}
template <bool kRoot> EMAT_NOTAIL EMAT_DN void branch_reform_move(Ctx& c) { EMAT_TIMED(2);
  ByteCount n;
  begin_move(c, k_branch_reform);
  if (hdr_of(c)->n_nodes >= 3) branch_reform_body<kRoot>(c, n, pick_random_node(c));
  count_bytes(c, n);
}
template <bool kRoot> EMAT_NOTAIL EMAT_DN void branch_reform_move_picked(Ctx& c, int X) { EMAT_TIMED(2); ByteCount n; begin_move(c, k_branch_reform); branch_reform_body<kRoot>(c, n, X); count_bytes(c, n); }

// subrun.cpp:325-350, iterative with an explicit stack in scratch
EMAT_DN SVec<int> enumerate_descendant_branches_straddling(Ctx& c, int P, double t, int X) {
  SVec<int> out; out.n = 0;
  // results grow up from the bottom of a scratch span, the DFS stack grows down from its top
  ScSpan span = sc_span(c, 512);
  out.p = (int*)span.lo; out.cap = 0;
  int* stack_base = (int*)span.hi;
  int sp = 0;
  auto room = [&](int er, int es) -> bool {
    if (span.lo + (size_t)(out.n + er) * 4 + 16 <= span.hi - (size_t)(sp + es) * 4) return true;
    if (!span.lds) return false;
    ScSpan big = sc_span_hbm(c);   // outgrew the LDS arena: migrate
    if (big.lo + (size_t)(out.n + er) * 4 + 16 > big.hi - (size_t)(sp + es) * 4) return false;
    int* no = (int*)big.lo; int* nb = (int*)big.hi;
    for (int i = 0; i < out.n; ++i) no[i] = out.p[i];
    for (int i = 1; i <= sp; ++i) nb[-i] = stack_base[-i];
    span = big; out.p = no; stack_base = nb;
    return true;
  };
  if (!room(0, 1)) { EMAT_FAIL(c, k_part_overflow); return out; }
  stack_base[-(++sp)] = P;
  while (sp > 0 && !c.failed) {
    int n = stack_base[-sp]; --sp;
    if (n == X) continue;
    if (t <= nodes_of(c)[n].t) { if (!room(1, 0)) { EMAT_FAIL(c, k_part_overflow); break; } out.p[out.n++] = n; }
    else if (!is_tip(c, n)) {
      if (!room(0, 2)) { EMAT_FAIL(c, k_part_overflow); break; }
      stack_base[-(++sp)] = nodes_of(c)[n].child1;   // child0 is processed first, as in the recursive original
      stack_base[-(++sp)] = nodes_of(c)[n].child0;
    }
  }
  out.cap = out.n;
  sc_span_commit(c, span, (uint32_t)out.n * 4u);
  return out;
}

EMAT_NOTAIL EMAT_DN void subtree_slide_move(Ctx& c) { EMAT_TIMED(2);   // subrun.cpp:352-448
  begin_move(c, k_subtree_slide);
  if (hdr_of(c)->n_nodes < 2) return;
  const int X = pick_random_node(c);
  c.tr_node = X;
  const int root = hdr_of(c)->root;
  if (X == root) return;
  const int P = nodes_of(c)[X].parent, S = sibling_of(c, P, X);
  double t_early = (P == root) ? (nodes_of(c)[X].t < nodes_of(c)[S].t ? nodes_of(c)[X].t : nodes_of(c)[S].t) : nodes_of(c)[root].t;
  if (P == root) { if (nodes_of(c)[S].t < nodes_of(c)[X].t) t_early = nodes_of(c)[S].t; else t_early = nodes_of(c)[X].t; }   // std::min(tX, tS)
  double tree_span = c.t_max_tip - t_early;
  EMAT_CHECK(c, tree_span >= 0.0);
  double ds = (1 / nodes_of(c)[X].lambda) / 2;
  double delta_scale = tree_span < ds ? tree_span : ds;
  double delta_t = gaussian(c, 0.0, delta_scale);
  const double old_P_t = nodes_of(c)[P].t, new_P_t = old_P_t + delta_t;
  if (delta_t < 0.0) {
    if (P != root && new_P_t < nodes_of(c)[nodes_of(c)[P].parent].t) {
      int GG = nodes_of(c)[P].parent, SS = P;
      while (new_P_t < nodes_of(c)[GG].t) { SS = GG; GG = nodes_of(c)[GG].parent; if (GG == k_no_node) break; }
      SVec<int> branches = enumerate_descendant_branches_straddling(c, SS, old_P_t, X);
      if (c.failed) return;
      double a_o2n = 1.0, a_n2o = 1.0 / (double)branches.n;
      spr_move_core(c, X, SS, new_P_t, a_n2o / a_o2n);
    } else spr_move_core(c, X, S, new_P_t, 1.0);
  } else {
    if (new_P_t > nodes_of(c)[X].t) return;
    if (new_P_t > nodes_of(c)[S].t) {
      SVec<int> branches = enumerate_descendant_branches_straddling(c, P, new_P_t, X);
      if (c.failed) return;
      if (branches.n == 0) return;
      int bi = uniform_int(c, branches.n);
      int SS = branches.p[bi];
      double a_o2n = 1.0 / (double)branches.n, a_n2o = 1.0;
      spr_move_core(c, X, SS, new_P_t, a_n2o / a_o2n);
    } else spr_move_core(c, X, S, new_P_t, 1.0);
  }
}

// subrun.cpp:492-675 in three stretches on lane 0; between them the whole wave scans for candidate regions and weighs them
// (wave_scan_and_study).  A stretch that ends the move clears c.phase; one that parks it sets c.phase and c.svc.
EMAT_D void spr1_park(Ctx& c, int phase) { c.phase = (uint8_t)phase; c.svc = 1; }
EMAT_NOTAIL EMAT_DN void spr1_move_begin(Ctx& c) { EMAT_TIMED(2);
  begin_move(c, k_spr1);
  c.phase = 0;
  if (hdr_of(c)->n_nodes < 2) return;
  const double chooser = uniform_co(c, 0.0, 1.0);
  const int limit = chooser < 0.01 ? 0x7fffffff : 1;
  const int root0 = hdr_of(c)->root;
  c.mu_prop = nodes_of(c)[root0].lambda / (c.L - nodes_of(c)[root0].n_missing);
  int X;
  { int guard = 0; do { X = pick_random_node(c); } while (hdr_of(c)->root == X && guard++ < (1 << 26)); }
  c.tr_node = X;
  if (nodes_of(c)[X].lambda == 0.0) return;
  const int P = nodes_of(c)[X].parent;
  const bool pruning_changes_root = P == hdr_of(c)->root;
  if (pruning_changes_root && !c.includes_run_root) return;
  EMAT_PHASE_BEGIN();
  Spr1Frame* frp = (Spr1Frame*)sc_alloc(c, (uint32_t)sizeof(Spr1Frame));
  if (c.failed) return;
  Spr1Frame& fr = *frp;
  c.frame = (uint8_t*)frp;
  fr.X = X; fr.t_X = nodes_of(c)[X].t; fr.P = P; fr.old_t_P = nodes_of(c)[P].t; fr.old_S = sibling_of(c, P, X); fr.old_G = nodes_of(c)[P].parent;
  fr.limit = limit; fr.f = 0.8 /* annealing factor */; fr.t_max_tip = c.t_max_tip; fr.can_change_root = c.includes_run_root;
  // a part that leaves much of its staging area free (the large parts of a side class, whose scans run to hundreds of items)
  // sets aside half of what is free instead of the fixed block
  {
    const uint32_t a0 = (c.a_top + 15u) & ~15u, free_b = c.a_end > a0 ? c.a_end - a0 : 0u;
    uint32_t hot_b = EMAT_HOT_BYTES;
    if (free_b / 2 > hot_b) hot_b = (free_b / 2 < 32768u ? free_b / 2 : 32768u) & ~15u;
    fr.hot = (limit == 1) ? sc_reserve_hot(c, hot_b) : HotBlock{nullptr, 0};
  }
  analyze_graft(c, X, fr.old_graft);
  peel_graft(c, fr.old_graft);
  EMAT_PHASE(c, 5);
  if (c.failed) return;
  fr.old_min_muts = count_min_mutations(c, fr.old_graft);
  int extra = 4;
  if (limit != 1) { extra = 8; for (int n = 0; n < hdr_of(c)->n_nodes; ++n) if (c.includes_run_root || n != hdr_of(c)->root) extra += nmuts(c, n); }
  fr.extra = extra;
  fr.deltas = summarize_closed_mutations(c, fr.old_graft, extra);
  fr.missing_at_X = reconstruct_missing_sites_at(c, X);
  fr.n_missing_at_X = iv_num_sites(fr.missing_at_X.p, fr.missing_at_X.n);
  fr.lambda_X = nodes_of(c)[X].lambda;
  fr.init_branch = fr.old_S;
  if (c.failed) return;
  spr1_park(c, 1);   // -> scan from the old sibling, study; resumes in spr1_move_propose
}
EMAT_NOTAIL EMAT_DN void spr1_move_propose(Ctx& c) { EMAT_TIMED(2);
  Spr1Frame& fr = *(Spr1Frame*)c.frame;
  c.phase = 0;
  if (c.failed) return;
  EMAT_PHASE_BEGIN();
  const Study& pre = fr.study;
  const int X = fr.X, P = fr.P;
  int new_region; double new_t_P;
  { EMAT_TIMED(2);   /* spr1_propose: pick region, pick time, log_alpha_in_region */
  new_region = study_pick_nexus_region(c, pre);
  new_t_P = study_pick_time_in_region(c, pre, new_region);
  fr.log_alpha_o2n = study_log_alpha_in_region(c, pre, new_region, new_t_P); }
  const int new_S = pre.regions.p[new_region].branch;
  EMAT_CHECK(c, new_S != P);
  fr.pre_new_region_min_muts = pre.regions.p[new_region].min_muts;   // the second scan reuses the regions' storage
  fr.new_S = new_S; fr.new_t_P = new_t_P;
  const double t_new_S = nodes_of(c)[new_S].t;
  int new_G = nodes_of(c)[new_S].parent;
  if (new_G == P) new_G = fr.old_G;
  const double t_new_G = (new_G == k_no_node) ? k_neg_dbl_max : nodes_of(c)[new_G].t;
  if (c.failed) return;
  EMAT_PHASE(c, 7);
  if (new_t_P == fr.t_X || new_t_P == t_new_S || new_t_P == t_new_G) { apply_graft(c, fr.old_graft); return; }
  if (coal_needs_cells(c, new_t_P)) { apply_graft(c, fr.old_graft); if (!c.failed) stop_for_cells(c, k_spr1); return; }   // the old graft goes back on, as after a rejection
  spr_move_topology(c, X, new_S, new_t_P);
  EMAT_PHASE(c, 8);
  propose_new_graft(c, X, fr.new_graft);
  EMAT_PHASE(c, 9);
  if (c.failed) return;
  EMAT_CHECK(c, nodes_of(c)[X].parent == P);
  fr.new_min_muts = count_min_mutations(c, fr.new_graft);
  fr.deltas = summarize_closed_mutations(c, fr.new_graft, fr.extra);
  fr.init_branch = new_S;
  if (c.failed) return;
  spr1_park(c, 2);   // -> scan from the new sibling, study; resumes in spr1_move_finish
}
EMAT_NOTAIL EMAT_DN void spr1_move_finish(Ctx& c) { EMAT_TIMED(2);
  Spr1Frame& fr = *(Spr1Frame*)c.frame;
  c.phase = 0;
  if (c.failed) return;
  EMAT_PHASE_BEGIN();
  const Study& post = fr.study;
  const int X = fr.X;
  const int old_region = study_find_region(post, fr.old_S, fr.old_t_P);
  EMAT_CHECK(c, old_region != -1);
  if (c.failed) return;
  const double log_alpha_n2o = study_log_alpha_in_region(c, post, old_region, fr.old_t_P);
  EMAT_CHECK(c, fr.new_min_muts == fr.pre_new_region_min_muts);
  EMAT_CHECK(c, fr.old_min_muts == post.regions.p[old_region].min_muts);
  EMAT_PHASE(c, 11);
  const double d_prior = coal_delta_displace_coalescence(c, fr.old_t_P, fr.new_t_P);
  if (c.failed) return;
  const double log_mh = (fr.new_graft.delta_log_G - fr.new_graft.log_alpha_mut) - (fr.old_graft.delta_log_G - fr.old_graft.log_alpha_mut)
      + log_alpha_n2o - fr.log_alpha_o2n + d_prior;
  const bool acc = mh_accept(c, log_mh);
  note_move(c, log_mh, acc, k_spr1);
  if (acc) {
    apply_graft(c, fr.new_graft);
    hdr_of(c)->log_G -= fr.old_graft.delta_log_G; hdr_of(c)->log_G += fr.new_graft.delta_log_G;
    hdr_of(c)->log_aug_prior += d_prior;
    coal_coalescence_displaced(c, fr.old_t_P, fr.new_t_P);
  } else {
    EMAT_TIMED(2);   /* spr1_finish: rejected: move back + apply the old graft */
    spr_move_topology(c, X, fr.old_S, fr.old_t_P);
    apply_graft(c, fr.old_graft);
  }
  EMAT_PHASE(c, 12);
}

// ---- slab housekeeping ----------------------------------------------------------------------------------
// Squeeze the garbage out of the list heap by staging all live lists in the (idle) scratch region.
EMAT_DN bool compact_heap(Ctx& c) {
  uint32_t live = 0;
  const int n = hdr_of(c)->n_nodes;
  for (int i = 0; i < n; ++i) {
    live += (((uint32_t)nodes_of(c)[i].muts.cnt * 16u) + 15u) & ~15u;
    live += (((uint32_t)nodes_of(c)[i].miss.cnt * 8u) + 15u) & ~15u;
    live += (((uint32_t)nodes_of(c)[i].mfs.cnt * 8u) + 15u) & ~15u;
  }
  if (live > hdr_of(c)->scratch_end - hdr_of(c)->scratch_begin) return false;
  uint8_t* stage = c.G + hdr_of(c)->scratch_begin;
  uint32_t w = 0;
  for (int i = 0; i < n; ++i) {
    ListRef* refs[3] = {&nodes_of(c)[i].muts, &nodes_of(c)[i].miss, &nodes_of(c)[i].mfs};
    const uint32_t es[3] = {16u, 8u, 8u};
    for (int k = 0; k < 3; ++k) {
      uint32_t bytes = (uint32_t)refs[k]->cnt * es[k];
      const uint64_t* src = (const uint64_t*)heap_at(c, refs[k]->off); uint64_t* dst = (uint64_t*)(stage + w);
      for (uint32_t q = 0; q < bytes / 8; ++q) dst[q] = src[q];
      w += (bytes + 15u) & ~15u;
    }
  }
  uint32_t top = hdr_of(c)->heap_begin, r = 0;
  for (int i = 0; i < n; ++i) {
    ListRef* refs[3] = {&nodes_of(c)[i].muts, &nodes_of(c)[i].miss, &nodes_of(c)[i].mfs};
    const uint32_t es[3] = {16u, 8u, 8u};
    for (int k = 0; k < 3; ++k) {
      uint32_t bytes = (uint32_t)refs[k]->cnt * es[k], padded = (bytes + 15u) & ~15u;
      const uint64_t* src = (const uint64_t*)(stage + r); uint64_t* dst = (uint64_t*)heap_at(c, top);
      for (uint32_t q = 0; q < bytes / 8; ++q) dst[q] = src[q];
      refs[k]->off = top; refs[k]->cap = list_cap_for(padded, es[k]);
      top += padded; r += padded;
    }
  }
  hdr_of(c)->heap_top = top;
  return true;
}

// What is fixed for a whole leg of a part's pass, worked out where the leg fills its context (run_moves_body), not before every move.
// The heap mark up to which a move may start: a move wants `reserve` bytes free -- a quarter of the heap, at least 1 KB, at most
// half the heap.  heap_begin and heap_end do not change during a leg, and compact_heap moves heap_top only.
EMAT_D uint32_t heap_reserve(const Ctx& c) {
  const uint32_t heap_size = hdr_of(c)->heap_end - hdr_of(c)->heap_begin;
  uint32_t reserve = heap_size / 4 > 1024u ? heap_size / 4 : 1024u;
  if (reserve > heap_size / 2) reserve = heap_size / 2;
  return reserve;
}
// The move mix of subrun.cpp:98-121: inner-node displacement 7.5, tip displacement 7.5, branch reform 15, and with the topology moves
// subtree slide 1 and SPR1 1.  The draw that picks a move runs over [0, mix_total).
EMAT_D void begin_leg(Ctx& c) {
  c.heap_limit = hdr_of(c)->heap_end - heap_reserve(c);
  double total_weight = 15.0 + 15.0;
  if (c.topology_moves_enabled) total_weight += 1.0 + 1.0;
  c.mix_total = total_weight;
}
// The heap has less than the reserve free: squeeze the garbage out, and stop the part if that does not make the room.
EMAT_DN bool make_heap_room(Ctx& c) {
  const uint32_t reserve = heap_reserve(c), free_b = hdr_of(c)->heap_end - hdr_of(c)->heap_top;
  if (free_b < reserve) {
    if (!compact_heap(c) || hdr_of(c)->heap_end - hdr_of(c)->heap_top < reserve) { if (hdr_of(c)->status == 0) hdr_of(c)->status = k_part_need_space; return false; }
  }
  return true;
}

// Row `at` of the trace ring for a move settled in the frame, as mcmc_sub_iteration forms it from Ctx::tr_* (the caller has found
// at < trace_cap): kind, node, verdict, log MH ratio; a move that was not noted (acc < 0) reads "not accepted, NaN".
EMAT_DF void store_trace_row(Ctx& c, int at, int kind, int node, int acc, double log_mh) {
  double* tr = (double*)slab_at(c, hdr_of(c)->off_trace) + 4 * at;
  const bool noted = acc >= 0;
  tr[0] = (double)kind; tr[1] = (double)node; tr[2] = noted ? (double)acc : 0.0; tr[3] = noted ? log_mh : __builtin_nan("");
}

// ---- moves that end at once, settled in the chain's frame (parts without the run's root) ------------------------------------------
// Two in five of a chain's moves at C4 change nothing: a tip displacement of a tip whose date is exact (t_min == t_max: every tip of a
// data set with exact dates), a branch reform that picks the part's root, and a branch reform of a branch without mutations, which
// accepts g - g = 0 without a draw and adds 0 to log_G.  What such a move leaves is its draws gone from the stream, three or four
// counters and, when tracing, a row.  settle_moves makes the draw that picks the move and the pick of the node itself -- the same words
// of the stream through the same arithmetic (mix_draw, uniform_pick) -- and, while moves end at once, stays in one straight stretch
// without a call: stream position, moves left and the counters' increments are held in registers and stored once when the run ends.
// Per move it makes the chain's own tests (moves left, rng_pos_wants_fill), so a run ends exactly where the chain would have parked or
// stopped.  It enters with one move's frame begun (run_chain has counted it, mcmc_sub_iteration has checked the heap mark and reset
// the arena; a settled move touches neither, so both still hold for the move that ends the run) and says how it left:
enum {
  k_all_settled = 0,       // every move begun is settled; the chain's loop tests again before it begins the next
  k_move_undrawn,          // one move is begun and nothing of it drawn (the next word lies beyond the words computed ahead)
  k_move_drawn,            // ... its draw `r` is made, nothing else: every kind the stretch does not look into, and a pick that ran out of words
  k_tip_picked,            // ... a tip displacement that is a real move, its tip `node` picked
  k_reform_picked          // ... a branch reform that is a real move, its branch `node` picked
};
struct Unsettled {
  int what; int node; double r;
#ifdef EMAT_PROFILE_PHASES
  long long t0;            // when the move that ends the run began
#endif
};
// The longest run (1: every settled move stores its own counters and goes back to the chain's loop -- the A/B of the run against the pick alone).
#ifndef EMAT_SETTLE_RUN_MAX
#define EMAT_SETTLE_RUN_MAX 0x7fffffffu
#endif
// The draw that picks a move, of the word it takes: uniform_co(c, 0.0, mix_total) spelled on the word.
EMAT_DF double mix_draw(uint64_t word, double mix_total) { return 0.0 + (mix_total - 0.0) * to_co(word); }
EMAT_DF Unsettled settle_moves(Ctx& c) {
  Unsettled u; u.what = k_all_settled; u.node = -1; u.r = 0.0;
  const int n_nodes = (int)uniform_u32((uint32_t)hdr_of(c)->n_nodes), root = (int)uniform_u32((uint32_t)hdr_of(c)->root);
  const int trace_cap = (int)uniform_u32((uint32_t)hdr_of(c)->trace_cap), trace_len = (int)uniform_u32((uint32_t)hdr_of(c)->trace_len);
  const double mix_total = c.mix_total;
  const int64_t left_at_entry = c.moves_left;
  uint32_t pos = uniform_u32(c.rng_pos);
  // moves settled so far, by what they count: exact tips (proposed[1]), reforms that picked the root (proposed[2]), reforms of a branch
  // without mutations (proposed[2], accepted[2], 128 algorithmic bytes); rows written
  uint32_t n_tip = 0, n_root = 0, n_empty = 0, n_rows = 0;
  for (;;) {
#ifdef EMAT_PROFILE_PHASES
    u.t0 = clock64();
#endif
    if (!rng_pos_in_buffer(pos, k_rng_blocks)) { u.what = k_move_undrawn; break; }
    const double r = mix_draw(rng_buffer_word(pos), mix_total);
    pos += 1u;
    int kind = -1, node = -1, acc = -1;
    if (uniform_flag(r < 7.5)) { u.what = k_move_drawn; u.r = r; break; }
    else if (uniform_flag(r < 15.0)) {
      // tip_displace_move's pick loop (pick_random_tip) on the words computed ahead; should they run out, the pick is made again the general way
      const uint32_t pos_at_pick = pos;
      bool ran_out = false;
      int guard = 0;
      do {
        if (!rng_pos_in_buffer(pos, k_rng_blocks)) { ran_out = true; break; }
        node = (int)uniform_u32((uint32_t)uniform_pick(rng_buffer_word(pos), n_nodes));
        pos += 1u;
      } while (uniform_flag(!is_tip(c, node)) && guard++ < (1 << 26));
      if (ran_out) { pos = pos_at_pick; u.what = k_move_drawn; u.r = r; break; }
      if (!uniform_flag(nodes_of(c)[node].t_min == nodes_of(c)[node].t_max)) { u.what = k_tip_picked; u.node = node; break; }
      kind = k_tip_displace; n_tip += 1u;
    } else if (uniform_flag(r < 30.0)) {
      if (n_nodes < 3 || !rng_pos_in_buffer(pos, k_rng_blocks)) { u.what = k_move_drawn; u.r = r; break; }
      node = (int)uniform_u32((uint32_t)uniform_pick(rng_buffer_word(pos), n_nodes));
      pos += 1u;
      kind = k_branch_reform;
      if (node == root) n_root += 1u;
      else {
        if (uniform_flag(nmuts(c, node) != 0)) { u.what = k_reform_picked; u.node = node; break; }
        // branch_reform_body's n == 0 path, its arithmetic as it stands: g - g is 0, accepted without a draw -- unless g is not finite, and
        // then the move, which draws, is made the general way
        const int P = nodes_of(c)[node].parent;
        const double t_X = nodes_of(c)[node].t, t_P = nodes_of(c)[P].t;
        const double lam = nodes_of(c)[node].lambda;
        const double g = -lam * (t_X - t_P), delta_log_G = g - g;
        if (!uniform_flag(delta_log_G >= 0.0)) { u.what = k_reform_picked; u.node = node; break; }
        acc = 1; n_empty += 1u;   // (delta_log_G is +0.0 here: what it adds to log_G is added once, below)
      }
    } else { u.what = k_move_drawn; u.r = r; break; }
    // the move is settled
    if (trace_len + (int)n_rows < trace_cap) { store_trace_row(c, trace_len + (int)n_rows, kind, node, acc, 0.0); n_rows += 1u; }
#ifdef EMAT_PROFILE_PHASES
    { const long long _dt = clock64() - u.t0; hdr_of(c)->phase_ticks[14] += _dt; if (kind == k_tip_displace) EMAT_COUNT(c, 15, _dt); }
#endif
    // the chain's tests before the next move, on the values held here (run_chain makes them again on what is stored below)
    const uint32_t n_settled = n_tip + n_root + n_empty;
    const int64_t left = left_at_entry - (int64_t)(n_settled - 1u);   // c.moves_left as the chain would hold it now: the frame begun at entry is the first settled
    if (uniform_flag(left <= 0) || n_settled == EMAT_SETTLE_RUN_MAX) break;    // (the second: the counts are 32-bit; the chain simply begins another run)
    if (rng_pos_wants_fill(pos, k_rng_blocks, (uint32_t)EMAT_RNG_MARGIN)) break;
  }
  // A run that ends with a move begun has counted that move's frame too.
  const uint32_t n_settled = n_tip + n_root + n_empty, n_begun = n_settled + (u.what == k_all_settled ? 0u : 1u);
  c.rng_pos = pos;
  if (n_settled != 0u) {
    c.moves_left = left_at_entry - (int64_t)(n_begun - 1u);
    hdr_of(c)->proposed[k_tip_displace] += (int64_t)n_tip;
    hdr_of(c)->proposed[k_branch_reform] += (int64_t)(n_root + n_empty);
    hdr_of(c)->accepted[k_branch_reform] += (int64_t)n_empty;
    hdr_of(c)->moves_done += (int64_t)n_settled;
    c.bytes += (int64_t)(2u * 64u * n_empty);
    // log_G += 0.0 once for all of them: x + 0.0 is x for every x but -0.0, which the first addition turns into +0.0 and the later ones leave
    if (n_empty != 0u) hdr_of(c)->log_G += 0.0;
    if (n_rows != 0u) hdr_of(c)->trace_len = trace_len + (int)n_rows;
  }
  return u;
}

// Subrun::mcmc_sub_iteration (subrun.cpp:98-121).  Returns false when the part must stop.  An SPR1 move parks itself
// twice for the wave's scan + study (c.svc != 0 on return): the next call resumes it.
// kRoot: the part holds the run's root (Ctx::includes_run_root, fixed for the part's life).  Only that part can stop a move to have its
// grid regrown and rewind its random stream to the move's first draw (stop_for_cells), so only it remembers where that was.  Every
// other part settles the moves that end at once here, in the frame (settle_moves), and calls a move only when it is a real one.
template <bool kRoot> EMAT_NOTAIL EMAT_D bool mcmc_sub_iteration(Ctx& c) {
#ifdef EMAT_PROFILE_PHASES
  long long _mv0 = clock64();
#endif
  // (what the frame branches on is said to be uniform where it is loaded or returned: uniform_flag, emat_device_core.hpp)
  const uint32_t phase = uniform_u32(c.phase);
  if (phase == 1) spr1_move_propose(c);
  else if (phase == 2) spr1_move_finish(c);
  else {
  // space check BEFORE the move, so that a stop leaves a consistent state
  if (uniform_flag(hdr_of(c)->heap_top > c.heap_limit)) { if (!uniform_flag(make_heap_room(c))) return false; }
  sc_reset(c);
  if (kRoot) c.mv_rng_pos = c.rng_pos;
  if (c.only_displacing_inner_nodes) inner_node_displace_move<kRoot>(c);
  else if (!kRoot) {
    const Unsettled u = settle_moves(c);
    const int what = (int)uniform_u32((uint32_t)u.what);
    if (what == k_all_settled) return true;
#ifdef EMAT_PROFILE_PHASES
    _mv0 = u.t0;
#endif
    if (what == k_tip_picked) tip_displace_move_picked<kRoot>(c, u.node);
    else if (what == k_reform_picked) branch_reform_move_picked<kRoot>(c, u.node);
    else {
      // the general way: the draws settle_moves did not make are made here, through rng_next64
      const double r = what == k_move_drawn ? u.r : uniform_co(c, 0.0, c.mix_total);
      if (r < 7.5) inner_node_displace_move<kRoot>(c);
      else if (r < 15.0) tip_displace_move_picked<kRoot>(c, pick_random_tip(c));
      else if (r < 30.0) { if (hdr_of(c)->n_nodes < 3) begin_move(c, k_branch_reform); else branch_reform_move_picked<kRoot>(c, pick_random_node(c)); }
      else if (c.topology_moves_enabled) { if (r < 31.0) subtree_slide_move(c); else spr1_move_begin(c); }
      else trace_nothing(c, -1);
    }
  } else {
    double r = uniform_co(c, 0.0, c.mix_total);
    if (r < 7.5) inner_node_displace_move<kRoot>(c);
    else if (r < 15.0) tip_displace_move<kRoot>(c);
    else if (r < 30.0) branch_reform_move<kRoot>(c);
    else if (c.topology_moves_enabled) { if (r < 31.0) subtree_slide_move(c); else spr1_move_begin(c); }
    else trace_nothing(c, -1);
  }
  }
#ifdef EMAT_PROFILE_PHASES
  { const long long _dt = clock64() - _mv0; hdr_of(c)->phase_ticks[(c.tr_kind >= 3) ? 15 : 14] += _dt; if (c.tr_kind == 0) EMAT_COUNT(c, 10, _dt); else if (c.tr_kind == 1) EMAT_COUNT(c, 15, _dt); }   // (inner-node / tip displacements apart: reserved[10], [15])
#endif
  if (uniform_u32(c.svc) != 0 && !uniform_flag(c.failed)) return true;   // parked: the move is not over
  c.phase = 0; c.svc = 0;
  if (uniform_flag(hdr_of(c)->status == k_part_need_cells)) return false;   // stopped before the move changed anything (stop_for_cells): not a move
  if (uniform_flag(hdr_of(c)->trace_len < hdr_of(c)->trace_cap)) {
    double* tr = (double*)slab_at(c, hdr_of(c)->off_trace) + 4 * hdr_of(c)->trace_len;
    const bool noted = c.tr_acc >= 0;
    tr[0] = (double)c.tr_kind; tr[1] = (double)c.tr_node; tr[2] = noted ? (double)c.tr_acc : 0.0; tr[3] = noted ? c.tr_log_mh : __builtin_nan("");
    hdr_of(c)->trace_len++;
  }
  hdr_of(c)->moves_done++;
  return !uniform_flag(c.failed);
}

// The chain itself: `c.moves_left` sub-iterations.  Its own function, and its counter in the context, so that nothing is
// live in registers across a move: the moves clobber every register (no callee-saved saves, see the Makefile), and
// whatever their caller kept in registers would be spilled and reloaded around each of them.
// Returns with c.svc != 0 when the current move waits for the wave (the kernel serves it and calls again), else when the
// moves are done or the part had to stop.
// In a part without the run's root, one turn of the loop may settle a whole run of moves that end at once (settle_moves, which counts
// them off c.moves_left itself); the tests at the top of the loop are then made again on what it stored.
template <bool kRoot> EMAT_NOTAIL EMAT_DN void run_chain(Ctx& c) {
  c.svc = 0;
  for (;;) {
    if (uniform_u32(c.phase) == 0) {
      if (uniform_flag(c.moves_left <= 0)) return;
      if (uniform_flag(rng_wants_fill(c))) { c.svc = 2; return; }   // the wave computes the next stretch of the stream (rng_fill), then calls again
      c.moves_left -= 1;
    }
    if (!uniform_flag(mcmc_sub_iteration<kRoot>(c))) { c.moves_left = 0; c.phase = 0; c.svc = 0; return; }
    if (uniform_u32(c.svc) != 0) return;
  }
}
// The one place that asks which kind of part this is: the loop and the three simple moves below it are compiled for each.
EMAT_DF void run_chain_loop(Ctx& c) { if (c.includes_run_root) run_chain<true>(c); else run_chain<false>(c); }

// ---- derived quantities of one part from scratch (Subrun::recalc_derived_quantities, subrun.cpp:17-26;
//      calc_lambda_i phylo_tree_calc.cpp:420-436; calc_num_sites_missing_at_every_node :67-76;
//      calc_log_G_below_root :515-543; calc_log_root_prior :467-504; calc_partial_log_prior
//      very_scalable_coalescent.cpp:355-386).  `ref_freqs` = state counts of the reference sequence per site
//      partition [P][4] (Subrun::state_frequencies_of_ref_sequence_per_partition_).  Executed by ONE lane;
//      the wave-parallel version lives in emat_kernels.hip. --------------------------------------------------
EMAT_DN double calc_log_root_prior(Ctx& c, const int32_t* ref_freqs, int P) {
  const int root = hdr_of(c)->root;
  // counts are adjusted on the fly instead of copying the table
  double result = 0.0;
  for (int p = 0; p < P; ++p) {
    for (int a = 0; a < 4; ++a) {
      int f = ref_freqs[p * 4 + a];
      const MutRec* m = muts_of(c, root);
      for (int i = 0; i < nmuts(c, root); ++i) if (site_part(c, m[i].site) == p) { if (m[i].from == a) --f; if (m[i].to == a) ++f; }
      const IvRec* iv = miss_of(c, root);
      for (int i = 0; i < (int)nodes_of(c)[root].miss.cnt; ++i) for (int l = iv[i].start; l < iv[i].end; ++l) if (site_part(c, l) == p && (int)c.ref[l] == a) --f;
      const FsRec* fs = mfs_of(c, root);
      for (int i = 0; i < (int)nodes_of(c)[root].mfs.cnt; ++i) if (site_part(c, fs[i].site) == p) { if ((int)c.ref[fs[i].site] == a) ++f; if ((int)fs[i].state == a) --f; }
      double pa = pi_of(c)[p * 4 + a];
      if (pa != 0.0) result += f * m_log(pa);
      else if (f != 0) return -k_inf;
    }
  }
  return result;
}

}  // namespace EMAT_DEV_NS
}  // namespace emat
