"""The reference's tree probers restated in plain Python, as the yardstick of the device's (emat_tree_probe_*).

Written from the reference's definitions: Staircase / Staircase_family with add_boxcar and add_trapezoid
(core/staircase.{h,cpp}), Tree_prober (core/tree_prober.h), probe_ancestors_on_tree (core/ancestral_tree_prober.cpp) and
probe_site_states_on_tree (core/site_states_tree_prober.cpp), on a flat tree (the arrays of delphy_amd.FlatTree); the
recursions are explicit stacks.  Python floats are IEEE doubles and nothing here is fused, so every intermediate is the
double the reference computes.  A population model is anything with intensity_integral(a, b): OraclePop takes it from the
CPU oracle (orc_intensity_integral, pinned to the reference's pop_model_tests.cpp).

Where the reference's behaviour is undefined the model says what it does, and the device does the same: a cell index that
rounding puts outside [0, cells) is clamped (the reference asserts), and a boxcar or trapezoid whose last cell comes out
before its first is entered as if both ends lay in the first cell (the reference would run past its array).

test_prober_model.py holds this file to the reference's own unit tests (tests/golden/prober_expectations.json)."""
import ctypes as C
import math

import numpy as np


class Staircase:
    def __init__(self, x_start, x_end, num_cells):
        if not (x_start < x_end):
            raise ValueError("Invalid domain: need x_start < x_end, but x_start=%r and x_end=%r" % (x_start, x_end))
        if num_cells <= 0:
            raise ValueError("Number of cells should be positive, not %d" % num_cells)
        self.x_start = float(x_start)
        self.cell_size = (float(x_end) - float(x_start)) / num_cells
        self.f = np.zeros(num_cells)       # (element by element these are the reference's += on doubles, in its order)
        self.touched = np.zeros(num_cells, np.int64)   # fractional terms each cell received } not in the reference:
        self.adds = np.zeros(num_cells, np.int64)      # all terms each cell received        } what the tests' error bound counts

    @property
    def num_cells(self):
        return len(self.f)

    @property
    def x_end(self):
        return self.x_start + self.num_cells * self.cell_size

    def cell_for(self, x):
        return int(math.floor((x - self.x_start) / self.cell_size))

    def at(self, x):
        return self.f[self.cell_for(x)]

    def _clamp(self, c):
        return min(max(c, 0), self.num_cells - 1)

    def cell_for_lbound(self, x):
        return self._clamp(int(math.floor((x - self.x_start) / self.cell_size)))

    def cell_for_ubound(self, x):
        return self._clamp(self.num_cells - 1 - int(math.floor((self.x_end - x) / self.cell_size)))

    def cell_lbound(self, cell):
        return self.x_start + cell * self.cell_size

    def cell_ubound(self, cell):
        return self.cell_lbound(cell) + self.cell_size

    def _frac(self, cell, v):
        self.f[cell] += v
        self.touched[cell] += 1
        self.adds[cell] += 1


def add_boxcar(s, left, right, height):
    if not (left <= right):
        raise ValueError("Invalid domain: need left <= right, but left=%r and right=%r" % (left, right))
    if left > s.x_end or right < s.x_start:
        return
    left = max(left, s.x_start)
    right = min(right, s.x_end)
    if left == right:
        return
    cs, ce = s.cell_for_lbound(left), s.cell_for_ubound(right)
    if ce <= cs:
        s._frac(cs, height * (right - left) / s.cell_size)
        return
    s._frac(cs, height * (s.cell_ubound(cs) - left) / s.cell_size)
    s._frac(ce, height * (right - s.cell_lbound(ce)) / s.cell_size)
    s.f[cs + 1:ce] += height               # the cells in between, whole
    s.adds[cs + 1:ce] += 1


def add_trapezoid(s, left, right, left_height, right_height):
    if not (left <= right):
        raise ValueError("Invalid domain: need left <= right, but left=%r and right=%r" % (left, right))
    if left == right:                      # (the reference divides by zero here and never uses the quotient)
        m = c = float("nan")
    else:
        m = (right_height - left_height) / (right - left)
        c = left_height - m * left

    def y_at(x):
        return m * x + c
    if left > s.x_end or right < s.x_start:
        return
    if left < s.x_start:
        left = s.x_start
        left_height = y_at(left)
    if right > s.x_end:
        right = s.x_end
        right_height = y_at(right)
    if left == right:
        return
    cs, ce = s.cell_for_lbound(left), s.cell_for_ubound(right)
    if ce <= cs:
        s._frac(cs, 0.5 * (left_height + right_height) * (right - left) / s.cell_size)
        return
    first_ubound = s.cell_ubound(cs)
    s._frac(cs, 0.5 * (y_at(left) + y_at(first_ubound)) * (first_ubound - left) / s.cell_size)
    last_lbound = s.cell_lbound(ce)
    s._frac(ce, 0.5 * (y_at(last_lbound) + y_at(right)) * (right - last_lbound) / s.cell_size)
    lb = first_ubound
    for cell in range(cs + 1, ce):
        ub = lb + s.cell_size
        s._frac(cell, 0.5 * (y_at(lb) + y_at(ub)))
        lb = ub


class StaircaseFamily:
    def __init__(self, num_members, x_start, x_end, num_cells):
        if num_members <= 0:
            raise ValueError("Number of members should be positive, not %d" % num_members)
        self.members = [Staircase(x_start, x_end, num_cells) for _ in range(num_members)]

    def __getitem__(self, i):
        return self.members[i]

    def __len__(self):
        return len(self.members)

    x_start = property(lambda self: self.members[0].x_start)
    x_end = property(lambda self: self.members[0].x_end)
    cell_size = property(lambda self: self.members[0].cell_size)
    num_cells = property(lambda self: self.members[0].num_cells)

    def array(self):
        return np.array([m.f for m in self.members], np.float64)

    def touched(self):
        return np.array([m.touched for m in self.members], np.int64)

    def adds(self):
        return np.array([m.adds for m in self.members], np.int64)

    @staticmethod
    def from_array(counts, x_start, cell_size):
        """A family holding `counts` [members][cells] on the grid that starts at x_start with the given cell size (the device's counts)."""
        counts = np.asarray(counts, np.float64)
        fam = StaircaseFamily.__new__(StaircaseFamily)
        fam.members = []
        for row in counts:
            s = Staircase.__new__(Staircase)
            s.x_start, s.cell_size, s.f = float(x_start), float(cell_size), row.copy()
            s.touched = s.adds = np.zeros(len(row), np.int64)
            fam.members.append(s)
        return fam


def tree_prober(counts, cells_to_skip, pop_model, p_initial=None):
    """Tree_prober's constructor: p [members][cells - cells_to_skip]."""
    k = len(counts)
    p_initial = [0.0] * k if p_initial is None else list(p_initial)
    if len(p_initial) != k:
        raise ValueError("Invalid vector of starting probabilities: there are %d values but %d categories" % (len(p_initial), k))
    if any(p < 0.0 for p in p_initial):
        raise IndexError("Starting probabilities can't be negative")
    if sum(p_initial) > 1.0 + 1e-6:
        raise IndexError("Starting probabilities can't add up to more than 1")
    n = counts.num_cells
    out = np.zeros((k, n - cells_to_skip))
    p_before = p_initial
    first = counts[0]
    for cell in range(n):
        t_lbound = first.cell_lbound(cell)
        t_ubound = first.cell_ubound(cell)
        intensity = pop_model.intensity_integral(t_lbound, t_ubound)
        total = 0.0
        for m in counts.members:
            total += float(m.f[cell])
        p_coalesce = 1.0 - math.exp(-total * intensity)
        for cat in range(k):
            p_cat = 0.0 if total == 0.0 else p_coalesce * (float(counts[cat].f[cell]) / total)
            p_ubound = p_cat + (1.0 - p_coalesce) * p_before[cat]
            if cell >= cells_to_skip:
                out[cat, cell - cells_to_skip] = p_ubound
            p_before[cat] = p_ubound
    return out


def _extended_grid(tree, t_start, t_end, num_t_cells):
    """The probers' crude reach back to a root that lies before t_start: (real_t_start, cells, cells_to_skip)."""
    if not (t_start < t_end):
        raise ValueError("Invalid domain: need x_start < x_end")
    if num_t_cells <= 0:
        raise ValueError("Number of cells should be positive")
    real_t_start, skip = t_start, 0
    t_root = float(tree.t[tree.root])
    if t_start > t_root:
        cell_size = (t_end - t_start) / num_t_cells
        while real_t_start > t_root:
            real_t_start -= cell_size
            num_t_cells += 1
            skip += 1
    return real_t_start, num_t_cells, skip


def _children_first_to_last(tree, node):
    return [c for c in (int(tree.child0[node]), int(tree.child1[node])) if c >= 0]


def ancestors_branch_counts(tree, marked, t_start, t_end, num_t_cells):
    """(family, cells_to_skip) of probe_ancestors_on_tree."""
    marked = [int(v) for v in marked]
    n = tree.num_nodes
    for v in marked:
        if not (v == -1 or 0 <= v < n):
            raise IndexError("Node %d is neither `none` (-1) nor inside the valid range [0, %d)" % (v, n))
    k = len(marked)
    first_index = {}
    for i, v in enumerate(marked):
        first_index.setdefault(v, i)
    real_t_start, cells, skip = _extended_grid(tree, t_start, t_end, num_t_cells)
    fam = StaircaseFamily(k + 1, real_t_start, t_end, cells)
    stack = [(int(tree.root), k)]
    while stack:
        node, cma = stack.pop()
        if node != tree.root and cma >= 0:
            add_boxcar(fam[cma], float(tree.t[tree.parent[node]]), float(tree.t[node]), 1.0)
        if node in first_index:
            cma = first_index[node]
        for child in reversed(_children_first_to_last(tree, node)):
            stack.append((child, cma))
    return fam, skip


def probe_ancestors_on_tree(tree, pop_model, marked, t_start, t_end, num_t_cells):
    fam, skip = ancestors_branch_counts(tree, marked, t_start, t_end, num_t_cells)
    k = len(fam) - 1
    return tree_prober(fam, skip, pop_model, [0.0] * k + [1.0])


def state_at_root(tree, ref, site):
    s = int(ref[site])
    r = tree.root
    for j in range(int(tree.mut_offset[r]), int(tree.mut_offset[r + 1])):
        if int(tree.mut_site[j]) == site:
            s = int(tree.mut_to[j])
    return s


def site_states_branch_counts(tree, ref, site, t_start, t_end, num_t_cells):
    """(family, cells_to_skip, state at the root) of probe_site_states_on_tree."""
    if site < 0 or site >= len(ref):
        raise IndexError("Site %d is outside the valid range [1, %d]" % (site + 1, len(ref)))
    real_t_start, cells, skip = _extended_grid(tree, t_start, t_end, num_t_cells)
    root_state = state_at_root(tree, ref, site)
    fam = StaircaseFamily(4, real_t_start, t_end, cells)
    stack = [(int(tree.root), root_state)]
    while stack:
        node, state = stack.pop()
        if node != tree.root:
            parent = int(tree.parent[node])
            hit = None
            for j in range(int(tree.mut_offset[node]), int(tree.mut_offset[node + 1])):
                if int(tree.mut_site[j]) == site:
                    hit = j
                    break
            if hit is not None:
                add_trapezoid(fam[state], float(tree.t[parent]), float(tree.t[node]), 1.0, 0.0)
                state = int(tree.mut_to[hit])
                add_trapezoid(fam[state], float(tree.t[parent]), float(tree.t[node]), 0.0, 1.0)
            else:
                add_boxcar(fam[state], float(tree.t[parent]), float(tree.t[node]), 1.0)
        for child in reversed(_children_first_to_last(tree, node)):
            stack.append((child, state))
    return fam, skip, root_state


def probe_site_states_on_tree(tree, ref, pop_model, site, t_start, t_end, num_t_cells):
    fam, skip, root_state = site_states_branch_counts(tree, ref, site, t_start, t_end, num_t_cells)
    p_initial = [0.0] * 4
    p_initial[root_state] = 1.0
    return tree_prober(fam, skip, pop_model, p_initial)


class OraclePop:
    """intensity_integral of a delphy_amd.PopModel, from the CPU oracle."""

    def __init__(self, pop):
        import oracle_ffi
        self._lib = oracle_ffi.lib()
        self._pop = pop
        self._c = pop.c_struct()

    def intensity_integral(self, a, b):
        return float(self._lib.orc_intensity_integral(C.byref(self._c), a, b))
