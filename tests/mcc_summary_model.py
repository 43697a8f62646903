"""emat_mcc_node_times and emat_mcc_mutation_support restated: what a front end collects by looping over every base tree of an MCC tree
with corresponding_node_to (core/mcc_tree.h:91-98, exported at tools/delphy_wasm.cpp:1503-1523).

Inputs: the chosen samples (mcc_model.Sample, or samples_site_states_model.MutSample for the mutations) and the `corr` / `exact` tables of
mcc_model.derive_sets (or the device's, through mcc_correspondence).  Python's `sorted`, explicit loops and the index rules of
include/emat_backend.h; no code of the library.  Every output is one of the inputs' doubles, except mean_t, one sum in sample order
divided once: a comparison with the device is `==`.

  quantile q of m sorted values s:   s[floor(q * float(m - 1))]
  hpd of mass p:                     w = min(m, max(1, ceil(p * float(m)))); the smallest i in [0, m - w] minimising s[i + w - 1] - s[i]

Pure Python / numpy; needs no GPU."""
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np


def quantile_of(s, q):
    """s: sorted ascending."""
    return s[int(math.floor(q * float(len(s) - 1)))]


def hpd_window(m, mass):
    return min(m, max(1, int(math.ceil(mass * float(m)))))


def hpd_of(s, mass):
    """(lo, hi, i*) of the shortest window of hpd_window(m, mass) of the sorted values s, the first on ties."""
    m = len(s); w = hpd_window(m, mass)
    best_i, best_w = 0, s[w - 1] - s[0]
    for i in range(1, m - w + 1):
        width = s[i + w - 1] - s[i]
        if width < best_w: best_i, best_w = i, width
    return s[best_i], s[best_i + w - 1], best_i


@dataclass
class NodeTimes:
    num_exact: np.ndarray              # [nodes]
    q_exact: np.ndarray                # [q][nodes]
    q_mrca: np.ndarray
    hpd_exact: Optional[np.ndarray]    # [2][nodes], None with mass 0
    hpd_mrca: Optional[np.ndarray]
    times: np.ndarray                  # [nodes][M]
    is_exact: np.ndarray               # [nodes][M] bool
    i_star_exact: list                 # [nodes] where the window starts, or None
    i_star_mrca: list


def node_times(samples, corr, exact, nodes=None, quantiles=(), hpd_mass=0.0) -> NodeTimes:
    M = len(samples); n = int(samples[0].parent.shape[0])
    nodes = list(range(n)) if nodes is None else [int(v) for v in nodes]
    cols = len(nodes); nq = len(quantiles)
    out = NodeTimes(np.zeros(cols, np.int32), np.zeros((nq, cols)), np.zeros((nq, cols)), np.zeros((2, cols)) if hpd_mass else None, np.zeros((2, cols)) if hpd_mass else None,
                    np.zeros((cols, M)), np.zeros((cols, M), bool), [None] * cols, [None] * cols)
    for col, v in enumerate(nodes):
        for k in range(M):
            out.times[col, k] = float(samples[k].t[int(corr[k][v])]); out.is_exact[col, k] = bool(exact[k][v])
        everyone = sorted(float(x) for x in out.times[col])
        matching = sorted(float(out.times[col, k]) for k in range(M) if out.is_exact[col, k])
        out.num_exact[col] = len(matching)
        assert len(matching) >= 1, "the master matches itself"
        for j, q in enumerate(quantiles):
            out.q_mrca[j, col] = quantile_of(everyone, q); out.q_exact[j, col] = quantile_of(matching, q)
        if hpd_mass:
            out.hpd_mrca[0, col], out.hpd_mrca[1, col], out.i_star_mrca[col] = hpd_of(everyone, hpd_mass)
            out.hpd_exact[0, col], out.hpd_exact[1, col], out.i_star_exact[col] = hpd_of(matching, hpd_mass)
    return out


@dataclass
class MutationSupport:
    records: list                      # (node, site, from, to) of the master's mutations: node order, each list in stored order
    num_with: np.ndarray
    mean_t: np.ndarray
    t_min: np.ndarray
    t_max: np.ndarray


def mutation_support(samples, corr, exact, master) -> MutationSupport:
    """samples: with mut_offset / mut_site / mut_from / mut_to / mut_t (samples_site_states_model.MutSample)."""
    m = samples[master]; n = int(m.parent.shape[0])
    records, num_with, mean_t, t_min, t_max = [], [], [], [], []
    for v in range(n):
        for j in range(int(m.mut_offset[v]), int(m.mut_offset[v + 1])):
            key = (int(m.mut_site[j]), int(m.mut_from[j]), int(m.mut_to[j]))
            times = []
            for k, s in enumerate(samples):                 # in sample order
                if not exact[k][v]: continue
                c = int(corr[k][v])
                for i in range(int(s.mut_offset[c]), int(s.mut_offset[c + 1])):
                    if (int(s.mut_site[i]), int(s.mut_from[i]), int(s.mut_to[i])) == key:
                        times.append(float(s.mut_t[i])); break    # the first in stored order
            assert times, "the master has its own mutation"
            total = 0.0
            for x in times: total += x
            records.append((v,) + key); num_with.append(len(times)); mean_t.append(total / len(times)); t_min.append(min(times)); t_max.append(max(times))
    return MutationSupport(records, np.array(num_with, np.int32), np.array(mean_t, np.float64), np.array(t_min, np.float64), np.array(t_max, np.float64))
