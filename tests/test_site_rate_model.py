"""tests/site_rate_model.py held to definitions only (no engine): its delta_log_G against exact_model's log G under two evolution
models, and its log p(alpha) as a density that integrates to one normaliser however the range is cut.  These pin what
test_site_rate_moves_gpu.py compares the device against."""
from fractions import Fraction as F

import mpmath
import numpy as np
import pytest

import exact_model as X
import site_rate_model as SR
from delphy_amd.scenarios import make_scenario
from helpers import split_parts


@pytest.fixture(scope="module")
def scenario():
    return make_scenario("C1", num_tips=60, num_sites=2000)


def _summed_stats(sc, num_parts, ev):
    parts, incl, _, _, ref = split_parts(sc, num_parts, 5)
    tot = None
    for t in parts:
        s = X.stats(t, ref, ev)
        tot = s if tot is None else X.add_stats(tot, s)
    return parts, incl, ref, tot


@pytest.mark.parametrize("num_parts", [1, 6])
def test_delta_log_G_is_the_difference_of_log_G_under_the_two_models(scenario, num_parts):
    sc = scenario
    rng = np.random.default_rng(41)
    nu_old = 0.2 + 1.8 * rng.random(sc.num_sites)
    nu_new = rng.gamma(0.7, 1.0 / 0.7, sc.num_sites) + 1e-12
    nu_new[::97] = SR.NU_FLOOR                                    # floored draws are rates like any other
    ev_old, ev_new = X.Evo.of(sc, nu_old), X.Evo.of(sc, nu_new)
    parts, incl, ref, tot = _summed_stats(sc, num_parts, ev_old)
    assert int(tot["num_muts_l"].sum()) > 0
    before = sum((X.Derived(t, ref, ev_old).part_log_G(r).value for t, r in zip(parts, incl)), F(0))
    after = sum((X.Derived(t, ref, ev_new).part_log_G(r).value for t, r in zip(parts, incl)), F(0))
    Tt = [e.value for e in tot["Ttwiddle_l"]]                    # exact: the statistics do not depend on nu
    got = SR.delta_log_G([sc.mu] * sc.num_sites, Tt, tot["num_muts_l"], nu_old, nu_new)
    want = after - before
    assert abs(got.value - want) <= F(1, 10 ** 40) * abs(want), (float(got.value), float(want))
    assert got.S >= abs(got.value) and got.n == 2 * sc.num_sites


@pytest.mark.parametrize("num_parts", [1, 6])
def test_log_p_alpha_integrates_to_one_normaliser_over_two_splits(scenario, num_parts):
    sc = scenario
    _, _, _, tot = _summed_stats(sc, num_parts, X.Evo.of(sc))
    Tt = [float(e.value) for e in tot["Ttwiddle_l"]]
    mu = [sc.mu] * sc.num_sites
    Z1, _ = SR.alpha_posterior_quadrature(mu, Tt, tot["num_muts_l"], [0, 0.05, 0.5, 2, 8, 40, mpmath.inf], want_mean=False)
    Z2, _ = SR.alpha_posterior_quadrature(mu, Tt, tot["num_muts_l"], [0, 0.2, 1, 4, 20, 100, mpmath.inf], want_mean=False)
    assert Z1 > 0 and abs(Z1 - Z2) <= 1e-8 * Z1, (Z1, Z2)
    # the density itself, at a point, is exp(log_p_alpha - alpha) up to the reference point's constant
    a = 0.37
    lp, lp1 = SR.log_p_alpha(a, mu, Tt, tot["num_muts_l"]), SR.log_p_alpha(1.0, mu, Tt, tot["num_muts_l"])
    assert lp.S >= abs(lp.value) and lp.n == 2 * sc.num_sites + 6
    assert SR.log_metropolis(1.0, a, lp1.f, lp.f).err(-(a - 1.0) + (lp.f - lp1.f) + float(np.log(1.0 / a))) <= SR.log_metropolis(1.0, a, lp1.f, lp.f).bound()
