"""The designed spectrograms of tests/spectrum_cases.py do on the CPU oracle what they are meant to do: every condition
a case states is asserted here from the oracle alone (no device), and the numpy replay of the running-best rule
(FDR_impl.cc:339-409) reproduces the oracle's search on every K3 case.  tests/test_gpu_spectrum_edges.py then holds the
library to the oracle on the same inputs."""
import numpy as np
import pytest

import spectrum_cases as S


@pytest.fixture(scope="module")
def geoms(oracle):
    return S.geom


@pytest.mark.parametrize("name", sorted(S.K2_CASES))
def test_k2_case_condition_holds_on_the_oracle(geoms, name):
    kw, build, cond = S.K2_CASES[name]
    g = geoms(**kw)
    full = build(g)
    k2 = S.k2_oracle(g, full)
    print(name, cond(g, k2))
    # exact sums: the smoothed spectrum is n times the 7-tap sum of the integer profile
    p = full[0].astype(np.int64)
    assert (k2["smraw"] == [g.n * p[g.col(i) - 3:g.col(i) + 4].sum() for i in range(g.finpb)]).all()
    # and the oracle needs nothing outside the band: poison there changes none of its results
    lo, w = g.band()
    k2p = S.k2_oracle(g, S.embed(S.cut(full, lo, w), lo))
    assert k2p["psavg"][lo:lo + w].tobytes() == k2["psavg"][lo:lo + w].tobytes()
    assert S.same_float(k2p["smspec"], k2["smspec"]) and k2p["smraw"].tobytes() == k2["smraw"].tobytes()
    assert k2p["peaks"].tobytes() == k2["peaks"].tobytes()


def test_scalar_copy_geometry_is_what_it_says(geoms):
    g = geoms(**S.ODD_GEOMETRY)
    assert g.n == 349 and g.band()[1] % 2 == 1 and (g.n * g.band()[1]) % 4 != 0
    assert g.n * g.band()[1] * 4 <= 60 * 1024                  # staged in LDS: the copy is taken at all
    g = geoms(**S.EVEN_GEOMETRY)
    assert g.n == 349 and (g.n * g.band()[1]) % 4 == 0 and g.n * g.band()[1] * 4 <= 60 * 1024
    g = geoms(halfbandwidth=60)
    assert g.n * g.band()[1] * 4 > 60 * 1024                   # the unstaged path


def test_widest_pass_band(geoms):
    g = geoms(halfbandwidth=S.WIDEST_HALFBANDWIDTH)
    assert (g.finpb - 1) // 2 > 200 and g.band()[0] >= 0 and sum(g.band()) <= g.size
    with pytest.raises(ValueError):
        S.Geom(halfbandwidth=S.WIDEST_HALFBANDWIDTH + 1)


@pytest.mark.parametrize("name", sorted(S.K3_CASES))
def test_k3_case_condition_holds_and_replay_is_the_search(geoms, name):
    thr, _, _, cond = S.K3_CASES[name]
    g = geoms(threshold=thr)
    full, j = S.k3_build(g, name)
    pk, res, figs = S.k3_figures(g, full, j)        # (asserts replay == search for every candidate)
    print(name, figs)
    cond(g, j, figs)
    lo, w = g.band()
    for q, (c, grid) in enumerate(res):             # poison outside the band: the same search
        cp, gp = g.fdr.search(S.embed(S.cut(full, lo, w), lo), pk[q:q + 1], want_grid=True)
        assert S.same_float(gp, grid) and S.record_diff(cp, c) == []


@pytest.mark.parametrize("kw", [dict(maxdrift=2), dict(cf=6000), dict(cf=24000), dict(halfbandwidth=60)],
                         ids=["maxdrift2", "cf6000", "cf24000", "hb60"])
@pytest.mark.parametrize("name", ["allneg_flat_first_t10", "allneg_flat_last_t10", "allneg_tail_t10", "pruned_t10", "seeded_t10"])
def test_k3_cases_redesigned_for_other_geometries(geoms, kw, name):
    """the designs hold wherever the candidate's column lies; the replay equals the search there too.  The figures of the
    default geometry are not required here (at cf = 24000 most trajectories leave the designed columns and give exact
    zeros; with drifts the other linear hypotheses are not designed): only that the branch is still taken."""
    g = geoms(threshold=10, **kw)
    full, j = S.k3_build(g, name)
    pk, res, figs = S.k3_figures(g, full, j)
    print(name, kw, figs)
    assert j in [f["bin"] for f in figs]
    if g.maxdrift == 0 and name.startswith("allneg"):       # the branch under a negative best is taken there as well
        assert figs[0]["nl_neg"] >= 1 and figs[0]["sync"] < 0 and figs[0]["cstar"] == S.NCELL
    if g.maxdrift == 0 and name.startswith("pruned"):
        S.K3_CASES[name][3](g, j, figs)


def test_replay_on_a_hand_made_grid():
    """the replay itself, on a grid small enough to follow by hand (hc = 126, one linear hypothesis per cell)"""
    grid = np.full((S.NIFR, S.NK0, 126), np.nan, np.float32)
    grid[0, 0, 0] = -0.5         # linear: -0.5 > -1e30
    grid[0, 0, 3] = -0.6         # nonlinear: -0.6 / -0.5 = 1.2 > 1
    grid[0, 0, 4] = -0.55        # -0.55 / -0.6 < 1
    grid[0, 1, 0] = 0.0          # linear: 0 > -0.6
    grid[0, 1, 7] = 1e-3         # nonlinear over a zero best: +inf > 1
    grid[0, 2, 0] = 1e-3         # linear, not strictly greater
    grid[4, 25, 125] = 2e-3      # the very last hypothesis
    (best, gb), acc = S.replay(grid, 1, 1)
    assert [e for e, _, _ in acc] == [0, 3, 126, 126 + 7, S.NCELL * 126 - 1]
    assert [lin for _, _, lin in acc] == [True, False, True, False, False]
    assert best == np.float32(2e-3) and gb == S.NCELL * 126 - 1
    assert acc[3][1] == 0 and acc[1][1] == np.float32(-0.5)
