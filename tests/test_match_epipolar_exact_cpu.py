"""The restatements of the matcher and of the two-view geometry (tests/matchref.py, tests/epiref.py) against references that
share nothing with them: the squared distance in f64 (matchref.exact_d2), the nearest neighbour under it, and the Sampson
inequality in exact rational arithmetic (epiref.exact_inlier).  The bounds are derived (matchref.d2_bound, the docstring of
epiref.exact_inlier), not measured; the measured figures are printed.  tests/test_gpu_match_limits.py and
tests/test_gpu_epipolar_limits.py run the same checks on the device's own outputs."""
import functools

import numpy as np
import pytest

from tests import epiref, matchref
from tests.test_gpu_match import crafted


@functools.lru_cache(maxsize=None)
def exact_sets(signed):
    """The 1000 x 777 crafted sets (no NaN rows, no duplicated train rows) -> (q, t, exact_d2 [1000, 777], d2_bound [1000, 777])."""
    rng = np.random.default_rng(1000 * 1000 + 777 + int(signed))
    if signed:
        t = matchref.crafted(rng, 777, signed=True)
        q = matchref.crafted(rng, 1000, t, signed=True)
    else:
        t = crafted(rng, 777)
        q = crafted(rng, 1000, t)
    exact, bound = matchref.exact_d2(q, t), matchref.d2_bound(q, t)
    for a in (q, t, exact, bound):
        a.setflags(write=False)
    return q, t, exact, bound


def check_nn_against_exact(nn, exact, bound, what):
    """C1 on an nn array: dist2 is within B of the exact distance to the row it names; dist2 and second_dist2 are within
    max_j B of the exact smallest and second smallest (an order statistic moves by no more than the largest perturbation).
    C2: where the exact margin exceeds 2 max_j B the index is the exact nearest; at most 2 % of the queries are undecided."""
    n = len(nn)
    rows = np.arange(n)
    assert (nn["index"] >= 0).all()
    order = np.sort(exact, axis=1)
    bmax = bound.max(axis=1)
    r_own = np.abs(nn["dist2"].astype(np.float64) - exact[rows, nn["index"]]) / bound[rows, nn["index"]]
    r_best = np.abs(nn["dist2"].astype(np.float64) - order[:, 0]) / bmax
    r_second = np.abs(nn["second_dist2"].astype(np.float64) - order[:, 1]) / bmax
    decided = order[:, 1] - order[:, 0] > 2 * bmax
    wrong = int((nn["index"][decided] != exact.argmin(axis=1)[decided]).sum())
    print(f"{what}: worst |dist2 - exact| / B {r_own.max():.4f}, smallest / max B {r_best.max():.4f}, second / max B {r_second.max():.4f}; "
          f"undecided {100.0 * (~decided).mean():.2f} % of {n}, wrong among the decided {wrong}; negative dist2 {int((nn['dist2'] < 0).sum())}")
    assert r_own.max() <= 1.0 and r_best.max() <= 1.0 and r_second.max() <= 1.0
    assert wrong == 0
    assert (~decided).mean() <= 0.02


@pytest.mark.parametrize("signed", [False, True])
def test_c1_every_d2_of_the_restatement_is_within_the_derived_bound_of_f64(signed):
    q, t, exact, bound = exact_sets(signed)
    ratio = np.abs(matchref.d2_all(q, t).astype(np.float64) - exact) / bound
    print(f"C1 {'signed' if signed else 'unsigned'}: worst |d2 - exact| / B over {ratio.size} pairs: {ratio.max():.4f}")
    assert ratio.max() <= 1.0
    assert matchref.d2_all(q[:3], t[:5]).tobytes() == np.float32([[matchref.d2(a, b) for b in t[:5]] for a in q[:3]]).tobytes()


@pytest.mark.parametrize("signed", [False, True])
def test_c1_c2_nearest_two_of_the_restatement_against_exact_arithmetic(signed):
    q, t, exact, bound = exact_sets(signed)
    nn, _ = matchref.match(q, t)
    check_nn_against_exact(nn, exact, bound, "C1/C2 restatement, " + ("signed" if signed else "unsigned"))


def check_flags_against_exact(F, xy, flags, max_dist2):
    """C3 for one pair -> (records, exempt, disagreeing): every trusted record's flag is the exact predicate unless the two
    sides are within the exemption of each other; a record that is not trusted is no inlier."""
    inl, near, trusted = epiref.exact_inlier(F, xy, max_dist2)
    assert not flags[~trusted].any()
    return int(trusted.sum()), int((near & trusted).sum()), int((flags != inl)[trusted & ~near].sum())


def test_c3_inlier_flags_of_the_restatement_against_the_exact_sampson_predicate():
    total = np.zeros(3, np.int64)
    for seed in (1, 2, 3, 4):
        mt, qp, tp, _ = epiref.planted_scene(seed)
        model, flags, _ = epiref.ransac(mt, qp, tp, 512, seed, 4.0)
        assert int(model["best"][0]) >= 0 and flags.sum() > 100
        total += check_flags_against_exact(model["F"][0], epiref.coords(mt, qp, tp), flags, 4.0)
    print(f"C3 restatement: {total[0]} records, {total[1]} exempt, {total[2]} disagreeing")
    assert total[2] == 0 and total[1] <= 0.01 * total[0]


def test_exact_inlier_on_a_case_worked_by_hand():
    # F = antisymmetric [t]_x of t = (1, 0, 0): the epipolar lines are the rows, x'^T F x = y - y'
    F = np.array([0, 0, 0, 0, 0, -1, 0, 1, 0], np.float64)
    xy = np.array([[3, 5, 9, 5], [3, 5, 9, 6], [3, 5, 9, 7], [np.nan] * 4, [3, 5, 9, 5 + 2.0 ** -30]], np.float64)
    # e = y - y', den = 2: inlier iff (y - y')^2 < 2 max_dist2; at max_dist2 = 0.5 the second record sits exactly on the edge
    inl, near, trusted = epiref.exact_inlier(F, xy, 0.5)
    assert inl.tolist() == [True, False, False, False, True] and trusted.tolist() == [True, True, True, False, True]
    assert near.tolist() == [False, True, False, False, False]
    n, flags = epiref.score(F, xy, 0.5)
    assert flags.tolist() == inl.tolist() and n == 2
