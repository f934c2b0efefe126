"""Descriptor matching on the GPU at the detector's capacity and on hostile values (vslam_match_dev, include/vslam.h): bytes-equal
against tests/matchref.py like tests/test_gpu_match.py, but with more than one 16384-row chunk of the ordered list per pair, 626
train tiles dealt to 16 splits, 1500 pairs in one call, and rows with mixed signs, near copies (negative d2), subnormals,
overflow to +inf, inf - inf and - at the very top of the range - a d2 of -inf that wins, single Inf / NaN entries and -0.0.  The last test compares the device's own nn with f64
arithmetic (matchref.exact_d2), with no restatement in between.

Every "require" comment marks a condition on the input, evaluated on the restatement's answer alone: the case only
exercises what it is for while it holds."""
import numpy as np
import pytest

from tests import matchref
from tests.test_gpu_match import check_pair, crafted, env, make_pair, run_dev  # noqa: F401 (env: the module's fixture)
from tests.test_match_epipolar_exact_cpu import check_nn_against_exact, exact_sets
from visualslam_amd import capi

pytestmark = pytest.mark.gpu
CHUNK = 16384  # query rows per workgroup of the count -> scan -> scatter kernels: 256 flag words of 64 rows


# ---- A. capacity

def test_a1_40037_queries_three_chunks_of_the_ordered_list(env):
    ctx, torch = env
    rng = np.random.default_rng(101)
    nq, nt, qcap, tcap = 40037, 70, 65536, 72
    td = crafted(rng, nt)
    qd = crafted(rng, nq, base=td)
    planted = {16383: 3, 16384: 11, 32767: 24, 32768: 40, 40036: 69}  # query row -> the train row it copies (no train row is duplicated)
    for qrow, trow in planted.items():
        qd[qrow] = td[trow]
    qs, ts = (qd, None, None, nq), (td, None, None, nt)
    wnn, wm = matchref.match(qd, td)
    per_chunk = np.bincount(wm["query"] // CHUNK, minlength=3)
    # require: 25 % .. 75 % accepted, some in each chunk, the planted rows accepted with distance exactly 0
    assert 0.25 * nq <= len(wm) <= 0.75 * nq and (per_chunk > 0).all(), (len(wm), per_chunk)
    for qrow, trow in planted.items():
        assert wnn[qrow]["index"] == trow and wnn[qrow]["dist2"] == 0.0 and qrow in wm["query"], qrow
    cut = int(per_chunk[0]) + 5  # the cut falls inside chunk 1
    assert per_chunk[0] < cut < per_chunk[0] + per_chunk[1]
    for match_cap in (qcap, cut, 1):
        got = run_dev(ctx, torch, [qs], [ts], qcap, tcap, match_cap=match_cap)
        check_pair(got, 0, qs, ts, qcap, tcap, 0.64, False, match_cap)


def test_a2_40037_train_rows_626_tiles_dealt_to_16_splits(env):
    ctx, torch = env
    rng = np.random.default_rng(102)
    nq, nt, qcap, tcap = 70, 40037, 72, 65536
    td = crafted(rng, tcap)          # every row of the capacity is real data: the second run uses them all
    tdf = np.ones(tcap, np.uint8)
    j = 100                          # tile 1; + 64 * 5: tile 6, another split; + 64 * 16: tile 17, the same split as tile 1
    td[j + 64 * 5] = td[j]
    td[j + 64 * 16] = td[j]
    tdf[200] = 0                     # an undefined row that would be the best
    td[300] = np.nan
    qd = crafted(rng, qcap, base=td[:nt])
    for qrow, trow in enumerate((0, 63, 64, nt - 1, j, 200)):
        qd[qrow] = td[trow]
    wnn, _ = matchref.match(qd[:nq], td[:nt], t_defined=tdf[:nt])
    # require: the planted winners win, the lowest index of the triple with second == best, the skipped rows never
    assert wnn["index"][:4].tolist() == [0, 63, 64, nt - 1] and (wnn["dist2"][:4] == 0.0).all() and (wnn["second_dist2"][:4] > 0.0).all()
    assert (wnn[4]["index"], wnn[4]["dist2"], wnn[4]["second_dist2"]) == (j, 0.0, 0.0)
    assert wnn[5]["index"] != 200 and wnn[5]["dist2"] > 0.0 and (wnn["index"] != 300).all() and (wnn["index"] >= 0).all()
    for counts in ((nq, nt), (100000, 100000)):  # the second: min(count, cap) rows on both sides, 1024 train tiles
        qs, ts = (qd, None, None, counts[0]), (td, tdf, None, counts[1])
        got = run_dev(ctx, torch, [qs], [ts], qcap, tcap)
        check_pair(got, 0, qs, ts, qcap, tcap, 0.64, False, qcap)


def test_a3_1500_small_pairs_in_one_call(env):
    ctx, torch = env
    rng = np.random.default_rng(103)
    n, cap, match_cap = 1500, 8, 3
    pairs = []
    for _ in range(n):
        qs, ts = make_pair(rng, int(rng.integers(0, cap + 1)), int(rng.integers(0, cap + 1)), octaves=True, specials=False)
        if qs[3] >= 1 and ts[3] >= 3:    # a duplicated train row and a query equal to both: the tie goes to the lower index
            ts[0][2] = ts[0][0]
            ts[2][2] = ts[2][0]
            qs[0][0] = ts[0][0]
            qs[2][0] = ts[2][0]
        pairs.append((qs, ts))
    qsets, tsets = [p[0] for p in pairs], [p[1] for p in pairs]
    for same_octave in (False, True):
        got = run_dev(ctx, torch, qsets, tsets, cap, cap, same_octave=same_octave, match_cap=match_cap)
        totals = [len(check_pair(got, k, qsets[k], tsets[k], cap, cap, 0.64, same_octave, match_cap)[1]) for k in range(n)]
        assert min(totals) == 0 and max(totals) > match_cap  # require: empty lists and lists that are cut


# ---- B. hostile values

def near_copy(rng, t):
    """t * (1 + U(-1, 1) * 2^-20), formed in f64 and rounded to f32: d2 of the pair is below the rounding noise of its chains."""
    return (t.astype(np.float64) * (1.0 + rng.uniform(-1.0, 1.0, t.shape) * 2.0 ** -20)).astype(np.float32)


def block_mixed_signs(rng, nq, nt):
    t = matchref.crafted(rng, nt, signed=True)
    return matchref.crafted(rng, nq, t, signed=True), t


def block_near_copies(rng, nq, nt):
    t = matchref.reference_like_descriptors(rng, nt)
    return near_copy(rng, t[np.arange(nq) % nt]), np.concatenate([t, near_copy(rng, t)])  # two near copies of its row for every query


def block_subnormals(rng, nq, nt):
    def rows(n):
        d = matchref.reference_like_descriptors(rng, n)
        d[0::5] *= np.float32(1e-22)   # products of a few units of 2^-149: partial sums and norms are f32 subnormals
        d[1::5] *= np.float32(1e-23)   # products below half a unit of 2^-149: each one is absorbed by the fmaf, norm 0
        d[2::5] *= np.float32(1e-30)   # every product underflows: norm 0
        d[3::5] *= np.float32(1e-40)   # subnormal operands, norm 0
        d[4::10] = 0.0
        d[9::10] = -0.0
        return d
    return rows(nq), rows(nt)


def block_overflow(rng, nq, nt):
    def rows(n):
        d = matchref.crafted(rng, n, signed=True)   # mixed signs: s is small against the norms, d2 is about their sum
        d[0::4] *= np.float32(1e18)
        d[1::4] *= np.float32(1.5e18)
        d[2::4] = np.abs(d[2::4]) * np.float32(1e19)  # norm +inf; against each other s is +inf as well: inf - inf
        top = d[3::4].astype(np.float64)              # norm 2^127 up to rounding: n(a) + n(b) lies at the edge of the f32 range
        d[3::4] = (top * np.sqrt(2.0 ** 127 / (top * top).sum(axis=1))[:, None]).astype(np.float32)
        return d
    t = rows(nt)
    q = rows(nq)
    q[:8] = t[:8]
    # a near copy of a row at the top of the range: where the sum of the norms still rounds to a finite value and 2 s to +inf,
    # d2 is -inf, and it wins like any smaller value
    top = t[3::4]
    for n, i in enumerate(range(11, nq, 4)):
        for _ in range(40):  # about one near copy in ten gives -inf: draw until the restatement says so (an input choice)
            q[i] = near_copy(rng, top[n % len(top)])
            if np.isneginf(matchref.d2(q[i], top[n % len(top)])):
                break
    return q, t


def block_partial_specials(rng, nq, nt):
    def rows(n):
        d = matchref.crafted(rng, n, signed=True)
        k = rng.integers(0, 128, n)
        i = np.arange(n)
        d[i[0::4], k[0::4]] = np.inf
        d[i[1::4], k[1::4]] = -np.inf
        d[i[2::4], k[2::4]] = np.nan
        return d
    t = rows(nt)
    return np.concatenate([t[:8], rows(nq)[8:]]), t


BLOCKS = (block_mixed_signs, block_near_copies, block_subnormals, block_overflow, block_partial_specials)


def is_subnormal(x):
    return (x != 0.0) & (np.abs(x) < np.finfo(np.float32).tiny)


@pytest.mark.parametrize("nq,nt", [(300, 300), (129, 65), (64, 127)])
def test_b_hostile_values(env, nq, nt):
    ctx, torch = env
    rng = np.random.default_rng(3)
    benign_t = matchref.reference_like_descriptors(rng, nt)
    benign_q = crafted(rng, nq, base=benign_t)
    qsets, tsets, names = [], [], []
    for block in BLOCKS:
        q, t = block(rng, nq, nt)
        for role, (a, b) in (("itself", (q, t)), ("query", (q, benign_t)), ("train", (benign_q, t))):
            qsets.append((a, None, None, len(a))), tsets.append((b, None, None, len(b))), names.append((block.__name__, role))
    qcap, tcap = nq + 3, 2 * nt + 2
    got = run_dev(ctx, torch, qsets, tsets, qcap, tcap)
    want = {}
    for k, name in enumerate(names):
        wnn, wm = check_pair(got, k, qsets[k], tsets[k], qcap, tcap, 0.64, False, qcap)
        # the rule "a NaN distance never wins" in full: no field of the answer is NaN, so bytes-equality is well defined
        assert not np.isnan(wnn["dist2"]).any() and not np.isnan(wnn["second_dist2"]).any(), name
        assert ((wnn["index"] >= 0) == (wnn["dist2"] < np.inf)).all(), name   # +inf never wins; -inf (block_overflow) does
        want[name] = (wnn, wm, qsets[k][0], tsets[k][0])
    # require: each block shows what it is for
    wnn, _, q, t = want["block_near_copies", "itself"]
    neg = int((wnn["dist2"] < 0).sum()), int((wnn["second_dist2"] < 0).sum())
    print("near copies: negative dist2, negative second_dist2:", neg, "of", nq)
    if (nq, nt) == (300, 300):
        assert neg[0] >= 20 and neg[1] >= 5
    assert neg[0] >= 1
    wnn, _, q, t = want["block_subnormals", "itself"]
    sub = np.concatenate([wnn["dist2"][is_subnormal(wnn["dist2"])], wnn["second_dist2"][is_subnormal(wnn["second_dist2"])]])
    print("subnormals: subnormal distances in the answer:", len(sub), "smallest", sub.min() if len(sub) else None)
    assert len(sub) >= 1
    zero_norm_t = np.flatnonzero(matchref.norms(t) == 0.0)
    zero_norm_q = np.flatnonzero(matchref.norms(q) == 0.0)
    assert len(zero_norm_q) >= 4 and len(zero_norm_t) >= 4 and (np.signbit(t[zero_norm_t]).all(axis=1)).any()
    # rows of norm 0 - underflowed, subnormal, all zero, all -0.0 - tie at distance 0: the lowest index wins, second == best
    assert (wnn["index"][zero_norm_q] == zero_norm_t[0]).all() and (wnn["dist2"][zero_norm_q] == 0.0).all() and (wnn["second_dist2"][zero_norm_q] == 0.0).all()
    wnn, wm_over, q, t = want["block_overflow", "itself"]
    d2 = matchref.d2_all(q, t)
    chosen = np.zeros(d2.shape, bool)
    chosen[np.flatnonzero(wnn["index"] >= 0), wnn["index"][wnn["index"] >= 0]] = True
    print("overflow: finite d2 above 1e38:", int((np.isfinite(d2) & (d2 > 1e38)).sum()), "+inf:", int(np.isposinf(d2).sum()), "NaN:", int(np.isnan(d2).sum()),
          "chosen above 1e38:", int((chosen & (d2 > 1e38)).sum()))
    assert (np.isfinite(d2) & (d2 > 1e38)).any() and np.isposinf(d2).any() and np.isnan(d2).any()
    assert not chosen[np.isposinf(d2) | np.isnan(d2)].any()
    assert np.isnan(matchref.d2(q[2], t[2])) and np.isposinf(matchref.d2(q[2], t[0])) and wnn[2]["index"] == -1  # inf - inf, inf - finite: never chosen
    neginf = np.flatnonzero(np.isneginf(wnn["dist2"]))
    print("overflow: queries whose nearest distance is -inf:", len(neginf), "accepted among them:", int(np.isin(neginf, wm_over["query"]).sum()))
    # require: a -inf distance that wins and is accepted (sum of the norms finite, 2 s = +inf), from the rows at the top of the range
    assert len(neginf) >= 1 and np.isin(neginf, wm_over["query"]).any() and (neginf % 4 == 3).all()
    assert all(np.isneginf(matchref.d2(q[i], t[wnn[i]["index"]])) for i in neginf)
    assert np.isfinite(wnn["second_dist2"]).any() and (wnn["second_dist2"][np.isfinite(wnn["second_dist2"])] > 1e38).any()
    wnn, _, q, t = want["block_partial_specials", "itself"]
    special = ~np.isfinite(q).all(axis=1)
    assert special[:8:4].all() and (wnn["index"][special] == -1).all() and (wnn["index"][~special] >= 0).all()
    assert np.isfinite(t[wnn["index"][~special]]).all()  # a row with one Inf or NaN entry is never anyone's neighbour


# ---- C. the device against f64 arithmetic, no restatement in between

@pytest.mark.parametrize("signed", [False, True])
def test_c1_c2_device_nn_against_exact_arithmetic(env, signed):
    ctx, torch = env
    q, t, exact, bound = exact_sets(signed)
    nn, _, _ = run_dev(ctx, torch, [(q, None, None, len(q))], [(t, None, None, len(t))], len(q), len(t))
    nn = nn[0].copy().view(capi.NN2_DTYPE).reshape(-1)
    check_nn_against_exact(nn, exact, bound, "C1/C2 device, " + ("signed" if signed else "unsigned"))
