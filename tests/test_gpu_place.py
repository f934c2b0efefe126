"""Place recognition on the GPU (vslam_vocab_sample_dev, vslam_words_dev / _host, vslam_place_dev / _host; include/vslam.h):
every comparison is bytes-equal against the CPU restatement in tests/placeref.py, and sentinels stay intact past every count."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import matchref, placeref
from tests.test_gpu_match import detect, sets_to_device
from visualslam_amd import capi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -77
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def env():
    import torch

    capi.build()
    c = capi.Context(0, torch.cuda.current_stream().cuda_stream)
    yield c, torch
    c.close()


# ---- words

def run_words(ctx, torch, sets, cap, vocab, vdef, want=("words", "word_dist2", "hist"), with_defined=True):
    """sets: list of (desc [m, 128], defined [m] or None, count).  -> the wanted outputs as numpy, sentinel-filled before the call."""
    S, keep = sets_to_device(torch, [(d, df, None, cnt) for d, df, cnt in sets], cap, False)
    if not with_defined:
        S = capi.desc_sets(keep[0], keep[1])
    n, K = len(sets), len(vocab)
    tv = torch.from_numpy(np.ascontiguousarray(vocab, dtype=np.float32)).to(DEV)
    tvd = None if vdef is None else torch.from_numpy(np.ascontiguousarray(vdef, dtype=np.uint8)).to(DEV)
    outs = dict(words=torch.full((n, cap), SENT, dtype=torch.int32, device=DEV), word_dist2=torch.full((n, cap), SENT, dtype=torch.int32, device=DEV),
                hist=torch.full((n, K), SENT, dtype=torch.int32, device=DEV))
    ctx.words(S, tv, tvd, n, **{k: v for k, v in outs.items() if k in want})
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in outs.items()}


def want_words(sets, cap, vocab, vdef):
    n = len(sets)
    desc, counts = np.zeros((n, cap, 128), np.float32), np.zeros(n, np.int64)
    defined = np.ones((n, cap), np.uint8)
    for f, (d, df, cnt) in enumerate(sets):
        m = min(len(d), cap)
        desc[f, :m], counts[f] = d[:m], cnt
        if df is not None:
            defined[f, :m] = df[:m]
    return placeref.words(desc, counts, vocab, defined, vdef, fill=SENT), np.minimum(counts, cap)


def check_words(got, sets, cap, vocab, vdef, want=("words", "word_dist2", "hist")):
    (w, d, hist), used = want_words(sets, cap, vocab, vdef)
    for f, m in enumerate(used):
        if "words" in want:
            assert got["words"][f, :m].tobytes() == w[f, :m].tobytes(), ("words", f, int((got["words"][f, :m] != w[f, :m]).sum()), int(m))
            assert (got["words"][f, m:] == SENT).all(), "words past the count were written"
        if "word_dist2" in want:
            assert got["word_dist2"][f, :m].tobytes() == d[f, :m].tobytes(), ("word_dist2", f)
            assert (got["word_dist2"][f, m:] == SENT).all(), "word_dist2 past the count was written"
    if "hist" in want:
        assert got["hist"].tobytes() == hist.tobytes(), "hist"
    for k in ("words", "word_dist2", "hist"):
        if k not in want:
            assert (got[k] == SENT).all(), k + " was not asked for"
    return w, d, hist


def make_sets(rng, rows, vocab_src=None):
    out = []
    for m in rows:
        d = matchref.crafted(rng, m, vocab_src)
        out.append((d, None, m))
    return out


SEAM_ROWS = (0, 1, 31, 32, 33, 127, 128, 129, 257)


@pytest.mark.parametrize("K", [1, 63, 64, 65, 128, 1000])
def test_words_at_the_tile_seams(env, K):
    ctx, torch = env
    rng = np.random.default_rng(K)
    vocab = matchref.crafted(rng, K)
    sets = make_sets(rng, SEAM_ROWS, vocab)
    vdef = np.ones(K, np.uint8)
    w, d, hist = check_words(run_words(ctx, torch, sets, 260, vocab, vdef), sets, 260, vocab, vdef)
    assert hist.sum() == sum(SEAM_ROWS) and (w[8, :257] >= 0).all() and (d[8, :257] == 0).sum() > 30  # exact copies of words among the rows


def test_one_set_against_4096_words_with_ties_inside_a_tile_across_tiles_and_across_splits(env):
    ctx, torch = env
    rng = np.random.default_rng(4096)
    K, m = 4096, 300
    vocab = matchref.crafted(rng, K)
    (d, _, _), = make_sets(rng, [m], vocab)
    # 3 query tiles fill no chip: the 64 vocabulary tiles are dealt round robin to 16 workgroups per query tile (vslam_match_plan.h).
    # Words 5 == 6 (one tile), 70 == 200 == 1094 (tiles 1, 3 and 17: another workgroup, and tile 1's own workgroup again), 4095 == 64
    vocab[6], vocab[200], vocab[1094], vocab[4095] = vocab[5], vocab[70], vocab[70], vocab[64]
    d[0], d[1], d[2] = vocab[5], vocab[70], vocab[64]
    vdef = np.ones(K, np.uint8)
    vdef[[0, 63, 64, 127, 4095]] = 0  # undefined words at the ends of tiles; 64 is undefined, so its copy 4095 is too: row 2 finds neither
    d[3], d[4] = vocab[0], vocab[63]
    sets = [(d, None, m)]
    w, dist, hist = check_words(run_words(ctx, torch, sets, m, vocab, vdef), sets, m, vocab, vdef)
    assert (w[0, 0], w[0, 1]) == (5, 70) and dist[0, 0] == 0 and w[0, 2] not in (64, 4095) and w[0, 3] != 0 and w[0, 4] != 63
    assert hist[0, [0, 6, 63, 64, 127, 200, 1094, 4095]].sum() == 0


def test_forty_unequal_sets_and_a_count_above_cap(env):
    ctx, torch = env
    rng = np.random.default_rng(40)
    K, cap = 200, 150
    vocab = matchref.crafted(rng, K)
    rows = [int(v) for v in rng.integers(0, cap + 1, 40)]
    sets = make_sets(rng, rows, vocab)
    sets[7] = (matchref.crafted(rng, 400, vocab), None, 100000)  # more rows than the capacity, and a count above both
    sets[9] = (sets[9][0], (rng.random(len(sets[9][0])) < 0.7).astype(np.uint8), sets[9][2])
    got = run_words(ctx, torch, sets, cap, vocab, None)
    w, d, hist = check_words(got, sets, cap, vocab, None)
    assert hist[7].sum() == cap and (w[9, :rows[9]] == -1).sum() == (sets[9][1] == 0).sum()
    again = run_words(ctx, torch, sets, cap, vocab, None)  # two calls in a row: equal bytes
    assert all(got[k].tobytes() == again[k].tobytes() for k in got)


def hostile_rows(rng, n):
    d = matchref.crafted(rng, n, signed=True)
    f = np.finfo(np.float32)
    d[1] = np.nan                      # an all-NaN row, flagged defined: what real descriptors contain
    d[2, 17] = np.nan                  # one NaN entry poisons every distance of the row
    d[3, 5] = np.inf
    d[4, 9] = -np.inf
    d[5] = f.smallest_subnormal * np.arange(1, 129)  # subnormals: the chains are IEEE, no flush to zero
    d[6] = 0.0
    d[7] = -0.0
    d[8] = f.max / 4
    return d


def test_hostile_values_on_both_sides_and_undefined_everything(env):
    ctx, torch = env
    rng = np.random.default_rng(9)
    K, m = 130, 140
    vocab = hostile_rows(rng, K)
    d = hostile_rows(rng, m)
    d[20:60] = vocab[rng.integers(0, K, 40)]
    df = np.ones(m, np.uint8)
    df[[10, 21]] = 0
    vdef = np.ones(K, np.uint8)
    sets = [(d, df, m), (vocab.copy(), None, K)]
    w, dist, hist = check_words(run_words(ctx, torch, sets, m, vocab, vdef), sets, m, vocab, vdef)
    # the all-NaN row, flagged defined, gets -1 / +inf and counts nowhere; the NaN words are dead words
    assert w[0, 1] == -1 and np.isposinf(dist[0, 1]) and w[0, 2] == -1 and w[0, 10] == -1 and w[0, 21] == -1
    assert hist[:, [1, 2]].sum() == 0 and not np.isin(w[:, :], [1, 2]).any()
    assert hist[0].sum() == (w[0, :m] >= 0).sum() and w[1, 5] == 5 and w[1, 1] == -1
    # `defined` NULL on the sets: every row is
    got = run_words(ctx, torch, [(d, None, m)], m, vocab, vdef, with_defined=False)
    check_words(got, [(d, None, m)], m, vocab, vdef)
    # every word undefined: every row gets -1 and the histogram is zero
    none = np.zeros(K, np.uint8)
    got = run_words(ctx, torch, sets, m, vocab, none)
    w, dist, hist = check_words(got, sets, m, vocab, none)
    assert (w[0, :m] == -1).all() and np.isposinf(dist[0, :m]).all() and hist.sum() == 0 and (got["hist"] == 0).all()


def test_each_output_alone_the_host_twin_and_the_cxx_wrapper(env, tmp_path):
    ctx, torch = env
    rng = np.random.default_rng(17)
    K, cap = 90, 70
    rows = [70, 0, 33, 64]
    raw = [matchref.crafted(rng, m) for m in rows]
    defs = [(rng.random(m) < 0.8).astype(np.uint8) for m in rows]
    sets = [(d, df, m) for d, df, m in zip(raw, defs, rows)]
    desc, defined = np.zeros((4, cap, 128), np.float32), np.ones((4, cap), np.uint8)
    for f in range(4):
        desc[f, :rows[f]], defined[f, :rows[f]] = raw[f], defs[f]
    vocab, vdef = placeref.vocab_sample(desc, rows, K, defined)
    assert 0 < (vdef == 0).sum() < K
    for one in ("words", "word_dist2", "hist"):
        check_words(run_words(ctx, torch, sets, cap, vocab, vdef, want=(one,)), sets, cap, vocab, vdef, want=(one,))
    (w, d, hist), _ = want_words(sets, cap, vocab, vdef)
    hw, hd, hh = ctx.words_host(desc, rows, vocab, defined, vdef, fill=SENT)
    for f, m in enumerate(rows):
        assert hw[f, :m].tobytes() == w[f, :m].tobytes() and hd[f, :m].tobytes() == d[f, :m].tobytes()
        assert (hw[f, m:] == SENT).all() and np.isnan(hd[f, m:]).all()  # rows past the count keep the caller's bytes
    assert hh.tobytes() == hist.tobytes()
    only = ctx.words_host(desc, rows, vocab, defined, vdef, want_words=False, want_dist2=False)
    assert only[0] is None and only[1] is None and only[2].tobytes() == hist.tobytes()
    # vslam::sampleVocabulary + vslam::assignWords
    from tests.test_place_cpu import build_cxx_driver

    exe = build_cxx_driver(tmp_path)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(struct.pack("<3Q", 4, cap, K) + np.array(rows, np.uint32).tobytes() + desc.tobytes() + defined.tobytes())
    r = subprocess.run([exe, "words", str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    want = vocab.tobytes() + vdef.tobytes() + b"".join(w[f, :m].tobytes() + d[f, :m].tobytes() for f, m in enumerate(rows)) + hist.tobytes()
    assert dst.read_bytes() == want


def test_words_are_the_matchers_nearest_against_the_vocabulary(env):
    ctx, torch = env
    rng = np.random.default_rng(23)
    K, cap, n = 333, 200, 5
    vocab = matchref.crafted(rng, K)
    vdef = (rng.random(K) < 0.9).astype(np.uint8)
    rows = [200, 1, 129, 0, 77]
    sets = [(matchref.crafted(rng, m, vocab), (rng.random(m) < 0.9).astype(np.uint8), m) for m in rows]
    got = run_words(ctx, torch, sets, cap, vocab, vdef)
    Q, keepq = sets_to_device(torch, [(d, df, None, cnt) for d, df, cnt in sets], cap, False)
    T, keept = sets_to_device(torch, [(vocab, vdef, None, K)] * n, K, False)  # the vocabulary replicated as the train set of every pair
    nn = torch.full((n, cap, 3), SENT, dtype=torch.int32, device=DEV)
    ctx.match(Q, T, n, 0.64, False, nn=nn)
    torch.cuda.synchronize()
    nn = nn.cpu().numpy()
    for f, m in enumerate(rows):
        assert (nn[f, :m, 0] == got["words"][f, :m]).all() and nn[f, :m, 1].tobytes() == got["word_dist2"][f, :m].tobytes(), f


# ---- vocabulary

@pytest.mark.parametrize("n_sets,K", [(1, 1), (1, 300), (40, 7), (40, 40), (40, 1000)])
def test_vocabulary_is_the_rows_the_rule_names(env, n_sets, K):
    ctx, torch = env
    rng = np.random.default_rng(100 * n_sets + K)
    cap = 50
    rows = [int(v) for v in rng.integers(1, cap + 1, n_sets)]
    if n_sets > 1:
        rows[3], rows[5] = 0, 100000  # a set with no rows, a count above the capacity
    desc = rng.random((n_sets, cap, 128), dtype=np.float32)
    desc[0, 0] = np.nan  # a NaN row is copied like any other
    defined = (rng.random((n_sets, cap)) < 0.8).astype(np.uint8)
    t = [torch.from_numpy(a).to(DEV) for a in (desc, np.array(rows, np.int32), defined)]
    vocab = torch.full((K + 1, 128), SENT, dtype=torch.int32, device=DEV)
    vdef = torch.full((K + 3,), 9, dtype=torch.uint8, device=DEV)
    ctx.vocab_sample(capi.desc_sets(*t), vocab[:K].view(torch.float32), vdef[:K])
    torch.cuda.synchronize()
    wv, wd = placeref.vocab_sample(desc, rows, K, defined)
    assert vocab[:K].cpu().numpy().tobytes() == wv.tobytes() and vdef[:K].cpu().numpy().tobytes() == wd.tobytes()
    assert (vocab[K:] == SENT).all() and (vdef[K:] == 9).all()
    assert (wv[wd == 0] == 0).all() and not np.signbit(wv[wd == 0]).any()
    if n_sets > 1 and K > 5:
        assert wd[3] == 0 and 0 < wd.sum() < K
    ctx.vocab_sample(capi.desc_sets(t[0], t[1]), vocab[:K].view(torch.float32), vdef[:K])  # no `defined`: every row of a set with rows is
    torch.cuda.synchronize()
    wv, wd = placeref.vocab_sample(desc, rows, K, None)
    assert vocab[:K].cpu().numpy().tobytes() == wv.tobytes() and vdef[:K].cpu().numpy().tobytes() == wd.tobytes()


# ---- place

PLACE_OUTS = ("candidates", "cand_counts", "weights", "self_q", "self_db", "scores")


def run_place(ctx, torch, hist_q, hist_db=None, want=PLACE_OUTS, **kw):
    hq = torch.from_numpy(np.ascontiguousarray(hist_q).view(np.int32)).to(DEV)
    hd = None if hist_db is None else torch.from_numpy(np.ascontiguousarray(hist_db).view(np.int32)).to(DEV)
    nq, nd, K, c = len(hist_q), len(hist_q if hist_db is None else hist_db), hist_q.shape[1], kw.get("max_candidates", 3)
    shapes = dict(candidates=(nq, c, 3), cand_counts=(nq,), weights=(K,), self_q=(nq,), self_db=(nd,), scores=(nq, nd))
    outs = {k: torch.full(s, SENT, dtype=torch.int32, device=DEV) for k, s in shapes.items()}
    ctx.place(hq, hd, **kw, **{k: v for k, v in outs.items() if k in want})
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in outs.items()}


def check_place(got, hist_q, hist_db=None, want=PLACE_OUTS, **kw):
    ref = placeref.place(hist_q, hist_db, fill=SENT, **kw)
    for k in PLACE_OUTS:
        if k in want:
            assert got[k].tobytes() == ref[k].tobytes(), (k, got[k].reshape(-1)[:24], ref[k].reshape(-1)[:24])
        else:
            assert (got[k] == SENT).all(), k + " was not asked for"
    return ref


def random_hists(rng, n, K, fill=0.3, top=6):
    h = rng.integers(1, top, (n, K)).astype(np.uint32) * (rng.random((n, K)) < fill)
    return h.astype(np.uint32)


@pytest.mark.parametrize("nq,nd", [(1, 1), (2, 2), (15, 17), (16, 16), (17, 15), (40, 40)])
@pytest.mark.parametrize("K", [1, 100, 4096])
def test_place_sizes(env, nq, nd, K):
    ctx, torch = env
    rng = np.random.default_rng(1000 * nq + K)
    hd = random_hists(rng, nd, K, fill=0.3 if K > 1 else 0.8)
    hd[nd // 2] = 0  # an empty frame
    hq = random_hists(rng, nq, K)
    hq[: min(nq, nd)] = hd[: min(nq, nd)]  # the query frames are the db frames, where both exist: every score ties with its self-score
    for gap, c in ((0, 8), (1, 1), (3, 3)):
        kw = dict(q_first=5, db_first=5, min_gap=gap, max_candidates=c, num=1, den=8)
        check_place(run_place(ctx, torch, hq, hd, **kw), hq, hd, **kw)
    if nq == nd:  # one buffer searched in itself
        kw = dict(min_gap=2, max_candidates=8, num=0, den=1)
        check_place(run_place(ctx, torch, hd, None, **kw), hd, None, **kw)


@pytest.mark.parametrize("name", sorted(placeref.rule_cases()))
def test_place_rule_cases(env, name):
    ctx, torch = env
    kw = dict(placeref.rule_cases()[name])
    hq, hd = kw.pop("hist_q"), kw.pop("hist_db", None)
    ref = check_place(run_place(ctx, torch, hq, hd, **kw), hq, hd, **kw)
    without = run_place(ctx, torch, hq, hd, want=("candidates", "cand_counts"), **kw)  # no `scores`: tiles without an eligible pair are skipped
    assert without["candidates"].tobytes() == ref["candidates"].tobytes() and without["cand_counts"].tobytes() == ref["cand_counts"].tobytes()


def test_place_outputs_alone_the_host_twin_and_the_cxx_wrapper(env, tmp_path):
    ctx, torch = env
    rng = np.random.default_rng(77)
    K, nq, nd = 300, 37, 50
    hd, hq = random_hists(rng, nd, K), random_hists(rng, nq, K)
    hq[::3] = hd[5:5 + len(hq[::3])]
    kw = dict(q_first=6, db_first=0, min_gap=4, max_candidates=5, num=1, den=10, min_score=3)
    ref = check_place(run_place(ctx, torch, hq, hd, **kw), hq, hd, **kw)
    assert ref["cand_counts"].max() == 5 and ref["cand_counts"].min() < 5
    for one in ("cand_counts", "weights", "self_q", "self_db", "scores"):
        check_place(run_place(ctx, torch, hq, hd, want=(one,), **kw), hq, hd, want=(one,), **kw)
    got = run_place(ctx, torch, hq, hd, want=("candidates", "cand_counts"), **kw)  # `scores` absent: the same candidates
    check_place(got, hq, hd, want=("candidates", "cand_counts"), **kw)
    again = run_place(ctx, torch, hq, hd, **kw)
    assert all(again[k].tobytes() == ref[k].tobytes() for k in PLACE_OUTS)
    host = ctx.place_host(hq, hd, fill=SENT, **kw)
    assert all(host[k].tobytes() == ref[k].tobytes() for k in PLACE_OUTS)
    host = ctx.place_host(hd, None, min_gap=4, max_candidates=2, num=1, den=10, fill=SENT)
    own = placeref.place(hd, None, min_gap=4, max_candidates=2, num=1, den=10, fill=SENT)
    assert all(host[k].tobytes() == own[k].tobytes() for k in PLACE_OUTS)
    # vslam::findLoopCandidates
    from tests.test_place_cpu import build_cxx_driver

    exe = build_cxx_driver(tmp_path)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    P = capi.PlaceParams(kw["min_gap"], kw["max_candidates"], kw["num"], kw["den"], kw["min_score"], 0)
    src.write_bytes(struct.pack("<6Q", nq, nd, K, kw["q_first"], kw["db_first"], 0) + bytes(P) + hq.tobytes() + hd.tobytes())
    r = subprocess.run([exe, "place", str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    want = b"".join(struct.pack("<I", int(n)) + ref["candidates"][i, :n].tobytes() for i, n in enumerate(ref["cand_counts"]))
    assert dst.read_bytes() == want + ref["weights"].tobytes() + ref["self_q"].tobytes() + ref["self_db"].tobytes()


# ---- end to end

def test_seventeen_crops_on_the_device_and_the_place_executable(env, tmp_path):
    from tests.test_place_cpu import REVISITS, VOCAB_FRAMES, crop_sequence, expect_revisits

    ctx, torch = env
    crops = crop_sequence()
    # the home and blox images are smaller than some of their crops, so those frames are smaller: one batch call per frame size, each into its rows of the
    # sequence's descriptor buffers (copies on the device)
    n, K = len(crops), 256
    shapes = sorted({img.shape for img in crops})
    runs = [([f for f in range(n) if crops[f].shape == sh], sh) for sh in shapes]
    outs = [(idx, *detect(ctx, torch, np.stack([crops[f] for f in idx]))) for idx, _ in runs]
    cap = max(p.oriented_cap for _, p, _ in outs)
    d = torch.zeros((n, cap, 128), dtype=torch.float32, device=DEV)
    c = torch.zeros(n, dtype=torch.int32, device=DEV)
    df = torch.zeros((n, cap), dtype=torch.uint8, device=DEV)
    for idx, p, o in outs:
        at = torch.tensor(idx, device=DEV)
        d[at, : p.oriented_cap], c[at], df[at, : p.oriented_cap] = o["descriptors"], o["oriented_counts"], o["descriptor_defined"]
    assert int(c.max()) <= min(p.oriented_cap for _, p, _ in outs)
    S = capi.desc_sets(d, c, df)
    vocab = torch.full((K, 128), SENT, dtype=torch.int32, device=DEV).view(torch.float32)
    vdef = torch.full((K,), 9, dtype=torch.uint8, device=DEV)
    words = torch.full((n, cap), SENT, dtype=torch.int32, device=DEV)
    hist = torch.full((n, K), SENT, dtype=torch.int32, device=DEV)
    cands = torch.full((n, 3, 3), SENT, dtype=torch.int32, device=DEV)
    counts = torch.full((n,), SENT, dtype=torch.int32, device=DEV)
    V = VOCAB_FRAMES  # the vocabulary comes from the frames before the first revisit (tests/test_place_cpu.py)
    ctx.vocab_sample(capi.desc_sets(d[:V], c[:V], df[:V]), vocab, vdef)  # nothing comes down between the four calls
    ctx.words(S, vocab, vdef, words=words, hist=hist)
    ctx.place(hist, None, min_gap=4, max_candidates=3, num=1, den=5, candidates=cands, cand_counts=counts)
    torch.cuda.synchronize()
    hd, hc, hdf = d.cpu().numpy(), c.cpu().numpy(), df.cpu().numpy()
    assert (hc <= cap).all() and (hc[9:12] == 0).all() and (hc[:9] > 0).all()
    wv, wd = placeref.vocab_sample(hd[:V], hc[:V], K, hdf[:V])
    assert vocab.cpu().numpy().tobytes() == wv.tobytes() and vdef.cpu().numpy().tobytes() == wd.tobytes()
    ww, _, wh = placeref.words(hd, hc, wv, hdf, wd, fill=SENT)
    assert words.cpu().numpy().tobytes() == ww.tobytes() and hist.cpu().numpy().tobytes() == wh.tobytes()
    ref = placeref.place(wh, None, min_gap=4, max_candidates=3, num=1, den=5, fill=SENT)
    assert cands.cpu().numpy().tobytes() == ref["candidates"].tobytes() and counts.cpu().numpy().tobytes() == ref["cand_counts"].tobytes()
    # the executable on the same frames
    exe = os.path.join(ROOT, "visualslam_amd", "bin", "Place")
    assert os.path.exists(exe), "visualslam_amd/bin/Place is missing: __graft_entry__.build() builds it"
    paths = []
    for k, img in enumerate(crops):
        paths.append(str(tmp_path / f"crop{k:02d}.pgm"))
        with open(paths[-1], "wb") as f:
            f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]) + img.tobytes())
    r = subprocess.run([exe, "--words", "256", "--gap", "4", "--candidates", "3", "--threshold", "1/5", "--octaves", "3", "--vocab-frames", str(V)] + paths, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    assert rep["descriptors"] == [int(v) for v in hc] and rep["frames"] == n and rep["words"] == K
    assert [[c[0] for c in row] for row in rep["candidates"]] == [[int(c["frame"]) for c in ref["candidates"][i, : ref["cand_counts"][i]]] for i in range(n)]
    # the candidates, asserted as in tests/test_place_cpu.py (last: everything above is the device against the restatement)
    expect_revisits(ref)
    assert sorted(REVISITS) == [i for i in range(n) if rep["candidates"][i]]
