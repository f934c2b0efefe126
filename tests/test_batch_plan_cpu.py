"""The stream and event plan of one chunk of a batch call (csrc/vslam_batch_plan.h) without a GPU: on which lane the Harris
chain, the lattice scans, the second half's upsample and the orientation forks go, behind which event and after which octave.
tests/batch_plan_driver.cpp evaluates the header over every shape of the sweep - frame counts either side of the two
thresholds, every octave count, every tiled prefix, every flag combination the ABI admits - and this file checks the
invariants the enqueue code relies on (above all: no fork from one side stream to another while a capture is on, which only a
GPU run that dies of stack exhaustion would notice otherwise), compares every field with a restatement of the rules written
from the enqueue code before the plan existed, and pins named cases by hand."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "visualslam_amd", "csrc")
MAX_OCT = 16
MAIN, HARRIS_LANE, LIST_LANE, UP_LANE = 0, 1, 2, 3

(DOG, HARRIS, EXTREMA, LISTS, LOCALIZE, ORIENT, DENSE, WINDOW5, MX, BASES_SCRATCH, SIDE, CAPTURING, LATER, UP2_OK) = (1 << i for i in range(14))

REC = np.dtype([(n, "<i2") for n in ("nf", "n_oct", "n_tiled", "latv", "scnv")] + [("flags", "<u2")] +
               [(n, "<i2") for n in ("gate", "harris_lane", "harris_after", "scan_lane", "ev_oct", "up2_fused", "nf_a", "up_lane", "up_waits_chunk",
                                     "ev_chunk")] + [("fused", "<u2")] +
               [(n, "<i2") for n in ("sitemap", "wait_pack", "early_edge", "early_edge_forked", "spread")] + [("after_lo", "<u4"), ("after_hi", "<u4")])


def compile_driver(dest, *extra):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    return subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *extra, "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "batch_plan_driver.cpp"), "-o", str(dest)], capture_output=True, text=True)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = tmp_path_factory.mktemp("batch_plan") / "driver"
    r = compile_driver(path)
    assert r.returncode == 0, r.stderr
    return str(path)


@pytest.fixture(scope="module")
def sweep(exe):
    size = subprocess.run([exe, "recsize"], capture_output=True, text=True, timeout=60)
    assert size.returncode == 0 and int(size.stdout) == REC.itemsize
    out = subprocess.run([exe, "sweep"], capture_output=True, timeout=120)
    assert out.returncode == 0, out.stderr
    r = np.frombuffer(out.stdout, dtype=REC)
    r.flags.writeable = False
    return r


def after_of(r):
    """[records, MAX_OCT]: after[oo]."""
    both = r["after_lo"].astype(np.uint64) | (r["after_hi"].astype(np.uint64) << np.uint64(32))
    return np.stack([((both >> np.uint64(4 * o)) & np.uint64(15)).astype(np.int64) for o in range(MAX_OCT)], axis=1)


def admitted(f):
    if not f & DOG:
        return not f & (EXTREMA | LISTS | LOCALIZE | ORIENT | DENSE | WINDOW5 | MX | BASES_SCRATCH | UP2_OK)
    if f & LISTS and not f & EXTREMA:
        return False
    if f & DENSE and f & (WINDOW5 | LOCALIZE | ORIENT):
        return False
    if f & ORIENT and (not f & LOCALIZE or f & WINDOW5 or not f & LISTS):  # orient implies localize, window 3 and the lists
        return False
    return True


def test_the_plan_header_needs_no_hip():
    src = open(os.path.join(CSRC, "vslam_batch_plan.h")).read()
    assert "#include <hip" not in src and "hipStream_t" not in src and "hipEvent_t" not in src


def test_the_sweep_is_the_one_the_test_thinks_it_is(sweep):
    r = sweep
    assert sorted(set(r["nf"].tolist())) == [1, 31, 32, 63, 64, 65, 255, 256]
    flags = [f for f in range(1 << 14) if admitted(f)]
    assert sorted(set(r["flags"].tolist())) == flags and len(flags) == 2048 + 16
    dog = (r["flags"] & DOG) != 0
    assert sorted(set(r["n_oct"][dog].tolist())) == list(range(1, MAX_OCT + 1)) and (r["n_oct"][~dog] == 0).all()
    # a tiled prefix of 0, 1 or 2 octaves for every octave count that has room for it; three lattice / scan variants on the matrix path
    shapes = 2 + 3 * (MAX_OCT - 1)
    n_mx = sum(1 for f in flags if f & MX)
    assert len(r) == 8 * (16 + (len(flags) - 16 - n_mx) * shapes + n_mx * shapes * 3)
    assert set(zip(r["latv"].tolist(), r["scnv"].tolist())) == {(0, 0), (1, 1), (0, 2)}


def test_invariants_hold_for_every_swept_shape(sweep):
    r = sweep
    f = r["flags"].astype(np.int64)
    has = lambda bit: (f & bit) != 0
    n = np.where(has(DOG), r["n_oct"], 0).astype(np.int64)[:, None]
    oo = np.arange(MAX_OCT)[None, :]
    after = after_of(r)
    live = oo < n
    # every octave is scanned exactly once (the loop issues octave oo's scan while it is at octave after[oo], which must
    # exist), not before its own kernels, and in ascending order
    assert (after[live] >= np.broadcast_to(oo, after.shape)[live]).all()
    assert (after < np.maximum(n, 1))[live].all()
    assert ((after[:, 1:] >= after[:, :-1]) | ~live[:, 1:]).all()
    # the capture rule
    cap = has(CAPTURING)
    assert (r["early_edge_forked"][cap] == 0).all() and (r["spread"][cap] == 0).all()
    assert (r["early_edge_forked"] <= r["early_edge"]).all()
    # without side streams everything is on the main lane, unsplit, and no event of the side machinery is touched
    ns = ~has(SIDE)
    for lane in ("harris_lane", "scan_lane", "up_lane"):
        assert (r[lane][ns] == MAIN).all()
    assert (r["nf_a"][ns] == r["nf"][ns]).all()
    for ev in ("ev_chunk", "ev_oct", "wait_pack", "up_waits_chunk", "early_edge_forked", "spread"):
        assert (r[ev][ns] == 0).all(), ev
    assert (r["gate"][ns] == -1).all() and (r["harris_after"][ns] == -1).all()
    # the halves
    assert ((r["nf_a"] == r["nf"]) | (r["nf_a"] == r["nf"] // 2)).all() and (r["nf_a"] > 0).all()
    assert ((r["up_lane"] == UP_LANE) == (r["nf_a"] < r["nf"])).all()
    assert (r["up_waits_chunk"] <= (r["nf_a"] < r["nf"])).all()
    # what a later chunk owes the one before, only in a later chunk
    assert (r["wait_pack"] <= has(LATER)).all() and (r["up_waits_chunk"] <= has(LATER)).all()
    # the gate is a tiled octave, and the Harris chain never waits for an octave that does not exist
    assert (r["gate"] < np.maximum(r["n_tiled"], 0)).all() and (r["harris_after"] < n[:, 0]).all()
    # the site maps are asked for exactly when some shape with these flags fuses a scan
    any_fused = np.zeros(1 << 14, dtype=bool)
    np.logical_or.at(any_fused, f, r["fused"] != 0)
    assert (any_fused[f] == (r["sitemap"] != 0)).all()
    assert ((r["fused"].astype(np.int64) >> n[:, 0]) == 0).all()


def restated(r):
    """The rules as the enqueue code had them before the plan existed (vslam_detect_batch_dev, enqueue_dog, enqueue_octave_scan,
    enqueue_edge_flags_early, enqueue_orient_batch), over the sweep's inputs."""
    f = r["flags"].astype(np.int64)
    has = lambda bit: (f & bit) != 0
    nf, n_oct, n_tiled = (r[k].astype(np.int64) for k in ("nf", "n_oct", "n_tiled"))
    dog, side = has(DOG), has(SIDE)
    n_rec = len(r)
    oo = np.arange(MAX_OCT)[None, :]
    # dog_side_gate(plans, nf): the last Tile0 / Tile1 octave for nf >= 32, else -1
    side_gate = np.where(nf >= 32, np.minimum(n_tiled, n_oct) - 1, -1)
    w = {}
    # harris_gate = (dog && side_streams) ? dog_side_gate : -1; sh = side_streams ? aux[0] : stream
    w["harris_after"] = np.where(dog & side, side_gate, -1)
    w["harris_lane"] = np.where(side, HARRIS_LANE, MAIN)
    # enqueue_dog: gate = (side && p.localize) ? dog_side_gate : -1; octave o: `if (o < gate) continue;` then the scans of
    # oo = (o == gate ? 0 : o) .. o
    gate = np.where(side & has(LOCALIZE), side_gate, -1)[:, None]
    w["after"] = np.where(oo < (n_oct * dog)[:, None], np.where(oo <= gate, gate, oo), 0)
    w["scan_lane"] = np.where(side, LIST_LANE, MAIN)  # run.side = sx = side_streams ? aux[1] : nullptr
    w["ev_oct"] = side  # `if (side) hipEventRecord(ev_oct[o])`
    w["gate"] = np.where(side, side_gate, -1)  # both uses of dog_side_gate sit behind `side`
    # up2_fused = c->mx && bases_are_scratch && (geometry && mx_up2_supported); nf_a = (!up2_fused && side && up && nf >= 64) ? nf / 2 : nf
    up2 = has(MX) & has(BASES_SCRATCH) & has(UP2_OK)
    halves = ~up2 & side & (nf >= 64)
    w["up2_fused"] = up2
    w["nf_a"] = np.where(halves, nf // 2, nf)
    w["up_lane"] = np.where(halves, UP_LANE, MAIN)
    w["up_waits_chunk"] = halves & has(LATER)  # `if (nf_a < nf) { if (run.later_chunk) wait(up, ev_chunk)`
    w["ev_chunk"] = side  # `if (side && up) hipEventRecord(ev_chunk)`
    # fused[o] = c->mx && s.sitemap && do_extrema && !localize && !extrema_dense && window == 3 && lattice && mx_scan_supported
    lattice = (r["latv"][:, None] == 0) | (oo != (n_oct - 1)[:, None])
    scan_ok = (r["scnv"][:, None] == 0) | ((r["scnv"][:, None] == 1) & (oo < 2))
    mode = dog & has(MX) & has(EXTREMA) & ~has(LOCALIZE) & ~has(DENSE) & ~has(WINDOW5)
    fused = mode[:, None] & lattice & scan_ok & (oo < n_oct[:, None])
    w["fused"] = (fused * (1 << oo)).sum(axis=1)
    w["sitemap"] = mode
    # pack_pending: set by a fused scan on the side stream of the previous chunk of the same call, waited for by a later chunk
    w["wait_pack"] = has(LATER) & side & fused.any(axis=1)
    # after_list: `orient && o == 0 && L.n_octaves > 1`, forked to `(side_streams && !capturing) ? sh : nullptr`; the spread
    # launches with side_a, side_b = `(side_streams && !capturing) ? ... : nullptr`
    w["early_edge"] = dog & has(ORIENT) & (n_oct > 1)
    w["early_edge_forked"] = w["early_edge"] & side & ~has(CAPTURING)
    w["spread"] = dog & has(ORIENT) & side & ~has(CAPTURING)
    assert all(len(v) == n_rec for v in w.values())
    return w


def test_the_rules_match_the_restatement_over_the_whole_sweep(sweep):
    want = restated(sweep)
    got = {k: sweep[k].astype(np.int64) for k in want if k != "after"}
    got["after"] = after_of(sweep)
    for k, v in want.items():
        bad = np.nonzero((got[k] != v.astype(np.int64)).reshape(len(sweep), -1).any(axis=1))[0]
        assert len(bad) == 0, (k, len(bad), sweep[bad[0]], got[k][bad[0]], v[bad[0]])


BENCH = DOG | HARRIS | EXTREMA | LISTS | BASES_SCRATCH | SIDE | UP2_OK  # the benchmark's call: Harris and lists, side streams
NONE = dict(gate=-1, harris_lane=MAIN, harris_after=-1, scan_lane=MAIN, ev_oct=0, up2_fused=0, up_lane=MAIN, up_waits_chunk=0, ev_chunk=0, fused=0,
            sitemap=0, wait_pack=0, early_edge=0, early_edge_forked=0, spread=0)
SIDE_LANES = dict(NONE, harris_lane=HARRIS_LANE, scan_lane=LIST_LANE, ev_oct=1, ev_chunk=1)
# name: (nf, n_octaves, n_tiled, lattice variant, scan variant, flags), expected
NAMED = {
    "the benchmark's chunk": ((256, 4, 2, 0, 0, BENCH),
                              dict(SIDE_LANES, gate=1, harris_after=1, after="0,1,2,3", nf_a=128, up_lane=UP_LANE)),
    "... with localize": ((256, 4, 2, 0, 0, BENCH | LOCALIZE),
                          dict(SIDE_LANES, gate=1, harris_after=1, after="1,1,2,3", nf_a=128, up_lane=UP_LANE)),
    "... with orient": ((256, 4, 2, 0, 0, BENCH | LOCALIZE | ORIENT),
                        dict(SIDE_LANES, gate=1, harris_after=1, after="1,1,2,3", nf_a=128, up_lane=UP_LANE, early_edge=1, early_edge_forked=1, spread=1)),
    "... with orient, inside a capture": ((256, 4, 2, 0, 0, BENCH | LOCALIZE | ORIENT | CAPTURING),
                                          dict(SIDE_LANES, gate=1, harris_after=1, after="1,1,2,3", nf_a=128, up_lane=UP_LANE, early_edge=1)),
    "... on the matrix path, candidates mode, as a later chunk": (
        (256, 4, 2, 0, 1, BENCH | MX | LATER),
        dict(SIDE_LANES, gate=1, harris_after=1, after="0,1,2,3", up2_fused=1, nf_a=256, fused=0b11, sitemap=1, wait_pack=1)),
    "... as a later chunk": ((256, 4, 2, 0, 0, BENCH | LATER),
                             dict(SIDE_LANES, gate=1, harris_after=1, after="0,1,2,3", nf_a=128, up_lane=UP_LANE, up_waits_chunk=1)),
    "31 frames with everything on": ((31, 4, 2, 0, 0, BENCH | LOCALIZE | ORIENT),
                                     dict(SIDE_LANES, after="0,1,2,3", nf_a=31, early_edge=1, early_edge_forked=1, spread=1)),
    "a 4-frame later chunk": ((4, 3, 2, 0, 0, BENCH | LOCALIZE | ORIENT | LATER),
                              dict(SIDE_LANES, after="0,1,2", nf_a=4, early_edge=1, early_edge_forked=1, spread=1)),
    "the single-image pyramid build": ((1, 4, 2, 0, 0, DOG | UP2_OK), dict(NONE, after="0,1,2,3", nf_a=1)),
    "the watchdog's last step: no side streams": ((256, 4, 2, 0, 0, (BENCH | LOCALIZE | ORIENT | LATER) & ~SIDE),
                                                  dict(NONE, after="0,1,2,3", nf_a=256, early_edge=1)),
}


@pytest.mark.parametrize("name", list(NAMED))
def test_named_cases(exe, name):
    shape, want = NAMED[name]
    out = subprocess.run([exe, "case", *map(str, shape)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    got = dict(x.split("=", 1) for x in out.stdout.split())
    assert got == {k: str(v) for k, v in want.items()}


def test_the_sweep_is_clean_under_asan_and_ubsan(tmp_path):
    path = tmp_path / "driver_san"
    r = compile_driver(path, "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    if r.returncode != 0 and ("asan" in r.stderr or "sanitize" in r.stderr):
        pytest.skip("this compiler has no sanitizer runtime: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([str(path), "sweep"], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=300)
    assert out.returncode == 0 and out.stderr == "", out.stderr[-2000:]
