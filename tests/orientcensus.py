"""Coverage accounting for the batched filterKeypoints / SIFT kernels: block-noise frames whose coarse octaves carry
keypoints, and a census of what a frame's oracle lists put through each kernel form.

COVERAGE ACCOUNTING ONLY.  This module restates, in Python, how the host sizes the grids and how the kernels pick their
paths, so that a test can say "this frame sends N records through that path, T per workgroup".  It mirrors

  enqueue_orient_batch, enqueue_sift_batch, make_orient_plan   (visualslam_amd/csrc/vslam_hip.hip): workgroups per frame,
      which octave goes to k_orient_survivors_pk and which to k_orient_survivors, the LDS budget of an octave;
  k_orient_survivors_pk: geo_of                                 (kernels_orient_pk.hip.h): py0 / px0, interior, sh;
  k_orient_survivors: region / patch                            (kernels_orient_batch.hip.h): the three forms;
  k_edge_flags, k_survivor_ranges                               (kernels_orient_batch.hip.h): the shared flag word, the ranges;
  sift_one_keypoint                                             (kernels_sift.hip.h): the ext / kt filter forms.

It never decides an expected value: every value a GPU test compares comes from oracle.Pyramid.  If the kernels or the host
change their formulas this file goes stale and the floors of tests/test_orient_census_cpu.py describe the old dispatch; the
comparisons with the oracle stay valid either way."""
import numpy as np

import oracle
from visualslam_amd import synth

OR_WIN, OR_PAD = 16, 8   # kernels_orient.hip.h
OR_PK_MAX_SPAN = 60      # kernels_orient_pk.hip.h
BIG_LDS_FLOATS = 36 * 1024  # make_orient_plan: kBigLds
PK_MULT = 8              # enqueue_orient_batch: pk_mult; enqueue_sift_batch: 8 * gwg
SIFT_EXT_R = 47          # kernels_sift.hip.h


# ------------------------------------------------------------------------------------------------ content
def block_noise(rows, cols, block, frame=0, stream_id=0):
    """Uniform noise enlarged block-wise: np.kron(noise(rows / b, cols / b), ones((b, b))), cropped to rows x cols.  Integer-only
    and seeded through synth.frame_np(kind="noise"), like every synthetic frame here.  block = one block size, or a sequence
    of block sizes: horizontal bands of equal height, or of (block size, band height) pairs; the last band takes the
    remainder, band i is seeded with frame + i."""
    bands = [block] if np.isscalar(block) else list(block)
    bands = [b if isinstance(b, tuple) else (b, rows // len(bands)) for b in bands]
    out = np.empty((rows, cols), np.uint8)
    r1 = 0
    for i, (b, h) in enumerate(bands):
        r0 = r1
        r1 = rows if i == len(bands) - 1 else r0 + h
        small = synth.frame_np(-(-(r1 - r0) // b), -(-cols // b), frame + i, stream_id, "noise")
        out[r0:r1] = np.kron(small, np.ones((b, b), np.uint8))[: r1 - r0, :cols]
    return out


# ------------------------------------------------------------------------------------------------ the oracle's lists
def oracle_lists(img, n_oct, sigma0=1.6, window=3):
    """What the oracle says about one frame, octave by octave: localized keypoints (the batched path's dog_points with
    localize = 1), oriented points (filterKeypoints) and descriptors with their defined flags (SIFT)."""
    want = oracle.Pyramid(img, n_oct, sigma0)
    kps = [want.keypoints(o, window) for o in range(n_oct)]
    ori = [want.filter_keypoints(o, kps[o]) for o in range(n_oct)]
    dd = [want.sift_descriptors(o, ori[o]) for o in range(n_oct)]
    sizes = list(want.sizes)
    want.close()
    return dict(sizes=sizes, keypoints=kps, oriented=ori, descriptors=[d for d, _ in dd], defined=[k for _, k in dd], sigma0=sigma0)


# ------------------------------------------------------------------------------------------------ the host's plan, restated
def gwg(nf):
    return min(1024, max(16, 8192 // nf))


def tap_count(sigma0, o, l):
    return oracle.gauss_ksize_f32(1.5 * oracle.sigma_at(sigma0, o, l))


def span_of(kn):
    return OR_WIN + 2 * (kn // 2)


def _patch_floats(span):
    return (span + 2) * ((span + 8) >> 2)


def _region_floats(span):
    return 3 * span + span * OR_WIN + span * span


def octave_plan(sigma0, o):
    """(kernel, {level: form}) of octave o.  kernel: "pk" (k_orient_survivors_pk, one launch per level) or "surv"
    (k_orient_survivors, one launch for the octave).  form of a level under "surv": "patch" (interior survivors stage their u8
    patch in LDS), "region" (magnitude region in LDS, no patch) or "taps" (magnitudes tap by tap); under "pk" always "pk"."""
    spans = {l: span_of(tap_count(sigma0, o, l)) for l in (1, 2, 3)}
    if max(spans.values()) <= OR_PK_MAX_SPAN:
        return "pk", {l: "pk" for l in spans}
    worst = max(_region_floats(s) + _patch_floats(s) for s in spans.values())
    strip = max(s * (OR_WIN + 3) for s in spans.values())
    need = worst if worst <= BIG_LDS_FLOATS else max(strip, min(worst, BIG_LDS_FLOATS))
    forms = {}
    for l, s in spans.items():
        region = _region_floats(s) <= need
        forms[l] = "patch" if region and _region_floats(s) + _patch_floats(s) <= need else "region" if region else "taps"
    return "surv", forms


def _changes(cls, stride):
    """How many list neighbours one grid stride apart differ in class (= consecutive records of one workgroup)."""
    cls = np.asarray(cls)
    return int((cls[:-stride] != cls[stride:]).sum()) if len(cls) > stride else 0


def trips(n, workgroups):
    return -(-n // workgroups)


# ------------------------------------------------------------------------------------------------ the census
def census(lists, nf):
    """Per (octave, level), per octave and for the descriptor stage: how many records of this frame each kernel path sees in a
    chunk of nf frames, and how many records one workgroup walks.  lists = oracle_lists(...)."""
    sigma0, sizes = lists["sigma0"], lists["sizes"]
    n_oct = len(sizes)
    g = gwg(nf)
    levels, octaves = {}, {}
    surv_index = []  # list index (into the frame's keypoint list) of every survivor, in list order
    base = 0
    for o in range(n_oct):
        kp, ori = lists["keypoints"][o], lists["oriented"][o]
        rows, cols = sizes[o]
        keys = {(int(q["level"]), int(q["row"]), int(q["col"])) for q in ori}
        keep = np.array([(int(q["level"]), int(q["row"]), int(q["col"])) in keys for q in kp], bool)
        surv_index.extend((base + np.flatnonzero(keep)).tolist())
        base += len(kp)
        s = kp[keep]
        kernel, forms = octave_plan(sigma0, o)
        interior_all = np.zeros(len(s), bool)
        for l in (1, 2, 3):
            kn = tap_count(sigma0, o, l)
            R, span = kn // 2, span_of(kn)
            m = s["level"] == l
            y, x = s["row"][m].astype(np.int64), s["col"][m].astype(np.int64)
            py0, px0 = y - R - OR_PAD - 1, x - R - OR_PAD - 1
            interior = (py0 >= 0) & (px0 >= 0) & (py0 + span + 2 <= rows) & (px0 + span + 2 <= cols)
            if kernel == "surv" and forms[l] != "patch":
                interior[:] = False  # no patch at this level: every survivor takes the region / tap path
            interior_all[m] = interior
            wg = PK_MULT * g if kernel == "pk" else g
            levels[o, l] = dict(
                kernel=kernel, form=forms[l], kn=kn, span=span, survivors=int(m.sum()), workgroups=wg,
                trips=trips(int(m.sum()), wg) if kernel == "pk" else None,  # "surv" walks the octave, not the level
                interior=int(interior.sum()), border=int((~interior).sum()),
                sh=[int((interior & ((px0 & 3) == k)).sum()) for k in range(4)],
                interior_border_changes=_changes(interior, wg) if kernel == "pk" else None,
                oriented=int((ori["level"] == l).sum()),
                defined=int(lists["defined"][o][ori["level"] == l].sum()))
        octaves[o] = dict(kernel=kernel, survivors=len(s), workgroups=g if kernel == "surv" else None,
                          trips=trips(len(s), g) if kernel == "surv" else None,
                          interior_border_changes=_changes(interior_all, g) if kernel == "surv" else None,
                          form_changes=_changes([forms[int(l)] for l in s["level"]], g) if kernel == "surv" else None,
                          oriented=len(ori), defined=int(lists["defined"][o].sum()))
    # k_edge_flags: the early launch covers [0, obegin) (the list after octave 0), the late one the rest; they share one 64-bit word
    obegin = len(lists["keypoints"][0])
    w0 = (obegin >> 6) << 6
    si = np.array(surv_index, np.int64)
    flag_word = dict(obegin=obegin, below=int(((si >= w0) & (si < obegin)).sum()), above=int(((si >= obegin) & (si < w0 + 64)).sum()))
    # k_sift_descriptors_batch: the whole oriented list of the frame, 8 gwg workgroups
    ori = np.concatenate(lists["oriented"])
    defined = np.concatenate(lists["defined"]).astype(bool)
    kt = np.array([tap_count(sigma0, int(q["octave"]), int(q["level"])) // 2 > SIFT_EXT_R for q in ori], bool)
    wg = PK_MULT * g
    sift = dict(records=len(ori), workgroups=wg, trips=trips(len(ori), wg), defined=int(defined.sum()), kt=int(kt.sum()),
                kt_defined=int((kt & defined).sum()), defined_changes=_changes(defined, wg), form_changes=_changes(kt, wg),
                undefined_to_defined=int((~defined[:-wg] & defined[wg:]).sum()) if len(ori) > wg else 0)
    return dict(nf=nf, levels=levels, octaves=octaves, flag_word=flag_word, sift=sift,
                keypoints=int(base), survivors=len(surv_index), oriented=len(ori))


def report(name, c):
    """The census as text (printed by the CPU test, so the measured counts stand in its output)."""
    out = ["%s: nf = %d, %d keypoints, %d survivors, %d oriented; flag word at obegin = %d: %d below / %d above" %
           (name, c["nf"], c["keypoints"], c["survivors"], c["oriented"], c["flag_word"]["obegin"], c["flag_word"]["below"], c["flag_word"]["above"])]
    for (o, l), v in sorted(c["levels"].items()):
        out.append("  octave %d level %d  %-4s %-6s kn %3d span %3d  survivors %4d  trips %s  interior %4d (sh %s)  border %4d  int<->border %s  oriented %4d  defined %4d" %
                   (o, l, v["kernel"], v["form"], v["kn"], v["span"], v["survivors"], v["trips"], v["interior"], v["sh"], v["border"],
                    v["interior_border_changes"], v["oriented"], v["defined"]))
    for o, v in sorted(c["octaves"].items()):
        if v["kernel"] == "surv":
            out.append("  octave %d  k_orient_survivors: survivors %4d  trips %d at %d workgroups  int<->border %d  form changes %d" %
                       (o, v["survivors"], v["trips"], v["workgroups"], v["interior_border_changes"], v["form_changes"]))
    s = c["sift"]
    out.append("  sift: records %d  trips %d at %d workgroups  defined %d  kt %d (defined %d)  ext<->kt %d  undefined->defined %d  defined<->undefined %d" %
               (s["records"], s["trips"], s["workgroups"], s["defined"], s["kt"], s["kt_defined"], s["form_changes"], s["undefined_to_defined"], s["defined_changes"]))
    return "\n".join(out)


# ------------------------------------------------------------------------------------------------ the frames of the steady-state tests
# tests/test_gpu_orient_steady.py runs them inside 256-frame calls; tests/test_orient_census_cpu.py holds them to the
# coverage floors.  Sizes, layouts and seeds were chosen with report() so that the oracle meets every floor.
STEADY_NF = 256
PACKED_SHAPE = (400, 720)   # landscape: the rotated windows of the right-hand part of a frame leave the padded level (undefined)
COARSE_SHAPE = (640, 640)   # square: every descriptor is defined
_FINE, _MID, _BIG = [(4, 48), (64, 544), (4, 48)], [(4, 40), (16, 128), (32, 192), (64, 240), (4, 40)], [(4, 64), (16, 64), (48, 448), (4, 64)]


def steady_frame(name):
    """The content frames by name (every other frame of a call is synth's `constant`: empty lists)."""
    if name == "noise":       # uniform noise: hundreds of survivors at every level of octave 0, none above
        return synth.frame_np(*PACKED_SHAPE, kind="noise")
    if name == "block4":      # 4 x 4 blocks: ten times as many survivors at levels 2 and 3 as at level 1, and octave 1 populated
        return block_noise(*PACKED_SHAPE, 4)
    if name == "bands_4_64":  # fine bands at the top and bottom (the list on both sides of octave 0's end survives), 64-blocks between
        return block_noise(*COARSE_SHAPE, _FINE, stream_id=3)
    if name == "bands_4_16_32_64":
        return block_noise(*COARSE_SHAPE, _MID, stream_id=1)
    if name == "bands_4_16_48":
        return block_noise(*COARSE_SHAPE, _BIG, stream_id=1)
    raise ValueError(name)


PACKED_FRAMES = {0: "noise", 1: "block4"}  # position in the call -> frame
COARSE_FRAMES = {0: "bands_4_64", 128: "bands_4_16_32_64", 255: "bands_4_16_48"}
PACKED_CAPS = dict(dog_cap=12288, oriented_cap=9216)  # whole lists: block4 has 11.7 k keypoints, noise at sigma0 = 1.3 8.5 k oriented points
COARSE_CAPS = dict(dog_cap=12288, oriented_cap=8192)
