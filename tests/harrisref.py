"""What the Harris strip-kernel tests share (tests/test_harris_launch_cpu.py, tests/test_gpu_harris_strip.py), numpy only:

- `segment_trips`: a RESTATEMENT of the trip loop of harris_strip_rows (csrc/kernels_harris_strip.hip.h) - t_begin, t_end,
  y_lo, y_hi, t_hi, its three loops with the peeled steady trip, and k_harris_strip's edge_strip.  It is written from the
  kernel's text and has to be kept equal to it by hand; the launch geometry itself (seg, nseg, grid) is NOT restated here,
  the CPU test takes it from csrc/vslam_harris_launch.h through tests/harris_launch_driver.cpp.
- `frame`: seeded content that decides every output of the kernel - 3x3 mask pixels, responses on both sides of 253.5 and
  of 2^31, exact zeros - with the low-amplitude classes laid across every strip and segment seam.
- `coverage`: what the oracle says such a frame exercises; the GPU cases assert it before they compare anything.
"""
import numpy as np

STRIP_W = 240  # HS_STRIP_W
TRIP = 6       # rows per trip of the kernel's outer loop
TWO31 = np.float32(2147483648.0)
KP_LO = np.float32(253.5)


# ---- restatement of the kernel's loop structure -------------------------------------------------------------------------
def edge_strip(strip, cols):
    """k_harris_strip: the strip touches the image's left / right border, margin lanes included."""
    return strip == 0 or (strip + 1) * STRIP_W + 8 > cols


def interior_strips(cols):
    return [s for s in range((cols + STRIP_W - 1) // STRIP_W) if not edge_strip(s, cols)]


def lane_dwords_inside(strip, cols):
    """Every lane's dword [x0, x0 + 4) of the strip lies inside a row of `cols` pixels (x0 = strip * 240 + 4 * (lane - 2))."""
    return all(0 <= strip * STRIP_W + 4 * (lane - 2) and strip * STRIP_W + 4 * (lane - 2) + 4 <= cols for lane in range(64))


def segment_trips(rows, y_begin, y_end, fast_ok):
    """The trips one wave runs for rows [y_begin, y_end) of a strip: [(steady, t0)].  `fast_ok`: the kernel's flag of that name
    (interior strip, aligned form, response + mask + flags wanted, no NMS2 map)."""
    t_begin, t_end = y_begin - 5, y_end + 3
    y_lo, y_hi = max(y_begin, 2), min(y_end, rows - 2)
    t_hi = min(y_hi - 1, rows - 7)
    out = []
    t0 = t_begin
    while t0 <= t_end and not (fast_ok and t0 - 4 >= y_lo and t0 < t_hi and t0 + 2 >= 0):
        out.append((False, t0))
        t0 += TRIP
    if fast_ok and t0 <= t_end and t0 < t_hi:  # the peeled steady trip
        out.append((True, t0))
        t0 += TRIP
    while fast_ok and t0 <= t_end and t0 < t_hi:
        out.append((True, t0))
        t0 += TRIP
    while t0 <= t_end:
        out.append((False, t0))
        t0 += TRIP
    return out


def trip_rows(steady, t0, y_begin, y_end):
    """Rows [lo, hi) a trip finalises (y = t - 4 for its six t): a steady trip all six, unconditionally; a generic one those of
    its segment."""
    return (t0 - 4, t0 + 2) if steady else (max(t0 - 4, y_begin), max(min(t0 + 2, y_end), max(t0 - 4, y_begin)))


def trip_prefetch(t0):
    """Rows [lo, hi) a steady trip loads without reflection: t + 2 for its six t."""
    return t0 + 2, t0 + 8


def check_segment(rows, y_begin, y_end):
    """The loop invariants for one segment, with and without the steady trips: every row of the segment finalised exactly once
    (in order, so: each trip's rows start where the last one's ended), steady trips finalise only rows of
    [max(y_begin, 2), min(y_end, rows - 2)) and prefetch only rows of [0, rows).  Returns the number of steady rows."""
    steady_rows = 0
    for fast_ok in (False, True):
        trips = segment_trips(rows, y_begin, y_end, fast_ok)
        nxt = y_begin
        for steady, t0 in trips:
            lo, hi = trip_rows(steady, t0, y_begin, y_end)
            if hi > lo:
                assert lo == nxt, (rows, y_begin, y_end, fast_ok, t0)
                nxt = hi
            if steady:
                assert fast_ok and hi - lo == TRIP
                assert max(y_begin, 2) <= lo and hi <= min(y_end, rows - 2), (rows, y_begin, y_end, t0)
                plo, phi = trip_prefetch(t0)
                assert 0 <= plo and phi <= rows, (rows, y_begin, y_end, t0)
                steady_rows += TRIP
        assert nxt == y_end, (rows, y_begin, y_end, fast_ok, trips)
        first, last = trips[0][1], trips[-1][1]  # six rows per trip from t_begin on, the last one reaching t_end
        assert first == y_begin - 5 and last == first + TRIP * (len(trips) - 1) and last <= y_end + 3 < last + TRIP
    return steady_rows


def segments(rows, seg):
    nseg = (rows + seg - 1) // seg  # as k_harris_strip computes it
    return [(s * seg, min(s * seg + seg, rows)) for s in range(nseg)]


# ---- content ------------------------------------------------------------------------------------------------------------
def _hash(seed, salt, idx):
    """splitmix64 of (seed, salt, idx): uint64 array like idx (integer only, the same on every numpy)."""
    with np.errstate(over="ignore"):
        z = (np.asarray(idx, np.uint64) + np.uint64(((seed * 0x632BE59BD9B4E019 + salt * 0xD1342543DE82EF95) & ((1 << 64) - 1)))) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


AMPLITUDE = (2, 6, 40)  # grey levels around MID of classes 0, 1, 2; class 3: random 0 / 255 blocks of 2 x 2
MID = 128
TILE = 4


def seam_rows(rows, seg):
    return [y for y in range(seg, rows, seg)]


def seam_cols(cols):
    return [x for x in range(STRIP_W, cols, STRIP_W)]


def frame(rows, cols, seed, seg):
    """uint8 [rows, cols]: TILE x TILE tiles of the four classes, classes 0 / 1 only in the tiles that reach into columns
    240k - 6 .. 240k + 5 or rows k * seg - 6 .. k * seg + 5 (a pixel changes the response up to 3 pixels away: blur, gradient,
    window) and in the image's outermost tiles, 2 x TILE there; then the dots of `stamps`."""
    r, c = np.arange(rows)[:, None], np.arange(cols)[None, :]
    tr, tc = r // TILE, c // TILE
    tiles_c = (cols + TILE - 1) // TILE
    tid = (tr * tiles_c + tc).astype(np.uint64)
    cls = (_hash(seed, 1, tid) & np.uint64(3)).astype(np.int64)
    low = np.zeros((rows, cols), bool)
    for x in seam_cols(cols):
        low |= (tc >= (x - 6) // TILE) & (tc <= (x + 5) // TILE)
    for y in seam_rows(rows, seg):
        low |= (tr >= (y - 6) // TILE) & (tr <= (y + 5) // TILE)
    low |= (tr == 0) | (tc == 0) | (tr == (rows - 1) // TILE) | (tc == (cols - 1) // TILE)
    fine = (_hash(seed, 4, ((r // 2) * tiles_c + tc).astype(np.uint64)) & np.uint64(1)).astype(np.int64)  # 2 x TILE there: both classes reach short seams
    cls = np.where(low, fine, cls)
    pid = (r * cols + c).astype(np.uint64)
    amp = np.choose(np.minimum(cls, 2), AMPLITUDE)
    noise = (_hash(seed, 2, pid) % (2 * amp + 1).astype(np.uint64)).astype(np.int64) - amp
    bid = ((r // 2) * ((cols + 1) // 2) + c // 2).astype(np.uint64)
    blocks = np.where(_hash(seed, 3, bid) & np.uint64(1), 255, 0)
    img = np.where(cls == 3, blocks, MID + noise)
    st = stamps(rows, cols, seed, seg)
    for y, x, _ in st:  # flat patches first, so that no patch erases another stamp's dot
        img[max(y - 4, 0): y + 5, max(x - 4, 0): x + 5] = MID
    for y, x, d in st:
        img[y, x] = MID + d
    for y, x in wrap_stamps(rows, cols, seed):
        img[max(y - 5, 0): y + 8, max(x - 5, 0): x + 11] = 255
        img[y: y + 3, x: x + 6] = 0
    return img.astype(np.uint8)


DOT_KP, DOT_MASK = 12, 8  # a dot of +12 on a flat patch is a keypoint (response about 400 .. 700), one of +8 a set mask pixel (about 120)


def wrap_stamps(rows, cols, seed):
    """[(row, col)] of the top left corners of 3 x 6 black blocks on white 13 x 16 patches, one per strip of 240 columns that has
    room for it.  Four pixels of the white rows next to the block's long sides (one column in from each end) have a response
    below 2^31 that saturates the 8-bit view and neighbours that are smaller or at or above 2^31: they are set in the 3 x 3 mask
    only because the view of those neighbours wraps to 0.  (Found by a search over small symmetric patterns: the random tiles
    have no such pixel, and without one a kernel that lost the wrap would pass.)"""
    out = []
    for s in range((cols + STRIP_W - 1) // STRIP_W):
        lo, hi = s * STRIP_W + 16, min((s + 1) * STRIP_W, cols) - 16 - 6
        if hi >= lo and rows >= 9:
            y = 3 + int(_hash(seed, 6, 2 * s) % np.uint64(rows - 8))
            out.append((y, lo + int(_hash(seed, 6, 2 * s + 1) % np.uint64(hi - lo + 1))))
    return out


def stamps(rows, cols, seed, seg):
    """[(row, col, dot)]: single-pixel dots on flat 9 x 9 patches, the placement that random tiles do not give on short seams - a
    keypoint dot and a mask dot at a seeded place within 2 of every strip seam and every segment seam, keypoint dots in rows 2 and
    rows - 3 and columns 2 and cols - 3, a mask dot in the right-edge lane's columns."""
    n = [0]

    def pick(lo, hi):  # seeded integer in [lo, hi]
        n[0] += 1
        return lo + int(_hash(seed, 5, n[0]) % np.uint64(max(hi - lo + 1, 1)))

    out = []
    kp_ok = rows >= 5 and cols >= 5
    for x in seam_cols(cols):
        half = pick(0, 1)
        if kp_ok and x - 2 <= cols - 3:
            out.append((pick(2, rows - 3) if half else pick(2, max(2, (rows - 3) // 2)), min(x - pick(0, 1), cols - 3), DOT_KP))
        out.append((pick(rows // 2, rows - 1) if not half else pick(0, max(0, rows // 2 - 1)), min(x + pick(-2, 1), cols - 1), DOT_MASK))
    for y in seam_rows(rows, seg):
        if kp_ok and 2 <= y - 1 and y - 2 <= rows - 3:
            out.append((min(y - pick(0, 1), rows - 3), pick(2, max(2, cols // 2 - 1)), DOT_KP))
        out.append((min(y + pick(-2, 1), rows - 1), pick(cols // 2, cols - 1), DOT_MASK))
    if kp_ok:
        out += [(2, pick(2, cols - 3), DOT_KP), (rows - 3, pick(2, cols - 3), DOT_KP), (pick(2, rows - 3), 2, DOT_KP), (pick(2, rows - 3), cols - 3, DOT_KP)]
    if cols % 4:
        out.append((pick(0, rows - 1), pick(cols - cols % 4, cols - 1), DOT_MASK))
    return out


# ---- what a frame exercises, by the oracle alone ---------------------------------------------------------------------------
def near(n, seams):
    """bool [n]: within 2 of a seam at s, i.e. s - 2 .. s + 1."""
    m = np.zeros(n, bool)
    for s in seams:
        m[max(s - 2, 0): s + 2] = True
    return m


class Ref:
    """The oracle's outputs of one frame (computed once per frame and shared by every output set that runs it)."""

    def __init__(self, img, k=0.04):
        import oracle

        self.img = img
        self.R = oracle.harris_response(img, k)
        self.mask = oracle.nms_strict(oracle.convert_scale_abs(self.R), 3)
        self.nms2 = oracle.nms2(self.R, 5)[0]
        self.kps = oracle.harris_keypoints(self.nms2)
        # set mask pixels that would not be set if responses >= 2^31 read 255 in the 8-bit view instead of wrapping to 0
        view = oracle.convert_scale_abs(self.R)
        view[self.R >= TWO31] = 255
        self.wrap_decided = (self.mask != 0) & (oracle.nms_strict(view, 3) == 0)


def steady_rows_of(rows, seg):
    """Rows the steady trips finalise on an interior strip of an aligned frame (output set response + mask + list)."""
    return [y for y0, y1 in segments(rows, seg) for steady, t0 in segment_trips(rows, y0, y1, True) if steady for y in range(t0 - 4, t0 + 2)]


def coverage(ref, seg, steady_rows=()):
    """{condition: holds} for one frame; every value must be True before the frame is worth comparing, except those whose name
    starts with '?': content that only some cases have, which the cases named for it assert.  `steady_rows`: steady_rows_of() where
    the case runs steady trips."""
    rows, cols = ref.img.shape
    R, mask, n2 = ref.R, ref.mask != 0, ref.nms2
    kp = np.zeros((rows, cols), bool)
    kp[ref.kps["row"], ref.kps["col"]] = True
    got = {}
    for x in seam_cols(cols):
        band = near(cols, [x])
        got[f"mask pixel at strip seam {x}"] = mask[:, band].any()
        if x - 2 < cols - 2:  # a keypoint column exists in the band (NMS2 runs on columns [2, cols - 2))
            got[f"keypoint at strip seam {x}"] = kp[:, band].any()
    if cols % 4:  # the right-edge lane's columns
        got["mask pixel in the right-edge lane"] = mask[:, cols - cols % 4:].any()
    for y in seam_rows(rows, seg):
        band = near(rows, [y])
        got[f"mask pixel at segment seam {y}"] = mask[band].any()
        if y - 2 < rows - 2 and y + 2 > 2:
            got[f"keypoint at segment seam {y}"] = kp[band].any()
    for s in interior_strips(cols):
        got[f"response >= 2^31 in interior strip {s}"] = (R[:, s * STRIP_W: (s + 1) * STRIP_W] >= TWO31).any()
        got[f"mask pixel decided by the 2^31 wrap in interior strip {s}"] = ref.wrap_decided[:, s * STRIP_W: (s + 1) * STRIP_W].any()
    if rows >= 9 and cols >= 38:
        got["mask pixel decided by the 2^31 wrap"] = ref.wrap_decided.any()
    if steady_rows:
        inner = np.zeros(cols, bool)
        for s in interior_strips(cols):
            inner[s * STRIP_W: (s + 1) * STRIP_W] = True
        st = np.zeros(rows, bool)
        st[list(steady_rows)] = True
        got["mask pixel in a steady row of an interior strip"] = mask[st][:, inner].any()
        got["keypoint in a steady row of an interior strip"] = kp[st][:, inner].any()
        got["response >= 2^31 in a steady row of an interior strip"] = (R[st][:, inner] >= TWO31).any()
    if rows >= 5 and cols >= 5:
        surv = n2[n2 > 0]
        got["NMS2 survivor below 253.5"] = (surv < KP_LO).any()
        got["NMS2 survivor in [253.5, 2^31)"] = ((surv >= KP_LO) & (surv < TWO31)).any()
        got["NMS2 survivor at or above 2^31"] = (surv >= TWO31).any()
        got["keypoint in row 2"] = kp[2].any()
        got["keypoint in row rows-3"] = kp[rows - 3].any()
        got["keypoint in column 2"] = kp[:, 2].any()
        got["keypoint in column cols-3"] = kp[:, cols - 3].any()
        got["?NMS2 survivor in [253.5, 254.5)"] = ((surv >= KP_LO) & (surv < KP_LO + 1)).any()
        # the window of column 1 (columns -1 .. 2) has a maximum in column 1: only the column range [2, cols - 2) keeps it out
        got["?NMS2 maximum in column 1"] = any(R[y, 1] > 0 and R[y, 1] >= R[y - 2: y + 2, 0: 3].max() for y in range(2, rows - 2))
    return {k: bool(v) for k, v in got.items()}
