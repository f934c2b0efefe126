"""The difference form of the coarse octaves' horizontal pass without a GPU: the generated header is current and carries
the library's taps, the exactness bound holds where the form is chosen, and the form computed in f32 the way
k_gauss_h_diff computes it (a dense seed per 16-output segment, differences streamed column by column, prefix sum)
equals the integer dot form on random and extreme rows."""
import os
import re
import sys

import numpy as np
import pytest

from visualslam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_diff_taps  # noqa: E402

HBIAS = 128
HMAX = 255 * 256 + HBIAS
J = 16


def header_levels():
    """{(octave, level): (w, form, offsets, coefficients)} parsed from the header in the tree."""
    text = open(gen_diff_taps.HEADER).read()
    out = {}
    pat = (r"struct Lvl<(\d+), (\d+)> \{\s*static constexpr int n = (\d+), form = (\d), nd = (\d+);\s*"
           r"static constexpr uint16_t w\[n\] = \{([^}]*)\};\s*static constexpr int16_t de\[nd\] = \{([^}]*)\};\s*"
           r"static constexpr int16_t dc\[nd\] = \{([^}]*)\};")
    for m in re.finditer(pat, text):
        o, l, n, form, nd = (int(m.group(i)) for i in range(1, 6))
        w, de, dc = ([int(v) for v in m.group(i).split(",")] for i in (6, 7, 8))
        assert len(w) == n and len(de) == nd == len(dc)
        out[(o, l)] = (np.array(w, np.int64), form, de, dc)
    return out


def test_header_is_current():
    assert open(gen_diff_taps.HEADER).read() == gen_diff_taps.render(), "run python tools/gen_diff_taps.py"


def test_header_taps_are_the_librarys():
    lv = header_levels()
    assert sorted(lv) == [(o, l) for o in (1, 2, 3) for l in range(6)]
    for (o, l), (w, form, de, dc) in lv.items():
        s = capi.sigma_at(1.6, o, l)
        n = capi.gauss_ksize_u8(s)
        t = capi.gauss_taps_q8(n, s).astype(np.int64)
        z = (n - len(w)) // 2
        assert (t[:z] == 0).all() and (t[n - z:] == 0).all() and (t[z:n - z] == w).all(), (o, l)
        assert w.sum() == 256 and w[0] != 0
        r = len(w) // 2
        d = {e: int((w[e + r] if 0 <= e + r < len(w) else 0) - (w[e + r + 1] if e + r + 1 < len(w) else 0)) for e in range(-r - 1, r + 1)}
        assert {e: c for e, c in d.items() if c} == dict(zip(de, dc)), (o, l)


def test_exactness_bound_and_form_choice():
    lv = header_levels()
    for (o, l), (w, form, de, dc) in lv.items():
        if form == 1:
            assert sum(abs(c) for c in dc) * HMAX < 2 ** 24, (o, l)
            assert len(de) * 2.32 * 1.15 <= (len(w) + 1) / 2 * 4.27, (o, l)
    # the issue's table: octave 1 levels 0-2 stay dense, everything from octave 1 level 3 on takes the difference form
    assert [lv[(1, l)][1] for l in range(6)] == [0, 0, 0, 1, 1, 1]
    assert all(lv[(o, l)][1] == 1 for o in (2, 3) for l in range(6))


def test_form_is_refused_past_the_bound():
    f = gen_diff_taps.diff_form
    form, _, _ = f(np.array([0, 255, 0, 1, 0, 255, 0] * 9, np.uint16))  # sum |d| * 65408 far above 2^24
    assert form == 0
    with pytest.raises(ValueError):
        f(np.array([1, 2], np.uint16))  # even width


def simulate_diff(hrow_ext, w, de, dc, form, cols):
    """k_gauss_h_diff's arithmetic in f32 for one row: hrow_ext[x + off] = h[x] (reflect-101 extended, + HBIAS)."""
    n, r = len(w), len(w) // 2
    off = (len(hrow_ext) - cols) // 2
    ncs = (cols + J - 1) // J
    h = hrow_ext.astype(np.float32)
    x0 = np.arange(ncs) * J
    coef = dict(zip(de, dc)) if form == 1 else {e: int(w[e + r]) for e in range(-r, r + 1) if w[e + r]}
    lo = -r - 1 if form == 1 else -r
    acc = np.zeros((ncs, J), np.float32)
    seed = np.zeros(ncs, np.float32)
    for xr in range(lo, J + r):  # streamed in column order, as the kernel does
        hv = h[x0 + xr + off]
        if form == 1 and 0 <= xr + 1 + r < n and w[xr + 1 + r]:
            seed = np.float32(w[xr + 1 + r]) * hv + seed
        for j in range(J):
            c = coef.get(xr - j, 0)
            if c:
                acc[:, j] = np.float32(c) * hv + acc[:, j]
    if form == 1:
        acc[:, 0] += seed
        for j in range(1, J):
            acc[:, j] += acc[:, j - 1]
    assert (np.abs(acc) < 2 ** 24).all()
    return acc.reshape(-1)[:cols].astype(np.int64)


def reflect_ext(row, pad):
    idx = np.arange(-pad, len(row) + pad)
    n = len(row)
    while ((idx < 0) | (idx >= n)).any():
        idx = np.where(idx < 0, -idx, np.where(idx >= n, 2 * (n - 1) - idx, idx))
    return row[idx]


@pytest.mark.parametrize("kind", ["random", "max", "min", "alternating"])
def test_f32_difference_form_equals_integer_form(kind):
    rng = np.random.default_rng(7)
    for (o, l), (w, form, de, dc) in header_levels().items():
        n, r = len(w), len(w) // 2
        for cols in (961 // 2 ** (o - 1), 100, 37):
            if kind == "random":
                h = rng.integers(0, 255 * 256 + 1, cols)
            elif kind == "max":
                h = np.full(cols, 255 * 256)
            elif kind == "min":
                h = np.zeros(cols, np.int64)
            else:
                h = np.where(np.arange(cols) % 2 == 0, 255 * 256, 0)
            pad = r + J + 2
            hx = reflect_ext(h.astype(np.int64) + HBIAS, pad)
            dense = np.array([int((w * hx[x - r + pad: x + r + 1 + pad]).sum()) for x in range(cols)])
            got = simulate_diff(hx, w, de, dc, form, cols)
            assert (got == dense).all(), (o, l, cols, kind)
