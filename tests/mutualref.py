"""CPU restatement of mutual matching (include/vslam.h, "mutual matching"), bit for bit, in two forms that a test can hold
against each other:

  mutual()    the matcher's restatement run both ways (tests/matchref.py): forward for nn and ACCEPTED, swapped for the reverse
              nearest - d2 is symmetric bit for bit, so nn[t].index / nn[t].dist2 of match(train, query) IS rnn[t] -, and the
              join MUTUAL = ACCEPTED and rnn[nn[q].index].index == q
  rnn_walk()  the header's reverse rule written as it stands: per train row a walk over the query rows, ascending, in a few lines
              of C of its own (NOT a swapped call)

and the ordered integer key of f32 the device takes its minimum over (key(), unkey()).
"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from tests import matchref
from visualslam_amd import capi

_SRC = r"""
#include <math.h>
#include <stddef.h>
#include <stdint.h>
typedef struct { int32_t index; float dist2; } rnn_t;
static float chain(const float* a, const float* b) {
    float acc = 0.0f;
    for (int k = 0; k < 128; ++k) acc = fmaf(a[k], b[k], acc);
    return acc;
}
/* train rows t0 .. t1-1, each against every query row, ascending */
void ref_rnn(const float* q, const uint8_t* qdef, const int32_t* qoct, size_t nq, const float* t, const uint8_t* tdef,
             const int32_t* toct, size_t t0, size_t t1, int same_octave, rnn_t* out) {
    for (size_t j = t0; j < t1; ++j) {
        float best = INFINITY;
        int32_t index = -1;
        if (!tdef || tdef[j]) {
            const float nt = chain(t + 128 * j, t + 128 * j);
            for (size_t i = 0; i < nq; ++i) {
                if (qdef && !qdef[i]) continue;
                if (same_octave && qoct[i] != toct[j]) continue;
                const float nqi = chain(q + 128 * i, q + 128 * i);
                const float sum = nqi + nt, twice = 2.0f * chain(q + 128 * i, t + 128 * j);
                const float d2 = sum - twice;
                if (d2 < best) { best = d2; index = (int32_t)i; }
            }
        }
        out[j].index = index; out[j].dist2 = best;
    }
}
"""

_lib = None


def lib():
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="mutualref_")
        src, so = os.path.join(d, "mutualref.c"), os.path.join(d, "mutualref.so")
        with open(src, "w") as f:
            f.write(_SRC)
        flags = ["-O2", "-ffp-contract=off", "-shared", "-fPIC"]
        try:
            if " fma " in open("/proc/cpuinfo").read().replace("\n", " "):
                flags.append("-mfma")
        except OSError:
            pass
        subprocess.run(["gcc", *flags, src, "-o", so, "-lm"], check=True, capture_output=True)
        _lib = C.CDLL(so)
    return _lib


def _rows(a):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 128)


def rnn_walk(q, t, same_octave=False, q_defined=None, t_defined=None, q_octave=None, t_octave=None):
    """-> rnn [nt] capi.RNN_DTYPE by the header's reverse rule, one walk over the query rows per train row."""
    from concurrent.futures import ThreadPoolExecutor

    q, t = _rows(q), _rows(t)
    nq, nt = len(q), len(t)
    opt = [None if a is None else np.ascontiguousarray(a, dtype=dt) for a, dt in
           ((q_defined, np.uint8), (q_octave, np.int32), (t_defined, np.uint8), (t_octave, np.int32))]
    ptr = [C.c_void_p(None if a is None else a.ctypes.data) for a in opt]
    if same_octave:
        assert opt[1] is not None and opt[3] is not None
    out = np.zeros(nt, capi.RNN_DTYPE)
    L = lib()

    def run(lo):
        L.ref_rnn(C.c_void_p(q.ctypes.data), ptr[0], ptr[1], C.c_size_t(nq), C.c_void_p(t.ctypes.data), ptr[2], ptr[3], C.c_size_t(lo),
                  C.c_size_t(min(lo + step, nt)), C.c_int(int(bool(same_octave))), C.c_void_p(out.ctypes.data))

    step = max(64, (nt + 15) // 16)
    with ThreadPoolExecutor(8) as ex:  # ctypes releases the GIL; the chunks write disjoint rows
        list(ex.map(run, range(0, nt, step)))
    return out


def rnn_swapped(q, t, same_octave=False, q_defined=None, t_defined=None, q_octave=None, t_octave=None):
    """-> rnn [nt] capi.RNN_DTYPE as (index, dist2) of the matcher's restatement with the sets swapped."""
    back = matchref.match(t, q, 0.64, same_octave, t_defined, q_defined, t_octave, q_octave)[0]
    out = np.zeros(len(back), capi.RNN_DTYPE)
    out["index"], out["dist2"] = back["index"], back["dist2"]
    return out


def join(fwd_matches, rnn):
    """The forward list's records whose train row chose the query back, order kept."""
    m = np.asarray(fwd_matches)
    return m[rnn["index"][m["train"]] == m["query"]] if len(m) else m.copy()


def mutual(q, t, ratio2=0.64, same_octave=False, q_defined=None, t_defined=None, q_octave=None, t_octave=None):
    """-> (nn [nq] capi.NN2_DTYPE, rnn [nt] capi.RNN_DTYPE, matches capi.MATCH_DTYPE: the mutual list, ascending query order)."""
    nn, fwd = matchref.match(q, t, ratio2, same_octave, q_defined, t_defined, q_octave, t_octave)
    rnn = rnn_swapped(q, t, same_octave, q_defined, t_defined, q_octave, t_octave)
    return nn, rnn, join(fwd, rnn)


def key(d2):
    """The ordered map of f32 (uint32 array): a < b as floats iff key(a) < key(b), NaN apart; + 0.0f folds -0 into +0."""
    u = (np.asarray(d2, np.float32) + np.float32(0.0)).view(np.uint32)
    return u ^ np.where(u >> 31, np.uint32(0xffffffff), np.uint32(0x80000000)).astype(np.uint32)


def unkey(k):
    """The way back: the f32 whose key is k."""
    k = np.asarray(k, np.uint32)
    return np.where(k >> 31, k ^ np.uint32(0x80000000), ~k).astype(np.uint32).view(np.float32)


def multiply_claimed(matches):
    """(train rows that appear in more than one record, the records that name one of them)."""
    t, n = np.unique(np.asarray(matches)["train"], return_counts=True)
    return int((n > 1).sum()), int(n[n > 1].sum())
