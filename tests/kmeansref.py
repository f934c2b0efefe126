"""CPU restatement of the vocabulary training section of include/vslam.h, written from the header text and not from the kernels.

The assignment is placeref.words (the Words rule, untouched).  The ordered sum is Python floats - IEEE f64, every addition
rounded on its own - in the order the header states: blocks of 256 members from +0.0 in member order, then the blocks in
ascending order.  The mean is one Python division rounded once through numpy.float32.
"""
import numpy as np

from tests import placeref
from visualslam_amd import capi

BLOCK = 256


def members(words, counts):
    """words [n_sets, cap] -> {k: [(f, q), ...]} in member order: set ascending, then row ascending."""
    out = {}
    for f in range(words.shape[0]):
        for q in range(min(int(counts[f]), words.shape[1])):
            k = int(words[f, q])
            if k >= 0:
                out.setdefault(k, []).append((f, q))
    return out


def ordered_sum(rows):
    """rows: the member rows in member order, each a list of 128 Python floats -> the 128 sums of the header's step 4."""
    total = None
    for b in range(0, len(rows), BLOCK):
        B = [0.0] * 128
        for x in rows[b:b + BLOCK]:
            B = [s + v for s, v in zip(B, x)]
        total = B if total is None else [s + v for s, v in zip(total, B)]
    return total


def mean_word(rows):
    """-> the 128 f32 of step 5 for a word with these members (at least one)."""
    n = float(len(rows))
    with np.errstate(all="ignore"):
        return np.array([np.float32(np.float64(s) / np.float64(n)) for s in ordered_sum(rows)], np.float32)


def kmeans(desc, counts, vocab, rounds, defined=None, vocab_defined=None, history=False):
    """desc [n_sets, cap, 128] f32, counts [n_sets], vocab [K, 128] -> dict(vocab [K, 128] f32, sizes [K] u32, report [rounds]
    KMEANS_ROUND_DTYPE); with history also words (the assignment of every round that ran) and vocabs (V_0 and V_t of every round
    that updated)."""
    desc = np.ascontiguousarray(desc, dtype=np.float32)
    V = np.array(vocab, dtype=np.float32).reshape(-1, 128)
    n_sets, cap, K = desc.shape[0], desc.shape[1], len(V)
    report = np.zeros(rounds, capi.KMEANS_ROUND_DTYPE)
    sizes = np.zeros(K, np.uint32)
    used = [min(int(c), cap) for c in counts]
    hw, hv = [], [V.copy()]
    prev = None
    for t in range(rounds if n_sets else 0):
        w, _, _ = placeref.words(desc, counts, V, defined, vocab_defined)
        mem = members(w, counts)
        assigned = sum(len(m) for m in mem.values())
        if prev is None:
            changed = sum(used)
        else:
            changed = sum(int((w[f, :used[f]] != prev[f, :used[f]]).sum()) for f in range(n_sets))
        empty = sum(1 for k in range(K) if (vocab_defined is None or vocab_defined[k]) and k not in mem)
        report[t] = (assigned, changed, empty, 1)
        hw.append(w)
        if prev is not None and changed == 0:
            break
        new = V.copy()  # a word without members keeps its bytes
        sizes[:] = 0
        for k, m in mem.items():
            new[k] = mean_word([desc[f, q].tolist() for f, q in m])
            sizes[k] = len(m)
        V, prev = new, w
        hv.append(V.copy())
    out = dict(vocab=V, sizes=sizes, report=report)
    if history:
        out.update(words=hw, vocabs=hv)
    return out
