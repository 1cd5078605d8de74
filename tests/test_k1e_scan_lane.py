"""The reward scan's per-lane arithmetic on the CPU (csrc/cmdp_k1e.h: K1rLane, k1r_scan, exported as cmdp_k1e_scan_words):
the sum of one instance's code words against a plain loop that adds the rewards one by one in float64, in transition
order, compared with ==.  The statistics the export returns -- plain tiles advanced whole, tiles on the slow path, words
added step by step, rebases -- prove that every family of cases reaches every path."""
import ctypes as C

import numpy as np
import pytest

from colosseum_amd import _lib as L

K1R_T, K1R_D = 8, 3   # mirrors of cmdp_k1e.h
_TIE, _TIE8 = 2.0 ** -53, 0.75 + 2.0 ** -45   # the tie values of test_k1e_code_words.py
_SUBNORMAL = 5e-324
# name: (scaled reward of code 0, 1, 2 (, 3)), probability of each code
_SETS = {
    "three_values": ((0.0, 0.5, 1.0), (0.5, 0.3, 0.2)),
    "four_values": ((0.0, 0.5, 1.0, 0.25), (0.4, 0.2, 0.2, 0.2)),
    "minimum_not_zero": ((0.125, 0.5, 1.0), (0.5, 0.3, 0.2)),
    "tie_case": ((0.0, 0.5, _TIE, _TIE8), (0.4, 0.2, 0.2, 0.2)),
    "negative": ((0.0, -0.25, 1.0), (0.5, 0.2, 0.3)),
    "subnormal": ((0.0, 0.5, 1.0, _SUBNORMAL), (0.5, 0.3, 0.195, 0.005)),
    "deep_sea": ((0.0, 1.0 / 900.0, 1.0), (0.5, 0.499, 0.001)),
}
_STARTS = (0.0, 1.3125, float(np.nextafter(2.0, 0.0)))   # zero, inside a binade, one ulp below a power of two


def _words(codes, H, h0):
    """The code words of a segment whose transition t has reward code codes[t] and which starts h0 steps into an episode:
    ceil(H / 32) words per episode, the steps of an episode from field 0 of its first word on, unused fields zero."""
    n, nch = len(codes), (H + 31) // 32
    g = np.arange(n, dtype=np.int64) + h0
    e = g // H
    j = g % H - np.where(e == 0, h0, 0)
    words = np.zeros(int((h0 + n + H - 1) // H) * nch, np.uint64)
    np.add.at(words, e * nch + j // 32, np.asarray(codes, np.uint64) << (2 * (j % 32)).astype(np.uint64))
    return words, e * nch + j // 32


def _loop_sum(codes, rv, s0):
    s = float(s0)
    for v in np.asarray(rv, np.float64)[codes].tolist():
        s += v
    return s


def _scan(codes, H, h0, rv, s0):
    """cmdp_k1e_scan_words on the segment: (sum, stats)."""
    lib = L.load()
    words, _ = _words(codes, H, h0)
    r = np.zeros(4, np.float64)
    r[:len(rv)] = rv
    out, stats = C.c_double(), np.zeros(4, np.int32)
    rc = lib.cmdp_k1e_scan_words(words.ctypes.data, len(words), H, h0, len(codes), (H + 31) // 32, len(rv), r.ctypes.data, s0,
                                 C.byref(out), stats.ctypes.data)
    assert rc == 0, lib.cmdp_last_error()
    return out.value, stats


def _check(codes, H, h0, rv, s0, total):
    got, stats = _scan(codes, H, h0, rv, s0)
    want = _loop_sum(codes, rv, s0)
    assert got == want, (H, h0, len(codes), rv, s0, got, want, stats.tolist())
    total += stats
    return stats


def _steps_for(n_words, H, h0, rng):
    """a number of steps that fills n_words words from in-episode time h0 on and ends INSIDE an episode (when it can)"""
    nch = (H + 31) // 32
    E = max(1, n_words // nch)
    last = rng.randint(1, H) if H > 1 else 1   # steps into the last episode, 1 .. H - 1
    return max(1, (E - 1) * H + last - h0) if E > 1 else max(1, min(last, H - h0))


def _covered(total, negative=False):
    plain, slow, word, rebase = total.tolist()
    if negative:
        assert plain == 0 and slow >= 1 and word >= 1, total.tolist()   # a negative reward: no tile may advance in integers
    else:
        assert plain >= 1 and slow >= 1 and word >= 1 and rebase >= 1, total.tolist()


def test_scan_words_tile_boundaries():
    """word counts at the boundaries of a tile and of the three rolling tiles"""
    rng = np.random.RandomState(1)
    total = np.zeros(4, np.int64)
    rv, pr = _SETS["three_values"]
    for n_words in (1, 7, 8, 9, 15, 16, 17, 23, 24, 25, 200):
        for h0 in (0, 4):
            for s0 in _STARTS:
                n = _steps_for(n_words, 9, h0, rng)
                codes = rng.choice(len(rv), n, p=pr)
                assert len(_words(codes, 9, h0)[0]) == n_words
                _check(codes, 9, h0, rv, s0, total)
    _covered(total)


def test_scan_words_horizons():
    """H = 3, 9, 30, 32 (one word per episode) and 45 (two, the second partial); starts inside an episode, ends inside one"""
    rng = np.random.RandomState(2)
    total = np.zeros(4, np.int64)
    rv, pr = _SETS["four_values"]
    for H in (3, 9, 30, 32, 45):
        nch = (H + 31) // 32
        per_h = np.zeros(4, np.int64)
        for h0 in (0, H // 2, H - 1):
            for n_words in (26 * nch, 61 * nch):
                n = _steps_for(n_words, H, h0, rng)
                codes = rng.choice(len(rv), n, p=pr)
                assert (h0 + n) % H != 0 and len(_words(codes, H, h0)[0]) == n_words
                _check(codes, H, h0, rv, 0.0 if h0 else 1.3125, per_h)
        total += per_h
        if nch == 1:
            _covered(per_h)
        else:
            assert per_h[0] == 0 and per_h[1] >= 1 and per_h[2] >= 1   # chunked episodes have no plain tile
    _covered(total)


@pytest.mark.parametrize("name", list(_SETS))
def test_scan_words_reward_sets(name):
    rng = np.random.RandomState(3)
    total = np.zeros(4, np.int64)
    rv, pr = _SETS[name]
    for H, n_words in ((9, 200), (30, 120), (45, 60)):
        for h0 in (0, 5):
            for s0 in _STARTS:
                n = _steps_for(n_words, H, h0, rng)
                codes = rng.choice(len(rv), n, p=pr)
                _check(codes, H, h0, rv, s0, total)
    _covered(total, negative=name == "negative")


@pytest.mark.parametrize("target", (K1R_T, 2 * K1R_T - 1, 2 * K1R_T, 39))
def test_scan_words_crafted_crossing(target):
    """the sum reaches 1024 exactly at a step of word `target` of 40: word 0 and word 7 of the second tile, the word after
    (word 0 of the third), and the last word of the sequence"""
    rng = np.random.RandomState(4 + target)
    H, rv = 30, (0.0, 1.0, 0.25)
    codes = rng.choice(3, 40 * H, p=(0.5, 0.1, 0.4))
    words, word_of = _words(codes, H, 0)
    assert len(words) == 40
    t = int(np.flatnonzero((word_of == target) & (codes != 0))[3])   # a step of that word with a reward
    inc = np.asarray(rv)[codes]
    s0 = 1024.0 - float(inc[:t + 1].sum())   # (multiples of 1/4 below 2^10: exact)
    run = s0 + np.cumsum(inc)
    assert s0 >= 512.0 and run[t] == 1024.0 and run[t - 1] < 1024.0 and run[-1] < 2048.0
    assert word_of[int(np.flatnonzero(run >= 1024.0)[0])] == target
    total = np.zeros(4, np.int64)
    stats = _check(codes, H, 0, rv, s0, total)
    plain, slow, word, rebase = stats.tolist()
    # one crossing: one slow tile, one word step by step, one rebase.  Of the five tiles the first and the last are never
    # plain; the three between them are, but for the one with the crossing
    assert (slow, word, rebase) == (1, 1, 1) and plain == (3 if target == 39 else 2), stats.tolist()


def test_scan_words_random_sequences():
    """2 000 seeded random segments: horizon, start time, length, reward set and start sum drawn at random"""
    rng = np.random.RandomState(2026)
    total = np.zeros(4, np.int64)
    names = [n for n in _SETS if n != "negative"]
    horizons = (1, 2, 3, 5, 9, 17, 30, 31, 32, 33, 45, 64, 70)
    for _ in range(2000):
        H = horizons[rng.randint(len(horizons))]
        nch = (H + 31) // 32
        h0 = rng.randint(0, H)
        n_words = nch * rng.randint(1, 70)
        n = _steps_for(n_words, H, h0, rng)
        rv, pr = _SETS[names[rng.randint(len(names))]]
        codes = rng.choice(len(rv), n, p=pr)
        s0 = (0.0, 1.3125, float(np.nextafter(2.0, 0.0)), float(rng.uniform(0.0, 600.0)), 2.0 ** 40 + 0.5)[rng.randint(5)]
        _check(codes, H, h0, rv, s0, total)
    _covered(total)


def test_scan_words_rejects_a_wrong_word_count():
    lib = L.load()
    words, r = np.zeros(3, np.uint64), np.zeros(4, np.float64)
    out, stats = C.c_double(), np.zeros(4, np.int32)
    assert lib.cmdp_k1e_scan_words(words.ctypes.data, 3, 9, 0, 9 * 4, 1, 3, r.ctypes.data, 0.0, C.byref(out), stats.ctypes.data) == L.ERR_INVALID
    assert lib.cmdp_k1e_scan_words(words.ctypes.data, 3, 9, 9, 9 * 3, 1, 3, r.ctypes.data, 0.0, C.byref(out), stats.ctypes.data) == L.ERR_INVALID
