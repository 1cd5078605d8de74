"""The SINGLE-VALUE path of the reward scan's lane code on the CPU (csrc/cmdp_k1e.h: k1r_single, reached through
cmdp_k1e_scan_words_ex): a tile whose whole integer advance fails and in which at most one code present has a nonzero reward
is resolved from its step counts alone -- no code word is searched.  Every sum is compared with == against a plain loop that
adds the rewards one by one in float64, in transition order; the counters of the export (tiles resolved on the path, crossing
additions, additions of its float64 loop) prove that the path was taken, and that it was NOT where it must not be.  Every
scan also goes through cmdp_k1e_scan_words: its four counters are the first four of the new export."""
import ctypes as C

import numpy as np
import pytest

from colosseum_amd import _lib as L

K1R_T = 8   # mirror of cmdp_k1e.h
_V = 1.0 / 900.0
PLAIN, SLOW, WORD, REBASE, SINGLE, CROSS, FADD, RESERVED = range(8)
# name: (scaled reward of each code, probability of each code): ONE nonzero value among the codes that occur
_SETS = {
    "two_codes": ((0.0, _V), (0.5, 0.5)),
    "third_code_absent": ((0.0, _V, 1.0), (0.5, 0.5, 0.0)),
    "one_code": ((0.125,), (1.0,)),                                   # n_codes = 1: the active code is code 0
    "four_codes": ((0.0, 0.0, 0.0, _V), (0.25, 0.25, 0.25, 0.25)),    # the four-code count path
}
_STARTS = (0.0, 1.3125, float(np.nextafter(2.0, 0.0)), 2.0 ** 40 + 0.5)


def _words(codes, H, h0):
    """The code words of a segment whose transition t has reward code codes[t] and which starts h0 steps into an episode:
    ceil(H / 32) words per episode, the steps of an episode from field 0 of its first word on, unused fields zero."""
    n, nch = len(codes), (H + 31) // 32
    g = np.arange(n, dtype=np.int64) + h0
    e = g // H
    j = g % H - np.where(e == 0, h0, 0)
    words = np.zeros(int((h0 + n + H - 1) // H) * nch, np.uint64)
    np.add.at(words, e * nch + j // 32, np.asarray(codes, np.uint64) << (2 * (j % 32)).astype(np.uint64))
    return words


def _loop_sum(codes, rv, s0):
    s = float(s0)
    for v in np.asarray(rv, np.float64)[codes].tolist():
        s += v
    return s


def _scan(codes, H, h0, rv, s0):
    """Both exports on the segment: (sum, the eight counters); the old export gives the same sum and the first four."""
    lib = L.load()
    codes = np.asarray(codes, np.int64)
    words = _words(codes, H, h0)
    r = np.zeros(4, np.float64)
    r[:len(rv)] = rv
    args = (words.ctypes.data, len(words), H, h0, len(codes), (H + 31) // 32, len(rv), r.ctypes.data, float(s0))
    out, stats = C.c_double(), np.full(8, -1, np.int32)
    assert lib.cmdp_k1e_scan_words_ex(*args, C.byref(out), stats.ctypes.data) == 0, lib.cmdp_last_error()
    out4, stats4 = C.c_double(), np.full(4, -1, np.int32)
    assert lib.cmdp_k1e_scan_words(*args, C.byref(out4), stats4.ctypes.data) == 0, lib.cmdp_last_error()
    assert stats4.tolist() == stats[:4].tolist() and stats[RESERVED] == 0, (stats4.tolist(), stats.tolist())
    assert out4.value == out.value or (out4.value != out4.value and out.value != out.value)
    return out.value, stats


def _check(codes, H, h0, rv, s0, total=None):
    got, stats = _scan(codes, H, h0, rv, s0)
    want = _loop_sum(np.asarray(codes, np.int64), rv, s0)
    assert got == want, (H, h0, len(codes), rv, s0, got, want, stats.tolist())
    if total is not None:
        total += stats
    return stats


def _steps_for(n_words, H, h0, rng):
    """a number of steps that fills n_words words from in-episode time h0 on and ends INSIDE an episode (when it can)"""
    nch = (H + 31) // 32
    E = max(1, n_words // nch)
    last = rng.randint(1, H) if H > 1 else 1   # steps into the last episode, 1 .. H - 1
    return max(1, (E - 1) * H + last - h0) if E > 1 else max(1, min(last, H - h0))


def _only_single(stats):
    """with one nonzero value and no negative one EVERY tile that fails its advance is eligible: no word is ever searched"""
    assert stats[WORD] == 0 and stats[SLOW] == stats[SINGLE], stats.tolist()


@pytest.mark.parametrize("name", list(_SETS))
def test_single_value_sets_horizons_and_word_counts(name):
    """H = 1 .. 32: one word per episode, plain tiles (the plain entry); 45, 64, 70: chunked episodes, no plain tile (the
    non-plain entry).  Starts at h0 = 0 and inside an episode; segments end inside an episode when H > 1."""
    rng = np.random.RandomState(11)
    rv, pr = _SETS[name]
    total = np.zeros(8, np.int64)
    for H in (1, 2, 9, 30, 32, 45, 64, 70):
        nch = (H + 31) // 32
        per_h = np.zeros(8, np.int64)
        for h0 in sorted({0, H // 2}):
            for n_words in ((1, 7, 8, 9, 24, 25, 200) if nch == 1 else (nch, 4 * nch, 13 * nch, 40 * nch)):
                for s0 in _STARTS:
                    n = _steps_for(n_words, H, h0, rng)
                    codes = rng.choice(len(rv), n, p=pr)
                    assert len(_words(codes, H, h0)) == n_words
                    _only_single(_check(codes, H, h0, rv, s0, per_h))
        if nch > 1:
            assert per_h[PLAIN] == 0   # chunked episodes have no plain tile: these single-value tiles entered from the other branch
        assert per_h[SINGLE] >= 1 and per_h[FADD] >= 1, (H, per_h.tolist())   # (s0 = 0.0: the float64 loop of the first tile)
        total += per_h
    assert total[PLAIN] >= 1 and total[CROSS] >= 1 and total[REBASE] >= total[CROSS], total.tolist()


def _one_tile(na, v_code=1):
    """256 steps of H = 32 (eight words): `na` steps of the active code spread over the tile, the rest code 0"""
    codes = np.zeros(256, np.int64)
    codes[np.linspace(0, 255, na).astype(np.int64) if na > 1 else [131]] = v_code
    assert int((codes == v_code).sum()) == na
    return codes


def _cross_index(s0, v, na, limit):
    """the addition (1-based) at which s0 + v + v + ... first reaches `limit`; na + 1: none of the na"""
    s = float(s0)
    for i in range(1, na + 1):
        s += v
        if s >= limit:
            return i
    return na + 1


def _start_crossing_at(c, v, na, limit=1024.0):
    """a start sum below `limit` from which addition c (1 <= c <= na + 1) is the first to reach it: a backward search --
    bisection over the bit patterns of the positive float64 numbers, where the crossing index is monotone"""
    lo = np.float64(limit - (c + 2) * v).view(np.int64).item()   # crosses later than c (or not at all)
    hi = np.float64(np.nextafter(limit, 0.0)).view(np.int64).item()   # crosses at 1
    assert _cross_index(np.int64(lo).view(np.float64).item(), v, na + 2, limit) > c
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if _cross_index(np.int64(mid).view(np.float64).item(), v, na + 2, limit) > c:
            lo = mid
        else:
            hi = mid
    s0 = np.int64(hi).view(np.float64).item()   # the smallest start that crosses at c or earlier
    assert _cross_index(s0, v, na + 2, limit) == c, (c, v, s0)
    return s0


@pytest.mark.parametrize("tiles", (1, 3))
@pytest.mark.parametrize("v", (0.25, _V))
def test_crossing_position_exhaustive(v, tiles):
    """One tile of 256 steps with na steps of value v, the sum crossing 1024 at addition c of the na -- or not at all.
    tiles = 1: the tile is the segment's only one (never plain); tiles = 3: it is the middle one of three, a plain tile, the
    outer two hold zero rewards only.  v = 0.25: s0 = 1024 - c v is exact; v = 1/900: s0 from the backward search.
    c runs over 0, 1, 2, na - 1, na and na + 1: from s0 = 1024 - c v the sum REACHES 1024 with addition c, so "j additions
    stay in the binade and addition j + 1 leaves it" is c = j + 1 -- every j of (0, 1, na - 1, na) is among them both ways."""
    rv = (0.0, v)
    for na in (1, 2, 3, 120, 255, 256):
        for c in sorted({0, 1, 2, na - 1, na, na + 1}):
            # c = 0: the sum starts AT 1024 and stays in [1024, 2048); c = na + 1: it stays below 1024
            if v == 0.25:
                s0 = 1024.0 - c * v
            else:
                s0 = 1024.0 if c == 0 else _start_crossing_at(c, v, na)
            codes = _one_tile(na)
            if tiles == 3:
                codes = np.concatenate([np.zeros(256, np.int64), codes, np.zeros(256, np.int64)])
            crosses = 1 <= c <= na
            assert c == 0 or _cross_index(s0, v, na, 1024.0) == c
            stats = _check(codes, 32, 0, rv, s0)
            if crosses:
                assert stats[4:7].tolist() == [1, 1, 0] and stats[1:4].tolist() == [1, 0, 1], (na, c, stats.tolist())
            else:   # the whole advance holds: the path is not entered
                assert stats[1:7].tolist() == [0] * 6, (na, c, stats.tolist())
            assert stats[PLAIN] == ((1 if not crosses else 0) if tiles == 3 else 0), (na, c, stats.tolist())


@pytest.mark.parametrize("v", (0.25, _V))
def test_several_crossings_in_one_tile(v):
    codes = np.ones(256, np.int64)
    # from 0.0 there is no integer form: the float64 loop adds all 256, one rebase
    stats = _check(codes, 32, 0, (0.0, v), 0.0)
    assert stats[4:7].tolist() == [1, 0, 256] and stats[1:4].tolist() == [1, 0, 1], stats.tolist()
    # from v the sum is 257 v at the end: it leaves a binade at every 2^k v, k = 1 .. 8 -- counted from the plain loop
    s, crossings = v, 0
    for _ in range(256):
        t = s + v
        crossings += int(np.frexp(t)[1] != np.frexp(s)[1])
        s = t
    assert crossings == 8
    stats = _check(codes, 32, 0, (0.0, v), v)
    _only_single(stats)
    if v == 0.25:   # a power of two is no tie case in any binade above its own: every crossing in integers
        assert stats[4:7].tolist() == [1, crossings, 0] and stats[REBASE] == crossings, stats.tolist()
    else:   # (an odd mantissa is a tie case one binade up: the float64 loop takes the steps after that crossing)
        assert stats[SINGLE] == 1 and stats[REBASE] == stats[CROSS] + (1 if stats[FADD] else 0), stats.tolist()
        assert (stats[CROSS] == crossings) if stats[FADD] == 0 else (1 <= stats[CROSS] < crossings), stats.tolist()
        assert stats[CROSS] + stats[FADD] <= 256


def test_active_value_stops_advancing():
    ones = lambda n: np.ones(n, np.int64)   # noqa: E731
    # after the crossing v is exactly half a spacing -- a tie case -- and the sum saturates: the float64 loop takes the rest
    # (v = 0.25: four additions in integers, the fifth reaches 2^51, 251 + 44 in the float64 loop of the two tiles.  1/900 is
    # no power of two: near 2^53 v it is between half a spacing and a whole one, the sum keeps advancing; equality only)
    for v in (0.25, _V):
        s0 = 2.0 ** 53 * v - 5.0 * v
        stats = _check(ones(300), 32, 0, (0.0, v), s0)
        _only_single(stats)
        if v == 0.25:
            assert stats[4:7].tolist() == [2, 1, 295] and stats[REBASE] == 3, stats.tolist()
    assert _loop_sum(ones(300), (0.0, 0.25), 2.0 ** 51 - 1.25) == 2.0 ** 51   # saturated
    # q = 0 and no tie: the whole advance never fails, the path is not entered
    stats = _check(ones(300), 32, 0, (0.0, 1.0), 2.0 ** 60)
    assert stats[1:7].tolist() == [0] * 6, stats.tolist()
    # a tie from the start (v is half a spacing of [1, 2)), a subnormal value, a value at or above 2^(k+1): float64 loop only
    for v, s0 in ((2.0 ** -53, 1.0), (5e-324, 1.3125), (5e-324, 0.0)):
        stats = _check(ones(300), 32, 0, (0.0, v), s0)
        _only_single(stats)
        assert stats[SINGLE] == 2 and stats[CROSS] == 0 and stats[FADD] == 300, (v, s0, stats.tolist())
    # (after the first tile's 256 additions of 1.0 the sum is in [256, 512): the second tile's 44 advance in integers)
    stats = _check(ones(300), 32, 0, (0.0, 1.0), 1e-3)
    _only_single(stats)
    assert stats[4:7].tolist() == [1, 0, 256], stats.tolist()


def test_mixed_sequence_takes_both_paths():
    """DeepSea's rewards with a goal reward now and then: tiles with two nonzero values go the old way"""
    rng = np.random.RandomState(5)
    rv, pr = (0.0, _V, 1.0), (0.499, 0.499, 0.002)
    codes = rng.choice(3, 30_000 - 7, p=pr)
    stats = _check(codes, 30, 0, rv, 0.0)
    assert stats[WORD] >= 1 and stats[SINGLE] >= 1 and stats[PLAIN] >= 1 and stats[SLOW] > stats[SINGLE], stats.tolist()


def test_negative_reward_never_takes_the_path():
    rng = np.random.RandomState(6)
    total = np.zeros(8, np.int64)
    for H, n_words in ((9, 200), (30, 60), (45, 40)):
        for s0 in _STARTS:
            n = _steps_for(n_words, H, 0, rng)
            stats = _check(rng.choice(2, n), H, 0, (0.0, -0.25), s0, total)
            assert stats[4:7].tolist() == [0, 0, 0], stats.tolist()
    assert total[PLAIN] == 0 and total[SLOW] >= 1 and total[WORD] >= 1, total.tolist()


def test_random_segments():
    """2 000 seeded random segments: horizon, start time, length, reward set and start sum drawn at random"""
    rng = np.random.RandomState(2027)
    sets = list(_SETS.values()) + [
        ((0.0, _V, 1.0), (0.499, 0.499, 0.002)), ((0.0, 0.25), (0.5, 0.5)), ((0.0, 2.0 ** -53), (0.5, 0.5)),
        ((0.0, 5e-324), (0.5, 0.5)), ((0.0, 1.0), (0.7, 0.3)), ((0.0, 0.0, 1.0 / 3.0), (0.3, 0.3, 0.4))]
    horizons = (1, 2, 3, 5, 9, 17, 30, 31, 32, 33, 45, 64, 70)
    total = np.zeros(8, np.int64)
    for _ in range(2000):
        H = horizons[rng.randint(len(horizons))]
        nch = (H + 31) // 32
        h0 = rng.randint(0, H)
        n = _steps_for(nch * rng.randint(1, 70), H, h0, rng)
        rv, pr = sets[rng.randint(len(sets))]
        codes = rng.choice(len(rv), n, p=pr)
        s0 = (0.0, 1.3125, float(np.nextafter(2.0, 0.0)), float(rng.uniform(0.0, 600.0)), 2.0 ** 40 + 0.5, 1e-3,
              2.0 ** 53 * _V - 40.0 * _V)[rng.randint(7)]
        stats = _check(codes, H, h0, rv, s0, total)
        if len(rv) != 3 or rv[2] != 1.0 or pr[2] == 0.0:
            _only_single(stats)
    assert min(total[:7]) >= 1, total.tolist()
