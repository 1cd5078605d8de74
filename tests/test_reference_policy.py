"""CMDP_POLICY_RANDOM_REFERENCE, CPU part: the host twins of the device generator K16 (csrc/cmdp_actions.h) against numpy.

`cmdp_mt_randint` and `cmdp_mt_action_bits` are built from the functions the kernel draws with (twist of one word, tempering,
mask, accept test); the reference's RandomActor (colosseum/agent/actors/random.py:34-47) pops
`RandomState(seed).randint(0, A, 50_000)` blocks, which are consecutive pieces of one word stream."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from colosseum_amd import _lib as L

SEEDS = (0, 1, 7, 12345, 2**32 - 1)
N_ACTIONS = (1, 2, 3, 4, 5, 6, 7, 16, 17, 127)
LENGTHS = (1, 623, 624, 625, 5000)


def _randint(state, A, n):
    """(actions, new state) -- `state` as RandomState.get_state()."""
    key = np.ascontiguousarray(state[1], np.uint32).copy()
    pos = C.c_int32(int(state[2]))
    out = np.full(n, -1, np.int8)
    L.check(L.load().cmdp_mt_randint(L.ptr(key), C.byref(pos), int(A), int(n), L.ptr(out)))
    return out, ("MT19937", key, pos.value, 0, 0.0)


def _bits(state, n, offset, out):
    key = np.ascontiguousarray(state[1], np.uint32).copy()
    pos = C.c_int32(int(state[2]))
    L.check(L.load().cmdp_mt_action_bits(L.ptr(key), C.byref(pos), int(n), int(offset), L.ptr(out)))
    return ("MT19937", key, pos.value, 0, 0.0)


def _same_state(got, rs):
    want = rs.get_state()
    return got[2] == want[2] and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("A", N_ACTIONS)
def test_mt_randint_equals_numpy(A):
    """Action for action, and the state left behind is numpy's; then the same total drawn in three calls."""
    for seed in SEEDS:
        for n in LENGTHS:
            rs = np.random.RandomState(seed)
            got, st = _randint(rs.get_state(), A, n)
            want = rs.randint(0, A, n)
            np.testing.assert_array_equal(got, want, err_msg=f"seed {seed} A {A} n {n}")
            assert _same_state(st, rs), (seed, A, n)
            # three calls continue one stream
            st = np.random.RandomState(seed).get_state()
            parts = (n // 3, n // 2 - n // 3, n - n // 2)
            got3 = []
            for m in parts:
                g, st = _randint(st, A, m)
                got3.append(g)
            np.testing.assert_array_equal(np.concatenate(got3), want, err_msg=f"seed {seed} A {A} n {n} in {parts}")
            assert _same_state(st, rs), (seed, A, n)


@pytest.mark.parametrize("offset", (0, 1, 31, 32, 127))
def test_mt_action_bits_equal_numpy_packed(offset):
    for seed in SEEDS:
        for n in (1, 128, 129, 1300):
            rs = np.random.RandomState(seed)
            rs.randint(0, 2, 100 * (seed % 7))   # somewhere inside the first block
            n_words = (offset + n + 31) // 32 + 2
            fill = np.random.RandomState(5).randint(0, 2**32, n_words, dtype=np.uint64).astype(np.uint32)
            out = fill.copy()
            st = _bits(rs.get_state(), n, offset, out)
            want = rs.randint(0, 2, n)
            q = offset + np.arange(n)
            got = (out[q >> 5] >> (q & 31).astype(np.uint32)) & 1
            np.testing.assert_array_equal(got, want, err_msg=f"seed {seed} n {n}")
            assert _same_state(st, rs)
            # nothing outside the written span is touched: whole words, and the other bits of the two partial words
            mask = np.zeros(n_words, np.uint32)
            np.bitwise_or.at(mask, q >> 5, (np.uint32(1) << (q & 31).astype(np.uint32)))
            np.testing.assert_array_equal(out & ~mask, fill & ~mask)


def test_golden_action_streams_are_such_streams():
    """What lets the GPU tests hold the new policy against the reference's recorded trajectories with nothing uploaded: every
    stored action stream of these goldens is RandomState(seed).randint(0, A, n), and the host twin reproduces it."""
    from conftest import load_golden

    seed_of = {"G1_deepsea8": lambda i, c: 1000 + c["kwargs"]["seed"], "G2_deepsea30": lambda i, c: c["kwargs"]["seed"],
               "G3_stochastic": lambda i, c: 77 + i, "G12_families": lambda i, c: 500 + i}
    seen = set()
    for name, f in seed_of.items():
        z, cases = load_golden(name)
        for i, c in enumerate(cases):
            want = z[f"c{i}_actions"]
            A = int(z[f"c{i}_SAH"][1])
            got, _ = _randint(np.random.RandomState(f(i, c)).get_state(), A, len(want))
            np.testing.assert_array_equal(got, want, err_msg=f"{name} case {i}")
            seen.add(A)
    assert seen == {2, 3, 4, 5, 6}


def test_mt_twins_refuse_bad_arguments():
    st = np.random.RandomState(3).get_state()
    for bad in (("MT19937", st[1], 625, 0, 0.0), ("MT19937", st[1], -1, 0, 0.0)):
        with pytest.raises(L.CmdpError):
            _randint(bad, 2, 4)
        with pytest.raises(L.CmdpError):
            _bits(bad, 4, 0, np.zeros(2, np.uint32))
    for A in (0, 129):
        with pytest.raises(L.CmdpError):
            _randint(st, A, 4)


def test_python_constants_equal_the_header():
    src = open(os.path.join(ROOT, "include", "cmdp.h")).read()
    for name, val in (("CMDP_POLICY_RANDOM", L.POLICY_RANDOM), ("CMDP_POLICY_HOST_ACTIONS", L.POLICY_HOST_ACTIONS),
                      ("CMDP_POLICY_GREEDY_Q", L.POLICY_GREEDY_Q), ("CMDP_POLICY_RANDOM_REFERENCE", L.POLICY_RANDOM_REFERENCE),
                      ("CMDP_STAT_ACTIONS_KERNEL_MS", L.STAT_ACTIONS_KERNEL_MS)):
        m = re.search(r"\b%s\s*=\s*(\d+)" % name, src)
        assert m and int(m.group(1)) == val, name
    assert L.POLICY_RANDOM_REFERENCE == 3
    for sym in ("cmdp_set_action_streams", "cmdp_action_stream_state", "cmdp_set_action_stream_state", "cmdp_mt_randint",
                "cmdp_mt_action_bits"):
        assert sym in L.EXPORTS and hasattr(L.load(), sym)
