"""The batch solvers that take no environment handle (cmdp_gth, cmdp_extended_vi, cmdp_vi_discounted_model,
cmdp_vi_episodic_dense, cmdp_vi_episodic_map) keep one workspace per device each, which only grows and is reused by every
call.  One sequence of calls through the five Python wrappers in which every workspace shrinks, regrows and sees the other
solvers' calls in between: what a call returns depends on its own problems alone, bit for bit."""
import numpy as np
import pytest

import helpers_chains as HC
import helpers_map_vi as HM
import helpers_model_vi as HV
from helpers_evi import random_problem
from colosseum_amd import dynamic_programming as dp
from colosseum_amd.markov_chain import gth_batch

pytestmark = pytest.mark.gpu

SIZES, ACTIONS, HORIZON = (2, 65, 3), (2, 1, 3), 3   # ragged: the middle problem is the largest, the first the smallest
SHAPES = list(zip(SIZES, ACTIONS))


def _chains():
    d = HC.generate([("sparse_irreducible", S, {}) for S in SIZES], 31, A=3)
    return [HC.policy_chain(d["t"], b, d["acts"][b]) for b in range(len(SIZES))]


def _map_tables():
    return [HM.tables(S, A, seed=40 + i) for i, (S, A) in enumerate(SHAPES)]


def _evi(problems):
    out, sweeps = dp.extended_value_iteration_batch(problems, max_sweeps=3000)
    return [(sweeps[b],) + (() if o is None else tuple(o)) for b, o in enumerate(out)]   # no (span, Q, V): status not OK


def _model_vi(problems):
    out, sweeps, schemes = dp.discounted_value_iteration_batch(problems)
    return [(sweeps[b], schemes[b]) + (() if o is None else tuple(o)) for b, o in enumerate(out)]


# name -> (the three problems of batch X, problems -> one tuple of outputs per problem)
SOLVERS = {
    "gth": (_chains, lambda ps: [(x,) for x in gth_batch(ps)]),
    "extended_vi": (lambda: [random_problem(S, A, seed=50 + i, kind=("bernstein", "chernoff")[i % 2])
                             for i, (S, A) in enumerate(SHAPES)], _evi),
    "model_vi": (lambda: [HV.make_fixture(S, A, mix, 60 + i).dense()
                          for i, ((S, A), mix) in enumerate(zip(SHAPES, ("state_0", "two_c", "full_csr_row")))], _model_vi),
    "episodic_dense": (lambda: [(HM.map_estimate(thp), mu) for thp, mu, _ in _map_tables()],
                       lambda ps: dp.episodic_value_iteration_dense_batch(ps, HORIZON)),
    "episodic_map": (_map_tables, lambda ps: dp.episodic_value_iteration_map_batch(ps, HORIZON, return_map=True)),
}


def assert_same(got, want, where):
    assert len(got) == len(want), where
    for i, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w), (where, i)
        for k, (x, y) in enumerate(zip(g, w)):
            x, y = np.asarray(x), np.asarray(y)
            assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y), (where, i, k)


def test_workspaces_shrink_regrow_and_interleave(need_gpu):
    X = {name: make() for name, (make, _) in SOLVERS.items()}

    def round_of(batch):
        return {name: call(batch(X[name])) for name, (_, call) in SOLVERS.items()}

    first = round_of(lambda x: x)
    alone = round_of(lambda x: x[:1])
    second = round_of(lambda x: x)
    both = round_of(lambda x: x + x[::-1])
    third = round_of(lambda x: x)
    for name in SOLVERS:
        assert len(first[name]) == 3
        assert_same(second[name], first[name], (name, "X again"))
        assert_same(third[name], first[name], (name, "X once more"))
        assert_same(both[name][:3], first[name], (name, "first half of Y"))
        assert_same(both[name][3:][::-1], first[name], (name, "second half of Y"))
        assert_same(alone[name], first[name][:1], (name, "alone"))
