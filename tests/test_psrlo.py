"""What the optimistic continuous PSRL agent (K18) rests on, checked without a device: golden G23 (the reference's
PSRLContinuous on its default path, tools/gen_golden_psrlo.py); the NumPy twin of tests/helpers_psrlo.py reproduces it bit for
bit; the library's host draw (cmdp_psrlo_reference_draw) equals the twin's NumPy draws on the tables replayed from G23; the
Python class computes the reference's psi and eta; the refusals; the constants."""
import ctypes as C
import hashlib
import json
import os
import re
import types

import numpy as np
import pytest

from conftest import ROOT
from colosseum_amd import _lib as L
from colosseum_amd import agents
from helpers_psrlc import vi_rule, JACOBI, GAUSS_SEIDEL
from helpers_psrlo import PSRLOTwin, numpy_sample_sa
from test_psrl import _same_state, _state_args

G23 = os.path.join(ROOT, "tests", "golden", "G23_psrlo.npz")
N_CASES = 6


def _cases():
    z = np.load(G23)
    return z, json.loads(str(z["cases"]))


def sha(T, R):
    return hashlib.sha256(np.ascontiguousarray(T).tobytes() + np.ascontiguousarray(R).tobytes()).hexdigest()


def golden_twin(z, m, i, **kw):
    Qs = z[f"c{i}_Q"]
    twin = PSRLOTwin(m["seed"], m["S"], m["A"], m["r_max"], m["psi"], m["eta"], None, **kw)
    twin.solver = lambda T, R: Qs[twin.episode]
    return twin


def run_golden(z, m, i, twin, before_sample=None, after_sample=None):
    steps, rewards, shas, ext = z[f"c{i}_steps"], z[f"c{i}_rewards"], z[f"c{i}_sha"], z[f"c{i}_extended"]
    kept = z[f"c{i}_kept"].tolist()
    S, A, psi = m["S"], m["A"], m["psi"]

    def check_sample():
        k = twin.episode - 1
        assert twin.last_T.dtype == np.float32 and twin.last_R_ext.dtype == np.float32
        assert twin.last_T.shape == (S, A * psi, S) and twin.last_R_ext.shape == (S, A * psi)
        assert sha(twin.last_T, twin.last_R_ext) == str(shas[k]), f"sample {k}"
        assert int((twin.last_T != 0).sum()) == int(z[f"c{i}_nnz"][k])
        assert twin.last_n == tuple(z[f"c{i}_n12"][k])
        assert twin.last_z + [-1] * (psi - len(twin.last_z)) == z[f"c{i}_z"][k].tolist(), f"z of sample {k}"
        if k in kept:
            j = kept.index(k)
            assert np.array_equal(twin.last_T, z[f"c{i}_T"][j]) and np.array_equal(twin.last_R, z[f"c{i}_R"][j]), f"stored sample {k}"
        if after_sample:
            after_sample(k, twin)

    if before_sample:
        before_sample(0, twin, True)
    twin.before_start_interacting()
    check_sample()
    for t in range(m["T"]):
        s, a, s2, ended = (int(x) for x in steps[t])
        assert twin.select_action(s) == a and twin.last_extended == int(ext[t]), f"action at step {t}"
        twin.step_update(s, a, float(rewards[t]), s2)
        assert twin.is_episode_end(s, a) == bool(ended), f"episode end at step {t}"
        if ended:
            if before_sample:
                before_sample(twin.episode, twin, False)
            twin.episode_end_update()
            check_sample()
    assert twin.episode == m["n_solves"]


def test_golden_covers_what_the_issue_asks():
    z, meta = _cases()
    assert len(meta) == N_CASES and os.path.getsize(G23) <= 1 << 20
    assert [(m["S"], m["A"], m["psi"], m["eta"], m["n_solves"]) for m in meta] == [
        (5, 2, 26, 50, 36), (4, 2, 5, 5, 32), (10, 2, 2, 100, 46), (9, 4, 3, 5, 106), (9, 5, 7, 5, 154), (43, 4, 60, 430, 36)]
    assert [m["T"] for m in meta] == [600] * 5 + [60]
    c = [m["calls"] for m in meta]
    assert c[0]["mixed"] == 3 and meta[0]["one_posterior_row"] == 3 and meta[0]["tie_broken_steps"] == 320
    assert (c[1]["mixed"], c[1]["all_posterior"], c[1]["all_simple"]) == (10, 7, 15)
    assert c[2]["mixed"] == 0 and c[2]["all_posterior"] == 0 and c[3]["mixed"] == 72 and c[4]["mixed"] == 121
    assert (meta[3]["S"] * meta[3]["A"] * meta[3]["psi"]) % 2 == 0 and meta[3]["S"] % 2 == 1
    assert (meta[4]["S"] * meta[4]["A"] * meta[4]["psi"]) % 2 == 1 and meta[4]["gauss_left_over"]
    assert meta[0]["simple_rows_with_nonzero_p_minus"] == 49
    # the scheme rule on the EXTENDED array: every solve of the 43-state case is Jacobi, every other Gauss-Seidel
    for i, m in enumerate(meta):
        want = JACOBI if i == 5 else GAUSS_SEIDEL
        assert all(vi_rule(m["S"], m["A"] * m["psi"], int(k)) == want for k in z[f"c{i}_nnz"]), i
        assert z[f"c{i}_Q"].shape == (m["n_solves"], m["S"], m["A"] * m["psi"])
    assert len(z["c5_kept"]) == 0 and "c5_T" not in z.files


@pytest.mark.parametrize("i", range(N_CASES))
def test_twin_reproduces_the_reference_bit_for_bit(i):
    z, meta = _cases()
    m = meta[i]
    twin = golden_twin(z, m, i)
    run_golden(z, m, i, twin)
    assert np.array_equal(twin.reward_hp, z[f"c{i}_final_reward_hp"]) and twin.reward_hp.dtype == np.float32
    assert np.array_equal(twin.transition_hp, z[f"c{i}_final_transition_hp"]) and twin.transition_hp.dtype == np.float32
    assert np.array_equal(twin.N, z[f"c{i}_final_N"]) and twin.N.dtype == np.int32


def layout_of(transition_hp, prior):
    """A layout of the dense hyper-parameters over `prior`: per row the positions that differ from it, ascending."""
    S, A, _ = transition_hp.shape
    rows = transition_hp.reshape(S * A, S)
    ptr, col, val = [0], [], []
    for r in rows:
        cs = np.flatnonzero(r != prior)
        col += cs.tolist()
        val += r[cs].tolist()
        ptr.append(len(col))
    return np.array(ptr, np.int64), np.array(col + [0], np.int32), np.array(val + [0], np.float32)


def library_draw(tw, first):
    """cmdp_psrlo_reference_draw on copies of the twin's three streams and on its tables: (outputs, states left behind)."""
    lib = L.load()
    S, A, psi = tw.S, tw.A, tw.psi
    ta, ra = _state_args(tw.rng_t), _state_args(tw.rng_r)
    aa = _state_args(np.random.RandomState(tw.seed) if first else tw.rng_a)
    prior = tw.transition_hp.min()   # counts only add to it
    ptr, col, val = layout_of(tw.transition_hp, prior)
    n_sa = np.ascontiguousarray(tw.N.sum(-1).ravel(), np.int32)
    rhp = np.ascontiguousarray(tw.reward_hp, np.float32)
    simple, n1 = np.zeros(S * A, np.uint8), np.zeros(1, np.int32)
    post, zz, R = np.full(psi * S * A * S, np.nan, np.float32), np.zeros(psi, np.int32), np.zeros(S * A, np.float32)
    L.check(lib.cmdp_psrlo_reference_draw(*[L.ptr(x) for x in ta], *[L.ptr(x) for x in ra], *[L.ptr(x) for x in aa], S, A, psi,
                                          float(tw.eta), S * A * psi if first else 0, L.ptr(n_sa), L.ptr(ptr), L.ptr(col), L.ptr(val),
                                          float(prior), L.ptr(rhp), L.ptr(simple), L.ptr(n1), L.ptr(post), L.ptr(zz), L.ptr(R)))
    n1 = int(n1[0])
    return dict(simple=simple.astype(bool).reshape(S, A), n1=n1, post=post[:psi * n1 * S].reshape(psi, n1, S), z=zz,
                R=R.reshape(S, A)), (ta, ra, aa)


@pytest.mark.parametrize("i", range(N_CASES))
def test_host_draw_is_numpy_on_the_twins_tables(i):
    """Every episode_end_update of G23's runs: the library draws on copies of the streams before the twin draws on the streams
    themselves; posterior rows, z, rewards, the simple mask and the three stream states (the randn skip of the first call and
    a cached Gaussian included) must be equal, no element exempt."""
    z, meta = _cases()
    m = meta[i]
    pending, drawn, kinds = {}, [], set()

    def sample_sa(tw, rows):
        r = numpy_sample_sa(tw, rows)
        drawn.append(np.array(r).reshape(len(rows[0]), tw.S))
        return r

    def before(k, tw, first):
        del drawn[:]
        pending["lib"] = library_draw(tw, first)

    def after(k, tw):
        out, (ta, ra, aa) = pending.pop("lib")
        n1, n2 = tw.last_n
        assert out["n1"] == n1 and np.array_equal(out["simple"], tw.last_simple)
        assert len(drawn) == (tw.psi if n1 else 0)
        if n1:
            assert np.array_equal(out["post"], np.stack(drawn)), k
        assert out["z"].tolist() == (tw.last_z if n2 else [-1] * tw.psi), k
        assert np.array_equal(out["R"], tw.last_R), k
        assert _same_state(ta, tw.rng_t) and _same_state(ra, tw.rng_r) and _same_state(aa, tw.rng_a), k
        kinds.add("mixed" if n1 and n2 else "all_posterior" if n1 else "all_simple")
        if n1 == 1:
            kinds.add("one_posterior_row")

    twin = golden_twin(z, m, i, sample_sa=sample_sa)
    twin.seed = m["seed"]
    run_golden(z, m, i, twin, before_sample=before, after_sample=after)
    want = [{"mixed", "one_posterior_row", "all_simple"}, {"mixed", "all_posterior", "all_simple"}, {"all_simple"},
            {"mixed", "all_simple"}, {"mixed", "all_simple"}, {"all_simple"}][i]
    assert want <= kinds


def test_host_draw_refusals():
    lib = L.load()
    assert lib.cmdp_psrlo_reference_draw(*([None] * 12), 2, 2, 2, 5.0, 0, *([None] * 4), 0.5, *([None] * 6)) == L.ERR_INVALID
    assert b"null" in lib.cmdp_last_error()
    tw = PSRLOTwin(0, 3, 2, 1.0, 2, 5.0, None)
    tw.seed = 0
    for bad, text in ((dict(eta=0.0), b"eta"), (dict(eta=float("nan")), b"eta")):
        for k, v in bad.items():
            setattr(tw, k, v)
        with pytest.raises(L.CmdpError, match=text.decode()):
            library_draw(tw, True)
        tw.psi, tw.eta = 2, 5.0


def test_python_class_yields_the_references_scalars():
    z, meta = _cases()
    for m in meta:
        psi, omega, eta, log4s = agents.optimistic_sampling_scalars(m["S"], m["A"], m["T"], **m["agent_params"])
        assert (psi, eta, omega) == (m["psi"], m["eta"], m["omega"]), m
        assert log4s == float(np.log(4 * m["S"]))
    assert agents.optimistic_sampling_scalars(10, 2, 600, psi_weight=0.05)[0] == 2          # the lower clamp
    assert agents.optimistic_sampling_scalars(43, 4, 60)[0] == 60                           # max_psi


def test_python_class_refusals():
    O = agents.BatchedPSRLContinuousOptimistic
    assert issubclass(O, agents.BatchedPSRLContinuous) and O._PREFIX == "cmdp_psrlc"
    small = types.SimpleNamespace(n_states=[16, 25], A=4, B=2)
    with pytest.raises(NotImplementedError, match="BatchedPSRLContinuous"):
        O(small, [0, 1], 100, no_optimistic_sampling=True)
    mixed = types.SimpleNamespace(n_states=[16, 1300], A=4, B=2)   # 1300^2 * 4 > 6 000 000
    with pytest.raises(NotImplementedError, match=r"instance 1.*6 000 000.*BatchedPSRLContinuous"):
        O(mixed, [0, 1], 100)
    for kw, text in ((dict(truncate_reward_with_max=True), "truncate_reward_with_max"),
                     (dict(min_steps_before_new_episode=5), "min_steps_before_new_episode"),
                     (dict(epsilon_greedy=0.1), "epsilon_greedy"), (dict(boltzmann_temperature=1.0), "boltzmann_temperature"),
                     (dict(reward_prior_model="N_N", rewards_prior_prms=[0, 1]), "N_NIG"),
                     (dict(transitions_prior_model="M_DIR", transitions_prior_prms=[[0.1, 0.2]]), "per-pair"),
                     (dict(get_psi=lambda *a: 3.0), "get_psi"), (dict(get_omega=lambda *a: 3.0), "get_omega"),
                     (dict(get_kappa=lambda *a: 3.0), "get_kappa"), (dict(get_eta=lambda *a: 3.0), "get_eta")):
        with pytest.raises(NotImplementedError, match=text):
            O(small, [0, 1], 100, **kw)
    with pytest.raises(ValueError):
        O(small, [0, 1], 100, sampler="mt")
    with pytest.raises(NotImplementedError):
        O.run_logged(None, None, 1)
    # the plain class names the new one where it refuses the default
    with pytest.raises(NotImplementedError, match="BatchedPSRLContinuousOptimistic"):
        agents.BatchedPSRLContinuous(small, [0, 1], 100)


def test_refusals_that_need_no_device():
    lib = L.load()
    h = C.c_void_p()
    seeds, rp, tp = np.zeros(1, np.int32), np.ones(4, np.float32), np.ones(1, np.float32)
    psi, eta, l4 = np.array([2], np.int32), np.array([5.0]), np.array([1.0])
    assert lib.cmdp_psrlc_create_optimistic(C.byref(h), None, L.ptr(seeds), 1000, L.ptr(rp), L.ptr(tp), L.ptr(psi), L.ptr(eta),
                                            L.ptr(l4), L.PSRL_SAMPLER_REFERENCE, L.ACTOR_GREEDY) == L.ERR_INVALID
    assert b"null" in lib.cmdp_last_error() and not h.value
    assert lib.cmdp_psrlc_create_optimistic(None, None, L.ptr(seeds), 1000, L.ptr(rp), L.ptr(tp), L.ptr(psi), L.ptr(eta), L.ptr(l4),
                                            0, 0) == L.ERR_INVALID
    assert lib.cmdp_psrlc_create_optimistic(C.byref(h), None, L.ptr(seeds), 1000, L.ptr(rp), L.ptr(tp), L.ptr(psi), L.ptr(eta),
                                            L.ptr(l4), L.PSRL_SAMPLER_REFERENCE, L.ACTOR_BOLTZMANN) == L.ERR_UNSUPPORTED
    assert lib.cmdp_psrlc_last_sample_optimistic(*([None] * 10)) == L.ERR_INVALID
    assert lib.cmdp_psrlc_counts(None, None) == L.ERR_INVALID


def test_declarations_agree():
    """Every new entry is declared in include/cmdp.h, bound in _lib.py and listed in its EXPORTS."""
    src = open(os.path.join(ROOT, "include", "cmdp.h")).read()
    lib = L.load()
    for name in ("cmdp_psrlc_create_optimistic", "cmdp_psrlc_last_sample_optimistic", "cmdp_psrlc_counts", "cmdp_psrlo_reference_draw"):
        assert re.search(r"\bint " + name + r"\(", src), name
        assert name in L.EXPORTS and getattr(lib, name).argtypes, name
    n_args = lambda name: re.search(name + r"\(([^;]*)\);", src).group(1).count(",") + 1  # noqa: E731
    for name in ("cmdp_psrlc_create_optimistic", "cmdp_psrlc_last_sample_optimistic", "cmdp_psrlc_counts", "cmdp_psrlo_reference_draw"):
        assert n_args(name) == len(getattr(lib, name).argtypes), name


def test_philox_restatement_is_a_function_of_its_arguments():
    """z lies in [0, S), differs between episodes and seeds and is spread over the states; the restated posterior rows are
    normalised like the reference's and depend on k."""
    from helpers_psrlo import philox_posterior_rows, philox_z

    z = philox_z(3, 5, 7, 4000)
    assert min(z) == 0 and max(z) == 6 and abs(np.bincount(z, minlength=7) / 4000 - 1 / 7).max() < 0.03
    assert z != philox_z(3, 6, 7, 4000) and z != philox_z(4, 5, 7, 4000) and z[:10] == philox_z(3, 5, 7, 10)
    hp = np.full((5, 2, 5), 0.2, np.float32)
    hp[1, 0, 2] += 9
    rows = (np.array([1, 3]), np.array([0, 1]))
    T0, tol = philox_posterior_rows(3, 5, hp, 4, rows, 0)
    T1, _ = philox_posterior_rows(3, 5, hp, 4, rows, 1)
    assert T0.shape == (2, 5) and T0.dtype == np.float32 and (T0 >= 0).all() and not np.array_equal(T0, T1)
    assert np.abs(T0.astype(np.float64).sum(-1) - 1).max() < 1e-3 and T0[0, 2] > 0.5 and (tol > 0).all()
    assert np.array_equal(T0[:1], philox_posterior_rows(3, 5, hp, 4, (rows[0][:1], rows[1][:1]), 0)[0])
