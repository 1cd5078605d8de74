"""The Markov-chain kernels on generated chains: K7 (k_gth), K9 (k_chain_average_reward) and K9F (k_chain_fast with its
host planner plan_chains of cmdp_chain_plan.h, which is also held against a Python mirror and the promises k_chain_fast
relies on, without a GPU) against CPU references only -- the reference's own class bookkeeping over the oracle's GTH
(bit for bit, K7 and K9 in the reference's order) and float64 GTH in numpy (the reordered sums of the default order).

The chains (helpers_chains.SUITE) are built to reach what the family MDPs never do: packed columns of more than 256
non-zeros, row / column scans beyond 512 entries, pivots with 65 to 128 candidates, instances without a plan beside planned
ones, K9 and K9F taking turns on one workspace, closed classes of 1, 2 and many states behind permuted labels, the float32
branch above 128 and 256 states, and the largest instance K9's LDS admits."""
import ctypes as C

import numpy as np
import pytest

import helpers_chains as H

# ---- tolerance of the default order (K9 with butterfly sums, K9F in its own elimination order) ------------------------------
# GTH is subtraction-free: another elimination or summation order moves the result by rounding only.  G64 / G32 are the
# largest relative gaps of the average reward, over every chain of the suite with a float64 / float32 result, between four
# elimination orders of the float64 numpy GTH (index, reverse, two seeded random permutations), each pushed through the
# reference's own bookkeeping (float32 results: its float32 distribution and float32 pairwise sum).
# test_order_sensitivity_of_the_suite measures them on the CPU and fails when a measurement exceeds the figure recorded
# here; measured: G64 = 1.94e-15 (sparse ring of 1 023 states), G32 = 0 (no reordering moved a float32 result at all).
# The device may differ from the index-order CPU reference by 16 times that: butterfly sums and K9F's order are further
# reorderings of the same sums.  A float32 result moves in steps of its own roundoff, so a measured 0 cannot be scaled:
# a float64 change of 1e-15 that crosses a float32 rounding boundary shows as one unit in the last place, and that -- 2^-23
# relative, the precision of the format -- is the float32 tolerance.
G64 = 2e-15
G32 = 0.0
REL64 = 16 * G64
REL32 = max(16 * G32, 2.0 ** -23)
CAP64, CAP32 = 1e-11, 1e-6   # conditions, not measurements: what tests/test_gpu_chain.py allows


# ---- host-only checks -----------------------------------------------------------------------------------------------------
def test_lds_formulas_mirror_the_header():
    c, k9, k9f = H.parse_header()
    assert (c["K9F_MAXC"], c["NW"], c["PFB"], c["PF"]) == (H.K9F_MAXC, H.K9F_NW, H.PFB, H.PF)
    for S in (1, 2, 64, 190, 600, 1706, 1707):
        for deg in (1, 4, 40, S):
            assert k9(S, deg) == H.chain_lds_bytes(S, deg)
            assert k9f(S, deg, c["NW"]) == H.chain_fast_lds_bytes(S, deg)
    assert (H.DENSE_MAX, H.S_MAX4) == (192, 1706)
    assert H.chain_lds_bytes(H.S_MAX4, 4) <= H.LDS_BUDGET < H.chain_lds_bytes(H.S_MAX4 + 1, 4)
    assert H.chain_lds_bytes(H.DENSE_MAX, H.DENSE_MAX) <= H.LDS_BUDGET < H.chain_lds_bytes(H.DENSE_MAX + 1, H.DENSE_MAX + 1)


def test_header_parser_sees_a_changed_constant(tmp_path):
    src = open(H.CHAIN_H).read()
    p = tmp_path / "cmdp_chain.h"
    p.write_text(src.replace("12 * (size_t)S + 1", "13 * (size_t)S + 1", 1))
    assert H.parse_header(str(p))[1](100, 4) == H.chain_lds_bytes(100, 4) + 400
    p.write_text(src.replace("#define K9F_KC 2", "#define K9F_KC 3", 1))
    assert H.parse_header(str(p))[0]["K9F_MAXC"] == 192


def test_lds_gap_size():
    """With 4 entries per row K9F fits wherever K9 does; with one row of 40 entries there are sizes that K9 alone fits."""
    assert all(H.chain_fast_lds_bytes(S, 4) <= H.LDS_BUDGET for S in range(1, H.S_MAX4 + 1))
    assert H.chain_lds_bytes(H.GAP_S, H.GAP_NNZ) <= H.LDS_BUDGET < H.chain_fast_lds_bytes(H.GAP_S, H.GAP_NNZ)
    assert H.max_row_nnz(H.suite("lds_gap")["t"]) == H.GAP_NNZ


@pytest.mark.parametrize("name", sorted(H.SUITE) + ["refused"])
def test_generator_tables_are_well_formed(name):
    d = H.suite(name)
    t = d["t"]
    A, off, ptr, col, val = t["A"], t["state_off"], t["csr_ptr"], t["csr_col"], t["csr_val"]
    assert A >= 2 and t["H"] == 0 and len(ptr) == off[-1] * A + 1
    assert H.chain_lds_bytes(int(np.diff(off).max()), H.max_row_nnz(t)) <= H.LDS_BUDGET or name == "refused"
    for b in range(t["B"]):
        S = int(off[b + 1] - off[b])
        act = d["acts"][b]
        for s in range(S):
            rows = []
            for a in range(A):
                r = (off[b] + s) * A + a
                c, v = col[ptr[r]:ptr[r + 1]], val[ptr[r]:ptr[r + 1]]
                assert len(c) >= 1 and (np.diff(c) > 0).all() and 0 <= c[0] and c[-1] < S   # ascending, no duplicates
                assert (v >= 0).all() and v.astype(np.float64).sum() == pytest.approx(1.0, abs=2e-6)
                rows.append((c.tolist(), v.tolist(), float(t["R"][r])))
            # picking another action than the policy's shows: its row or at least its reward differs
            assert all(rows[a] != rows[act[s]] for a in range(A) if a != act[s])
            if S > 1:
                assert all(rows[a][:2] != rows[act[s]][:2] for a in range(A) if a != act[s])
    v = t["csr_val"]
    if name in ("sparse_mid", "multi_class", "one_class_with_transients", "mixed"):
        assert (v == 0).any() and (v > 1).any() and ((v > 0) & (v < 2e-7)).any()


@pytest.mark.parametrize("name,b", H.instances())
def test_generator_makes_the_intended_structure(name, b):
    """Class count, kind of the result, the class the start state is sent to, periodicity, and -- where the structure decides
    it -- whether plan_chains has a plan (the minimum-degree mirror)."""
    d = H.suite(name)
    m = d["meta"][b]
    t, act, start = d["t"], d["acts"][b], d["starts"][b]
    value, classes = H.reference(t, b, act, start)
    assert len(classes) == m["n_classes"] == H.suite_reference(name, b)[1]
    assert type(value) is m["kind"]
    P = H.policy_chain(t, b, act)
    S = len(P)
    if m["n_classes"] == 1 and m["kind"] is np.float64:
        assert len(classes[0]) == S
    if m["kind"] is np.float32:
        assert 1 < len(classes[0]) < S
    if m.get("period") == 2:   # bipartite: no edge inside a colour class of the class's 2-colouring by parity of the ring
        assert S % 2 == 0 and not (P[0::2, 0::2] > 0).any() and not (P[1::2, 1::2] > 0).any()
    if m["fast"] is not None:
        worst, first = (0, 0) if S < 2 else H.min_degree_max_candidates(t, b, stop=H.K9F_MAXC)
        planned = S >= 2 and worst <= H.K9F_MAXC
        assert (planned and m["n_classes"] == 1 and m["kind"] is np.float64) == m["fast"], (worst, first)
        if m["name"] == "dense_irreducible":
            assert first == S - 1 and (64 < first <= 128) == m["fast"]   # the second candidate chunk, or no plan
    if m["name"] in ("multi_class", "reuse"):
        sizes = sorted(len(c) for c in classes)
        assert sizes[0] == 1 and 2 in sizes and sizes[-1] > 64 or len(classes) == 12


def test_multi_class_starts_cover_the_selection():
    """Among the multi-class chains: labels are permuted so that the classes' list order is not their label order; starts
    inside a class pick that class, first in the list or not; a transient start that reaches several classes is sent to
    the first of THOSE in list order, which is not always the first of the list."""
    import colosseum_amd.markov_chain as mc
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import breadth_first_order

    d = H.suite("multi_class")
    chosen_not_first = transient_several = transient_not_first = unsorted_list = 0
    for b, m in enumerate(d["meta"]):
        P = H.policy_chain(d["t"], b, d["acts"][b])
        classes = mc.recurrent_classes(P)
        reach = set(breadth_first_order(csr_matrix(P > 0), d["starts"][b], directed=True, return_predecessors=False).tolist())
        hit = [i for i, c in enumerate(classes) if int(c[0]) in reach]
        recurrent = any(d["starts"][b] in c for c in classes)
        assert hit and (len(hit) == 1) == (recurrent or len(hit) == 1)
        chosen_not_first += hit[0] != 0
        transient_several += (not recurrent) and len(hit) > 1
        transient_not_first += (not recurrent) and len(hit) > 1 and hit[0] != 0
        unsorted_list += [int(c.min()) for c in classes] != sorted(int(c.min()) for c in classes)
    assert chosen_not_first >= 3 and transient_several >= 3 and transient_not_first >= 1 and unsorted_list >= 3


@pytest.mark.parametrize("name,b", [(n, b) for n in ("in_hub", "expander") for b in range(len(H.SUITE[n][0]))])
def test_index_order_elimination_fills_long_columns(name, b):
    """K9's back-substitution keeps 64 * PFB = 256 entries of a packed column in registers and reads the rest from memory:
    these chains must give it such columns (and, from 514 states, scans beyond 64 * PF = 512 entries)."""
    d = H.suite(name)
    st = {}
    H.gth_numpy(H.policy_chain(d["t"], b, d["acts"][b]), stats=st)
    print(f"{name}[{b}] S={d['meta'][b]['S']}: longest packed column {st['max_col']}")
    if (name, d["meta"][b]["S"]) == ("expander", 300):
        # 3 random successors fill the first pivots' columns too slowly: pivot i has 299 - i rows left, and more than 256
        # of them non-zero needs a nearly full column within 42 pivots.  Measured: 115.  The 800-state expander has them.
        assert 64 < st["max_col"] <= 64 * H.PFB
        return
    assert st["max_col"] > 64 * H.PFB
    if name == "in_hub" and d["meta"][b]["S"] >= 514:
        assert st["max_col"] > 64 * H.PF


def _irreducible():
    return [(n, b) for n, b in H.instances() if H.suite(n)["meta"][b]["n_classes"] == 1
            and H.suite(n)["meta"][b]["kind"] is np.float64 and H.suite(n)["meta"][b]["S"] <= 1100]


@pytest.mark.parametrize("name,b", _irreducible())
def test_numpy_gth_equals_oracle_gth(name, b):
    """The two CPU references agree bit for bit where they compute the same thing: index-order GTH of a whole chain."""
    from oracle import oracle as O

    d = H.suite(name)
    P = H.policy_chain(d["t"], b, d["acts"][b])
    np.testing.assert_array_equal(H.gth_numpy(P), O.gth(P))


def test_numpy_gth_early_stop_equals_oracle():
    from oracle import oracle as O

    P = _absorbing_first(40)
    x = O.gth(P)
    assert x[0] == 1.0 and not x[1:].any()
    np.testing.assert_array_equal(H.gth_numpy(P), x)


def _absorbing_first(n):
    P = np.random.default_rng(n).dirichlet(np.ones(n), n)
    P[0] = 0.0
    P[0, 0] = 1.0
    return P


def _order_gaps(name, b):
    d = H.suite(name)
    vals = [H.reference(d["t"], b, d["acts"][b], d["starts"][b], solve=H.ordered_gth(k))[0] for k in H.ORDERS]
    assert len({type(v) for v in vals}) == 1
    v = np.array(vals, np.float64)
    return type(vals[0]), float((v.max() - v.min()) / np.abs(v).min())


def test_order_sensitivity_of_the_suite():
    """Measures G64 and G32 (see the top of the file) and holds them against the recorded figures and the caps."""
    g = {np.float64: 0.0, np.float32: 0.0}
    for name, b in H.instances():
        kind, gap = _order_gaps(name, b)
        print(f"order gap {name}[{b}] {kind.__name__}: {gap:.3e}")
        g[kind] = max(g[kind], gap)
    print(f"measured G64 = {g[np.float64]:.3e}, G32 = {g[np.float32]:.3e}")
    assert g[np.float64] <= G64 and g[np.float32] <= G32
    assert 0 < REL64 <= CAP64 and 0 < REL32 <= CAP32


# ---- K9F's planner and the kernel choice, through the host-only entry points ------------------------------------------------
PLAN_ARRAYS = ("rank", "cptr", "cbase", "cand", "nrounds", "rbase", "rptr", "piv")


@pytest.mark.parametrize("name", ["one_state", "sparse_small", "periodic", "dense_planned", "dense_unplanned", "multi_class", "mixed",
                                  "two_components"])
def test_plan_equals_the_python_mirror(name):
    """All eight arrays of cmdp_chain_plan_desc equal the mirror's: S = 1 (no plan) and S = 2, 128 candidates against 129,
    planned instances beside unplanned ones (the packing of cbase / rbase), planned or not as the generator meant, and a
    graph of two components whose last position is listed for the last time long before the last round."""
    from colosseum_amd.batched import chain_plan_of_tables

    d = H.suite(name)
    got, want = chain_plan_of_tables(d["t"]), H.plan_mirror(d["t"])
    for k in PLAN_ARRAYS:
        assert got[k].dtype == want[k].dtype, k
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{name}: {k}")
    for b, m in enumerate(d["meta"]):
        if m["S"] == 1:
            assert got["nrounds"][b] == -1
        if m["fast"] is not None:
            assert (got["nrounds"][b] >= 0 and m["n_classes"] == 1 and m["kind"] is np.float64) == m["fast"], (name, b)
    planned = got["nrounds"] >= 0
    if name in ("dense_planned", "dense_unplanned"):
        assert planned.all() == (name == "dense_planned") and planned.any() == (name == "dense_planned")
    if name == "mixed":
        assert planned[0] and not planned[1] and planned[2] and not planned[3]   # a planned instance after unplanned ones
    if name == "two_components":   # what helpers_chains.two_components says of itself
        assert got["rank"][:13].tolist() == list(range(13)) and got["nrounds"].tolist() == [10, 1]
        assert got["piv"][:12].tolist() == [0, 10, 1, 11, 2, 3, 4, 5, 6, 7, 8, 9]


@pytest.mark.parametrize("name", sorted(H.SUITE) + ["refused", "two_components"])
def test_plan_keeps_what_the_kernel_takes_on_trust(name):
    """From the arrays of cmdp_chain_plan_desc alone, what k_chain_fast relies on (the K9F comment of cmdp_chain.h)."""
    from colosseum_amd.batched import chain_plan_of_tables

    t = H.suite(name)["t"]
    p = chain_plan_of_tables(t)
    off, B = t["state_off"], int(t["B"])
    n_planned = 0
    for b in range(B):
        so, S = int(off[b]), int(off[b + 1] - off[b])
        c_end = int(p["cbase"][b + 1]) if b + 1 < B else len(p["cand"])
        r_end = int(p["rbase"][b + 1]) if b + 1 < B else len(p["rptr"])
        nr = int(p["nrounds"][b])
        if nr < 0:   # no plan: no room taken, nothing written
            assert nr == -1 and c_end == p["cbase"][b] and r_end == p["rbase"][b]
            assert (p["rank"][so: so + S] == -1).all() and not p["cptr"][so + b: so + b + S + 1].any()
            continue
        n_planned += 1
        rank = p["rank"][so: so + S].astype(np.int64)
        assert sorted(rank.tolist()) == list(range(S))
        cp = p["cptr"][so + b: so + b + S + 1].astype(np.int64)
        n = np.diff(cp)
        assert cp[0] == 0 and (n >= 0).all() and n.max() <= H.K9F_MAXC and p["cbase"][b] + cp[S] == c_end
        cand = p["cand"][int(p["cbase"][b]): c_end].astype(np.int64)
        owner = np.repeat(np.arange(S), n)
        assert (cand > owner).all() and (cand < S).all()                   # strictly above the pivot's position
        assert (np.diff(cand)[np.diff(owner) == 0] > 0).all()              # ascending within a list
        lists = np.zeros((S, S), bool)
        lists[owner, cand] = True
        u, v = np.nonzero(H.transition_graph(t, b))
        up = rank[u] < rank[v]
        assert lists[rank[u][up], rank[v][up]].all()                       # every neighbour that ranks higher is listed
        rp = p["rptr"][int(p["rbase"][b]): r_end].astype(np.int64)
        width = np.diff(rp)
        assert len(rp) == nr + 1 and rp[0] == 0 and rp[-1] == S - 1 and (width >= 1).all() and (width <= H.K9F_NW).all()
        piv = p["piv"][so: so + S - 1].astype(np.int64)
        assert sorted(piv.tolist()) == list(range(S - 1))                  # every pivot scheduled exactly once
        round_of = np.full(S, nr, np.int64)                                # (the last position is eliminated by nobody)
        round_of[piv] = np.repeat(np.arange(nr), width)
        assert (round_of[cand] > round_of[owner]).all()                    # after every lower pivot that lists it
        f = lists.astype(np.float32)
        for r in range(nr):
            rnd = piv[rp[r]: rp[r + 1]]
            assert not lists[np.ix_(rnd, rnd)].any()                       # not each other's candidates
            common = f[rnd] @ f[rnd].T
            assert (common[~np.eye(len(rnd), dtype=bool)] <= 1).all()      # at most one shared candidate
    print(f"{name}: {n_planned} of {B} planned, {len(p['cand'])} candidates, {len(p['rptr'])} round offsets")
    assert n_planned >= sum(m["fast"] is True for m in H.suite(name)["meta"])   # the checks above had something to check
    assert n_planned == B or name != "two_components"


def test_chain_choice_follows_the_lds_formulas():
    from colosseum_amd import _lib as L
    from colosseum_amd.batched import chain_choice

    def shape(name):
        t = H.suite(name)["t"]
        return int(np.diff(t["state_off"]).max()), H.max_row_nnz(t)

    for name in ("lds_gap", "at_lds_limit", "sparse_small", "dense_unplanned"):
        S, deg = shape(name)
        c = chain_choice(S, deg)
        assert (c["refusal"], c["k9_lds"], c["fast_lds"]) == (L.OK, H.chain_lds_bytes(S, deg), H.chain_fast_lds_bytes(S, deg)), name
        assert c["fast"] == (H.chain_fast_lds_bytes(S, deg) <= H.LDS_BUDGET), name
        assert c["fast"] == {"lds_gap": False, "at_lds_limit": True}.get(name, c["fast"])   # K9 alone; both kernels
        for kw in (dict(exact_order=True), dict(fast_enabled=False), dict(any_plan=False)):
            c = chain_choice(S, deg, **kw)
            assert c["refusal"] == L.OK and not c["fast"] and c["k9_lds"] == H.chain_lds_bytes(S, deg), (name, kw)
    assert shape("at_lds_limit") == (H.S_MAX4, 4) and shape("refused") == (H.S_MAX4 + 1, 4)
    for kw in ({}, dict(exact_order=True), dict(fast_enabled=False)):
        assert chain_choice(*shape("refused"), **kw)["refusal"] == L.ERR_UNSUPPORTED


def test_plan_entry_points_reject_bad_arguments():
    from colosseum_amd import _lib as L
    from colosseum_amd.batched import chain_plan_of_tables, desc_from_tables

    lib = L.load()
    t = H.suite("sparse_small")["t"]
    NS, B = int(t["state_off"][-1]), int(t["B"])
    n_cand = len(chain_plan_of_tables(t)["cand"])
    d, keep = desc_from_tables(t, L.RNG_PHILOX)
    arr = dict(rank=np.zeros(NS, np.int32), cptr=np.zeros(NS + B, np.int32), cbase=np.zeros(B, np.int64), cand=np.zeros(n_cand, np.uint16),
               nrounds=np.zeros(B, np.int32), rbase=np.zeros(B, np.int64), rptr=np.zeros(NS + B, np.int32), piv=np.zeros(NS, np.int32))
    n = C.c_int64()

    def call(desc, capacity=n_cand, n_out=C.byref(n), **nulls):
        a = {k: None if k in nulls else L.ptr(v) for k, v in arr.items()}
        return lib.cmdp_chain_plan_desc(desc, a["rank"], a["cptr"], a["cbase"], a["cand"], capacity, n_out, a["nrounds"], a["rbase"],
                                        a["rptr"], a["piv"])

    assert call(C.byref(d)) == L.OK and n.value == n_cand            # exactly enough room
    n.value = 0
    assert call(C.byref(d), capacity=n_cand - 1) == L.ERR_INVALID and n.value == n_cand   # one short: says how many
    for k in arr:
        assert call(C.byref(d), **{k: True}) == L.ERR_INVALID, k
    assert call(C.byref(d), n_out=None) == L.ERR_INVALID and call(None) == L.ERR_INVALID
    bare, keep2 = desc_from_tables({k: v for k, v in t.items() if not k.startswith("csr_")}, L.RNG_PHILOX)
    assert call(C.byref(bare)) == L.ERR_INVALID and b"DP half" in lib.cmdp_last_error()
    bad = dict(t, csr_col=np.where(np.arange(len(t["csr_col"])) == 5, 99, t["csr_col"]).astype(np.int32))
    d3, keep3 = desc_from_tables(bad, L.RNG_PHILOX)
    assert call(C.byref(d3)) == L.ERR_INVALID
    out = np.zeros(4, np.int64)
    assert lib.cmdp_chain_choice(10, 4, 0, 1, 1, None) == L.ERR_INVALID and lib.cmdp_chain_choice(0, 4, 0, 1, 1, L.ptr(out)) == L.ERR_INVALID


# ---- device tests -----------------------------------------------------------------------------------------------------------
gpu = pytest.mark.gpu


def _run(d, exact, mask=None, acts=None, env=None):
    """(values, class counts, K9F's instance count) of one average-reward call, on a fresh handle unless one is given."""
    from colosseum_amd import _lib as L
    from colosseum_amd.batched import BatchedMDP

    own = env is None
    if own:
        env = BatchedMDP(tables=d["t"], with_env=False)
    env.set_option(L.OPT_CHAIN_EXACT_ORDER, int(exact))
    vals, ncls = env.average_reward(d["acts"] if acts is None else acts, d["starts"], mask=mask)
    n_fast = C.c_double()
    L.check(L.load().cmdp_stat(env.handle, L.STAT_CHAIN_FAST_INSTANCES, C.byref(n_fast)))
    if own:
        env.close()
    return vals, ncls, int(n_fast.value)


def _same(x, y):
    return type(x) is type(y) and x == y


def _close(x, want):
    rel = REL32 if isinstance(want, np.float32) else REL64
    return type(x) is type(want) and abs(float(x) - float(want)) <= rel * abs(float(want))


K7_SIZES = [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025]


@gpu
def test_k7_gth_equals_oracle(need_gpu):
    """cmdp_gth on ragged batches of class matrices at the workgroup's size edges (256 threads), sparse, dense and filled by
    the elimination, and one chain whose first state is absorbing (the scale <= 0 early stop)."""
    from colosseum_amd.markov_chain import gth_batch
    from oracle import oracle as O

    mats = []
    for name in ("one_state", "sparse_small", "sparse_mid", "sparse_big", "dense_planned", "dense_unplanned", "in_hub", "periodic"):
        d = H.suite(name)
        mats += [H.policy_chain(d["t"], b, d["acts"][b]) for b in range(d["t"]["B"])]
    d = H.suite("multi_class")   # the closed classes of a reducible chain, as the host path cuts them out
    import colosseum_amd.markov_chain as mc
    for b in (0, 6):
        P = H.policy_chain(d["t"], b, d["acts"][b])
        mats += [P[np.ix_(c, c)] for c in mc.recurrent_classes(P)]
    mats.insert(3, _absorbing_first(70))
    assert set(K7_SIZES) <= {len(m) for m in mats}
    got = gth_batch(mats)
    for m, x in zip(mats, got):
        np.testing.assert_array_equal(x, O.gth(m), err_msg=f"n = {len(m)}")
    assert got[3][0] == 1.0 and not got[3][1:].any()


@gpu
@pytest.mark.parametrize("name", sorted(H.SUITE))
def test_k9_reference_order_is_bit_equal(need_gpu, name):
    """CMDP_OPT_CHAIN_EXACT_ORDER = 1: value, numpy type and class count of every instance equal the reference-order
    reference; K9F takes no part; a masked call returns the same for the selected instances and leaves the others' outputs
    as the call before left them."""
    from colosseum_amd import _lib as L
    from colosseum_amd.batched import BatchedMDP

    d = H.suite(name)
    B = d["t"]["B"]
    env = BatchedMDP(tables=d["t"], with_env=False)
    vals, ncls, n_fast = _run(d, True, env=env)
    assert n_fast == 0
    for b in range(B):
        want, nc = H.suite_reference(name, b)
        print(f"{name}[{b}] S={d['meta'][b]['S']} exact {vals[b]!r} reference {want!r} classes {ncls[b]}/{nc}")
    for b in range(B):
        want, nc = H.suite_reference(name, b)
        assert ncls[b] == nc == d["meta"][b]["n_classes"], (name, b)
        assert type(vals[b]) is type(want) is d["meta"][b]["kind"], (name, b)
        assert vals[b] == want, (name, b, vals[b], want)
    if B >= 2:
        # the unselected instances get another policy: were they evaluated, their outputs would change
        mask = np.arange(B) % 2 == 0
        other = [a if mask[b] else (a + 1) % d["t"]["A"] for b, a in enumerate(d["acts"])]
        vals2, ncls2, _ = _run(d, True, mask=mask, acts=other, env=env)
        assert all(_same(x, y) for x, y in zip(vals2, vals)), (name, vals2, vals)
        np.testing.assert_array_equal(ncls2, ncls)
        full, _, _ = _run(d, True, acts=other, env=env)
        assert any(not _same(full[b], vals[b]) for b in range(B) if not mask[b])
    env.close()


@gpu
@pytest.mark.parametrize("name", sorted(H.SUITE))
def test_default_order_within_the_order_sensitivity(need_gpu, name):
    """Option at 0 (K9 with butterfly sums, K9F where it has a plan and the chain is irreducible): types and class counts
    equal, values within 16 x the measured order sensitivity of GTH of the CPU reference; K9F's instance count where the
    structure decides it."""
    d = H.suite(name)
    B = d["t"]["B"]
    vals, ncls, n_fast = _run(d, False)
    for b in range(B):
        want, nc = H.suite_reference(name, b)
        print(f"{name}[{b}] S={d['meta'][b]['S']} default {vals[b]!r} reference {want!r} "
              f"rel {abs(float(vals[b]) - float(want)) / abs(float(want)):.3e} classes {ncls[b]}/{nc}")
    print(f"{name}: K9F took {n_fast} of {B}")
    for b in range(B):
        want, nc = H.suite_reference(name, b)
        assert ncls[b] == nc, (name, b)
        assert _close(vals[b], want), (name, b, vals[b], want)
    fast = [m["fast"] for m in d["meta"]]
    if None not in fast:
        want_fast = 0 if name == "lds_gap" else sum(fast)   # lds_gap: planned and irreducible, but K9F does not fit LDS
        assert n_fast == want_fast, (name, n_fast, fast)
    assert 0 <= n_fast <= B


@gpu
def test_mixed_batch_masks_and_slow_flags(need_gpu):
    """Planned and unplanned, irreducible and reducible instances in one batch, under a caller's mask: the selected
    instances return the bits of the unmasked call, the others keep their outputs, and the statistic counts the
    masked-out instances plus the selected ones K9F solved (its definition in include/cmdp.h)."""
    from colosseum_amd.batched import BatchedMDP

    d = H.suite("mixed")
    B = d["t"]["B"]
    fast = np.array([m["fast"] for m in d["meta"]], bool)
    assert 0 < fast.sum() < B and [m["S"] for m in d["meta"]].count(1) == 1
    env = BatchedMDP(tables=d["t"], with_env=False)
    vals, ncls, n_fast = _run(d, False, env=env)
    assert n_fast == fast.sum()
    for mask in (np.arange(B) % 2 == 0, np.arange(B) % 2 == 1, ~fast, fast):
        other = [a if mask[b] else (a + 1) % d["t"]["A"] for b, a in enumerate(d["acts"])]
        vals2, ncls2, n2 = _run(d, False, mask=mask, acts=other, env=env)
        assert all(_same(x, y) for x, y in zip(vals2, vals)), (mask, vals2, vals)
        np.testing.assert_array_equal(ncls2, ncls)
        assert n2 == (~mask).sum() + (mask & fast).sum(), (mask, n2)
    env.close()


@gpu
def test_k9_and_k9f_take_turns_on_one_workspace(need_gpu):
    """K9 writes the work matrix as m x m (m = class size), K9F as S x S in elimination positions and clears only the
    entries of the filled graph: alternating a reducible and an irreducible policy on ONE handle must give, call by call,
    the bits a fresh handle gives for that call alone."""
    from colosseum_amd.batched import BatchedMDP

    d = H.suite("reuse")
    assert d["meta"][0]["S"] >= 200 and H.max_row_nnz(d["t"]) <= 4
    multi, irreducible = d["acts"], d["acts2"]
    want_multi, nc_multi = H.suite_reference("reuse", 0)
    want_irr, nc_irr = H.suite_reference("reuse", 0, second=True)
    assert nc_multi == 3 and nc_irr == 1 and type(want_irr) is np.float64
    calls = [(multi, False), (irreducible, False), (multi, False), (irreducible, True), (irreducible, False), (multi, True),
             (irreducible, False)]
    fresh = {}
    for acts, exact in calls:
        key = (acts is multi, exact)
        if key not in fresh:
            fresh[key] = _run(d, exact, acts=acts)
    assert fresh[False, False][2] == 1 and fresh[True, False][2] == 0 and fresh[False, True][2] == 0   # K9F, K9, K9
    assert fresh[True, True][0][0] == want_multi and fresh[False, True][0][0] == want_irr
    assert _close(fresh[True, False][0][0], want_multi) and _close(fresh[False, False][0][0], want_irr)
    env = BatchedMDP(tables=d["t"], with_env=False)
    for k, (acts, exact) in enumerate(calls):
        vals, ncls, n_fast = _run(d, exact, acts=acts, env=env)
        fv, fn, ff = fresh[acts is multi, exact]
        assert _same(vals[0], fv[0]) and ncls[0] == fn[0] and n_fast == ff, (k, vals, fv, n_fast, ff)
    env.close()


@gpu
def test_one_state_more_than_lds_admits_is_refused(need_gpu):
    """S_max + 1 states at 4 entries per row: CMDP_ERR_UNSUPPORTED from the host-side check, in either order, before any
    launch; the handle stays usable for what does not need K9."""
    from colosseum_amd import _lib as L
    from colosseum_amd.batched import BatchedMDP

    d = H.suite("refused")
    assert H.max_row_nnz(d["t"]) == 4 and int(np.diff(d["t"]["state_off"]).max()) == H.S_MAX4 + 1
    assert H.max_row_nnz(H.suite("at_lds_limit")["t"]) == 4
    env = BatchedMDP(tables=d["t"], with_env=False)
    for exact in (0, 1):
        env.set_option(L.OPT_CHAIN_EXACT_ORDER, exact)
        with pytest.raises(L.CmdpError) as e:
            env.average_reward(d["acts"], d["starts"])
        assert e.value.code == L.ERR_UNSUPPORTED
    with pytest.raises(L.CmdpError) as e:
        env.average_reward(d["acts"], [0, H.S_MAX4 + 1])          # argument checks come first
    assert e.value.code == L.ERR_INVALID
    env.close()
