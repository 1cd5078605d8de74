"""Synthetic continuous MDPs whose chain under one deterministic policy has a prescribed structure, for the Markov-chain
kernels K7 (k_gth), K9 (k_chain_average_reward) and K9F (k_chain_fast); host mirrors of the two LDS formulas of
colosseum_amd/csrc/cmdp_chain.h and of K9F's planner, plan_chains (colosseum_amd/csrc/cmdp_chain_plan.h): the minimum-degree
order with its candidate lists, the round schedule and the packing; and the two CPU references
of the average reward: the reference's own bookkeeping (colosseum_amd.markov_chain) over the oracle's GTH, and float64 GTH
in numpy under any elimination order.  Host only: no GPU is touched here."""
import contextlib
import functools
import os
import re

import numpy as np

from helpers_dp_shapes import _row_probs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHAIN_H = os.path.join(ROOT, "colosseum_amd", "csrc", "cmdp_chain.h")

LDS_BUDGET = 160 * 1024   # kLdsBudget
K9F_MAXC = 128            # candidates per pivot a plan may hold
K9F_NW = 16               # wavefronts of k_chain_fast's workgroup
PFB, PF = 4, 8            # K9: 64-entry chunks of a packed column held in registers; chunks a row / column scan prefetches
ABOVE_ONE = np.nextafter(np.float32(1), np.float32(2))   # min(1, v) clamps it


# ---- LDS formulas (cmdp_chain.h) ----------------------------------------------------------------------------------------
def chain_lds_bytes(S, max_deg):
    return 8 * 4 * S + 4 * (12 * S + 1 + S * max_deg)


def chain_fast_lds_bytes(S, max_deg, nw=K9F_NW):
    return 8 * (2 * S + 2 * nw * K9F_MAXC + nw) + 4 * (7 * S + 2 + S * max_deg + 2 * nw * K9F_MAXC + 2 * nw + 16)


def parse_header(path=CHAIN_H):
    """The constants and the two LDS formulas as cmdp_chain.h states them: (dict of constants, chain_lds_bytes,
    chain_fast_lds_bytes), the formulas turned into Python functions from the header's own expressions."""
    src = open(path).read()
    c = dict(K9F_KC=int(re.search(r"#define K9F_KC (\d+)", src).group(1)),
             PFB=int(re.search(r"constexpr int PFB = (\d+);", src).group(1)),
             PF=int(re.search(r"constexpr int PF = (\d+);", src).group(1)))
    assert re.search(r"#define K9F_MAXC \(64 \* K9F_KC\)", src)
    c["K9F_MAXC"] = 64 * c["K9F_KC"]
    hip = open(os.path.join(os.path.dirname(CHAIN_H), "cmdp.hip")).read()   # the launch fixes K9F's wavefront count
    c["NW"] = int(re.search(r"chain_fast_lds_bytes\(h->max_S, h->max_row_nnz, (\d+)\)", hip).group(1))

    def formula(name):
        body = re.search(r"inline size_t %s\(([^)]*)\) \{\s*return (.*?);\s*\}" % name, src, re.S).group(2)
        expr = re.sub(r"\(size_t\)", "", " ".join(body.split()))
        expr = expr.replace("sizeof(double)", "8").replace("sizeof(int)", "4").replace("K9F_MAXC", str(c["K9F_MAXC"]))
        assert re.fullmatch(r"[\sS0-9+*()a-z_]*", expr), expr   # arithmetic over the arguments only
        return expr

    e1, e2 = formula("chain_lds_bytes"), formula("chain_fast_lds_bytes")
    return (c, lambda S, max_deg: eval(e1, {}, dict(S=S, max_deg=max_deg)),
            lambda S, max_deg, nw: eval(e2, {}, dict(S=S, max_deg=max_deg, nw=nw)))


def largest_S(max_deg, bytes_of=chain_lds_bytes, dense=False):
    """Largest S whose K9 fits the budget with `max_deg` entries per row (dense: max_deg = S)."""
    S = 1
    while bytes_of(S + 1, S + 1 if dense else max_deg) <= LDS_BUDGET:
        S += 1
    return S


# ---- the generator ------------------------------------------------------------------------------------------------------
W = 6   # local chords reach this far: the transition graph of a banded structure has bounded bandwidth


def _local(rng, s, S, n, odd=False):
    off = rng.integers(-W, W + 1, size=n)
    if odd:
        off = 2 * (off // 2) + 1
    return {int((s + o) % S) for o in off}


def _ring(rng, lo, n, chords=(1, 3)):
    """Irreducible on lo .. lo + n - 1: a ring and local chords (self-loops included)."""
    out = []
    for i in range(n):
        cols = {lo + (i + 1) % n}
        cols |= {lo + c for c in _local(rng, i, n, int(rng.integers(chords[0], chords[1])))}
        out.append(cols)
    return out


def s_sparse_irreducible(rng, S, **kw):
    return dict(pol=_ring(rng, 0, S), other=lambda s: _local(rng, s, S, int(rng.integers(1, 4))), start=int(rng.integers(S)),
                n_classes=1, kind=np.float64, fast=S >= 2)


def s_dense_irreducible(rng, S, **kw):
    return dict(pol=[set(range(S)) for _ in range(S)], other=lambda s: set(rng.choice(S, int(rng.integers(1, 4)), replace=False).tolist()),
                start=int(rng.integers(S)), n_classes=1, kind=np.float64, fast=S - 1 <= K9F_MAXC, zero_cols=False)


def s_in_hub(rng, S, **kw):
    """Every state has an edge to state 0 (and to state 1 from 600 states), and goes on along the ring; state 0 has a sparse
    row of its own.  The hub edges together carry 0.5 to 3 percent of a row: the ring is the only way up, so the stationary
    mass of state s falls like (1 - hub mass)^s, and with Dirichlet rows it would leave the float64 range long before
    s = 600 (the reference's GTH then returns nan)."""
    hubs = [0, 1] if S >= 600 else [0]
    pol = [set(hubs) | {(s + 1) % S} for s in range(S)]
    pol[0] = {1} | set(rng.choice(np.arange(2, S), 2, replace=False).tolist())

    def probs(s, cols):
        if s == 0 or len(cols) != len(hubs) + 1:
            return None
        h = rng.dirichlet(np.ones(len(hubs))) * rng.uniform(0.005, 0.03)
        p = np.array([h[hubs.index(c)] if c in hubs else 1.0 - h.sum() for c in cols])
        return p.astype(np.float32)

    return dict(pol=pol, other=lambda s: {0, int(rng.integers(S))}, start=int(rng.integers(S)), n_classes=1, kind=np.float64,
                fast=None, probs=probs)


def s_expander(rng, S, **kw):
    cyc = rng.permutation(S)
    succ = np.empty(S, np.int64)
    succ[cyc] = np.roll(cyc, -1)
    pol = [{int(succ[s])} | set(rng.choice(S, 2, replace=False).tolist()) for s in range(S)]
    return dict(pol=pol, other=lambda s: set(rng.choice(S, 2, replace=False).tolist()), start=int(rng.integers(S)),
                n_classes=1, kind=np.float64, fast=None)


def s_periodic(rng, S, **kw):
    assert S % 2 == 0
    pol = [{(s + 1) % S} | _local(rng, s, S, int(rng.integers(1, 3)), odd=True) for s in range(S)]
    return dict(pol=pol, other=lambda s: _local(rng, s, S, int(rng.integers(1, 4))), start=int(rng.integers(S)),
                n_classes=1, kind=np.float64, fast=True, period=2)


def _closed_class(rng, lo, n):
    if n == 1:
        return [{lo}]
    if n == 2:
        return [{lo + 1} | ({lo} if rng.random() < 0.5 else set()), {lo}]
    return _ring(rng, lo, n)


def s_multi_class(rng, S, sizes=(1, 2, 70, 5), start="all", permute=True, **kw):
    """Closed classes of `sizes` at the front, then transient states t_0 .. t_n-1: t_i goes on to t_i+1 and into class
    i mod k, so t_0 reaches every class, t_n-2 two of them (n > k >= 3) and t_n-1 one.  start: "all", "subset", or
    ("in", j) = inside class j.  Labels are then permuted."""
    k, lo, pol = len(sizes), 0, []
    first = []
    for n in sizes:
        first.append(lo)
        pol += _closed_class(rng, lo, n)
        lo += n
    nt = S - lo
    assert nt > k
    for i in range(nt):
        j = i % k
        cols = {first[j] + int(rng.integers(sizes[j]))}
        if i + 1 < nt:
            cols |= {lo + i + 1}
            if rng.random() < 0.3:
                cols |= {lo + int(rng.integers(i + 1, nt))}
        pol.append(cols)
    if start == "all":
        st = lo
    elif start == "subset":
        st = lo + nt - 2
    else:
        st = first[start[1]] + int(rng.integers(sizes[start[1]]))
    return dict(pol=pol, other=lambda s: set(rng.choice(S, int(rng.integers(1, 4))).tolist()), start=st,
                n_classes=k, kind=np.float64, fast=False, perm=rng.permutation(S) if permute else None)


def s_one_class_with_transients(rng, S, **kw):
    n = (3 * S) // 5
    pol = _ring(rng, 0, n)
    for i in range(n, S):
        pol.append({int(rng.integers(n))} | ({i + 1} if i + 1 < S and rng.random() < 0.7 else set()))
    return dict(pol=pol, other=lambda s: set(rng.choice(S, int(rng.integers(1, 4))).tolist()),
                start=int(rng.integers(S)), n_classes=1, kind=np.float32, fast=False, perm=rng.permutation(S))


def s_reuse(rng, S, **kw):
    """Two policies on one banded MDP: `pol` has three closed classes (the large one first) and transient states between
    them, `pol2` is irreducible; every row of every action stays within the band but for the rings' closing edges."""
    big, small = (3 * S) // 4, 2
    d = s_multi_class(rng, S, sizes=(big, small, 1), start=("in", 0), permute=False)
    d["other"] = lambda s: _local(rng, s, S, int(rng.integers(1, 4)))
    d["pol2"] = _ring(rng, 0, S)
    return d


STRUCTURES = dict(sparse_irreducible=s_sparse_irreducible, dense_irreducible=s_dense_irreducible, in_hub=s_in_hub,
                  expander=s_expander, periodic=s_periodic, multi_class=s_multi_class,
                  one_class_with_transients=s_one_class_with_transients, reuse=s_reuse)


def _row(rng, S, cols, zero_col, probs=None):
    """(columns ascending, float32 probabilities) of one row over the successor set `cols`, every one of them with a
    positive probability: Dirichlet, nearly one-hot, or with a 1.2e-7 entry (_row_probs), the dominant entry of some nearly
    one-hot rows a hair above 1; with `zero_col` some rows list one more column with probability exactly 0.
    probs: the structure's own probabilities for this row (or None)."""
    cols = sorted(cols)
    p = _row_probs(rng, len(cols), False) if probs is None else probs
    if len(cols) <= 4 and np.sort(p)[:-1].sum() < 1e-6 and rng.random() < 0.5:   # alone or nearly one-hot
        p[p.argmax()] = ABOVE_ONE
    if zero_col and len(cols) < S and rng.random() < 0.25:
        z = int(rng.integers(S))
        if z not in cols:
            k = int(np.searchsorted(cols, z))
            cols.insert(k, z)
            p = np.insert(p, k, np.float32(0))
    return cols, p


def generate(specs, seed, A=3, wide=None):
    """specs: [(structure, S, options)] -> dict(t = tables for BatchedMDP(tables=..., with_env=False), acts, starts, acts2
    (second policy of the structures that have one, else None), meta = what every instance was built to be).
    The policy's row of state s sits under a random action acts[b][s]; the other actions' rows are drawn apart from it.
    wide = (instance, n): one row of that instance, under an action neither policy takes, lists n columns."""
    rng = np.random.default_rng(seed)
    ptr, col, val, R, acts, acts2, starts, meta = [0], [], [], [], [], [], [], []
    for b, (name, S, opt) in enumerate(specs):
        d = STRUCTURES[name](rng, S, **opt)
        perm = d.pop("perm", None)
        pol, pol2, other = d.pop("pol"), d.pop("pol2", None), d.pop("other")
        zero_col, probs = d.pop("zero_cols", True), d.pop("probs", None)
        inv = np.arange(S) if perm is None else np.argsort(perm)   # new label -> natural label
        lab = np.arange(S) if perm is None else perm                # natural label -> new label
        a1 = rng.integers(A, size=S)
        a2 = (a1 + 1 + rng.integers(A - 1, size=S)) % A
        for s_new in range(S):
            s = int(inv[s_new])
            rows = {}
            for a in sorted(range(A), key=lambda a: (a != a1[s_new], a)):   # the policy's row first: the others keep clear of it
                for attempt in range(50):
                    pp = None
                    if a == a1[s_new]:
                        cols = pol[s]
                        pp = probs(s, sorted(cols)) if probs else None   # in_hub keeps its labels
                    elif pol2 is not None and a == a2[s_new]:
                        cols = pol2[s]
                    elif wide and wide[0] == b and s == S // 2 and a == (a1[s_new] + 1) % A:
                        cols = {(s + o) % S for o in range(1, wide[1] + 1)}
                    else:
                        cols = other(s)
                    cs, p = _row(rng, S, {int(lab[c]) for c in cols}, zero_col and len(cols) <= 3, pp)
                    mine = rows.get(int(a1[s_new]))
                    if mine is None or S == 1 or mine[0] != cs or mine[1].tolist() != p.tolist():
                        break
                else:
                    raise AssertionError("no row apart from the policy's")
                rows[a] = (cs, p)
            for a in range(A):
                cs, p = rows[a]
                col.extend(cs)
                val.extend(p.tolist())
                ptr.append(ptr[-1] + len(cs))
        R.append(rng.random(S * A))
        acts.append(a1.astype(np.int32))
        acts2.append(a2.astype(np.int32) if pol2 is not None else None)
        starts.append(int(lab[d.pop("start")]))
        meta.append(dict(d, name=name, S=S))
    sizes = [s[1] for s in specs]
    t = dict(B=len(specs), A=A, H=0, rewards_range=(0.0, 1.0),
             state_off=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64),
             csr_ptr=np.asarray(ptr, np.int64), csr_col=np.asarray(col, np.int32), csr_val=np.asarray(val, np.float32),
             R=np.concatenate(R).astype(np.float32))
    return dict(t=t, acts=acts, acts2=acts2, starts=starts, meta=meta)


def max_row_nnz(t):
    return int(np.diff(t["csr_ptr"]).max())


# ---- the suite: name -> (specs, seed, A, wide) ----------------------------------------------------------------------------
DENSE_MAX = largest_S(0, dense=True)     # 192: K9 keeps S * max_row_nnz adjacency entries in LDS
S_MAX4 = largest_S(4)                    # 1706: at most 4 entries per row
GAP_S, GAP_NNZ = 600, 40                 # K9 fits, K9F does not (test_lds_gap_size checks it from the formulas)


def _sp(*sizes):
    return [("sparse_irreducible", S, {}) for S in sizes]


SUITE = {
    "sparse_small": (_sp(2, 63, 64, 65), 11, 3, None),
    "one_state": (_sp(1, 1), 12, 2, None),
    "sparse_mid": (_sp(127, 128, 129, 255, 256, 257), 13, 3, None),
    "sparse_big": (_sp(1023, 1024, 1025), 14, 2, None),
    "dense_planned": ([("dense_irreducible", S, {}) for S in (66, 100, 128, 129)], 15, 2, None),
    "dense_unplanned": ([("dense_irreducible", S, {}) for S in (130, 160, DENSE_MAX)], 16, 2, None),
    "in_hub": ([("in_hub", S, {}) for S in (300, 600, 1025)], 17, 2, None),
    "expander": ([("expander", S, {}) for S in (300, 800)], 18, 2, None),
    "periodic": ([("periodic", S, {}) for S in (2, 64, 130, 258)], 19, 3, None),
    "multi_class": ([("multi_class", 100, dict(start="all")), ("multi_class", 100, dict(start="subset")),
                     ("multi_class", 100, dict(start=("in", 0))), ("multi_class", 100, dict(start=("in", 1))),
                     ("multi_class", 100, dict(start=("in", 2))), ("multi_class", 100, dict(start=("in", 3))),
                     ("multi_class", 300, dict(sizes=(130, 1, 1, 2, 65), start="all")),
                     ("multi_class", 90, dict(sizes=(3, 1, 4, 1, 5, 9, 2, 6, 5, 3, 5, 8), start="all")),
                     ("multi_class", 90, dict(sizes=(3, 1, 4, 1, 5, 9, 2, 6, 5, 3, 5, 8), start="subset"))], 20, 3, None),
    "one_class_with_transients": ([("one_class_with_transients", S, {}) for S in (100, 200, 600)], 21, 3, None),
    "mixed": ([("sparse_irreducible", 100, {}), ("dense_irreducible", 140, {}), ("dense_irreducible", 100, {}),
               ("sparse_irreducible", 1, {}), ("multi_class", 90, dict(start="all")), ("one_class_with_transients", 150, {}),
               ("periodic", 66, {})], 22, 3, None),
    "at_lds_limit": (_sp(S_MAX4), 23, 2, None),
    "lds_gap": (_sp(GAP_S), 24, 3, (0, GAP_NNZ)),
    "reuse": ([("reuse", 220, {})], 25, 3, None),
}
REFUSED = (_sp(5, S_MAX4 + 1), 26, 2, None)   # one state more than K9's LDS admits


def two_components():
    """For the planner alone (one action, no policy): a transition graph of two components, a 10-cycle on states 0 .. 9 and
    a triangle on states 10 .. 12, then an instance of 2 states.  Every degree is 2, so the minimum-degree order is the
    index order and the triangle holds the last two positions; it is eliminated in the first two rounds, beside the
    cycle's first pivots: the only lister of the last position, pivot 11, goes eight rounds before the last one."""
    succ = [(s + 1) % 10 for s in range(10)] + [11, 12, 10] + [1, 0]
    n = len(succ)
    t = dict(B=2, A=1, H=0, rewards_range=(0.0, 1.0), state_off=np.array([0, 13, 15], np.int64),
             csr_ptr=np.arange(n + 1, dtype=np.int64), csr_col=np.asarray(succ, np.int32), csr_val=np.ones(n, np.float32),
             R=np.zeros(n, np.float32))
    return dict(t=t, meta=[dict(name="two_components", S=13, fast=None), dict(name="two_components", S=2, fast=None)])


@functools.lru_cache(maxsize=None)
def suite(name):
    if name == "two_components":
        return two_components()
    return generate(*(SUITE[name] if name != "refused" else REFUSED))


def instances():
    """Every (batch name, instance) of the suite."""
    return [(n, b) for n in SUITE for b in range(len(SUITE[n][0]))]


# ---- the chain of a policy ------------------------------------------------------------------------------------------------
def dense_TR(t, b):
    """(T[S, A, S], R[S, A]) float32 of instance b."""
    A, off, ptr = int(t["A"]), t["state_off"], t["csr_ptr"]
    s0, s1 = int(off[b]), int(off[b + 1])
    S = s1 - s0
    T = np.zeros((S * A, S), np.float32)
    lo, hi = ptr[s0 * A], ptr[s1 * A]
    rows = np.repeat(np.arange(S * A), np.diff(ptr[s0 * A: s1 * A + 1]))
    T[rows, t["csr_col"][lo:hi]] = t["csr_val"][lo:hi]
    return T.reshape(S, A, S), t["R"][s0 * A: s1 * A].reshape(S, A)


def policy_chain(t, b, act):
    """float32 chain min(1, T[s, act(s), :]) of a deterministic policy."""
    T, _ = dense_TR(t, b)
    return np.minimum(np.float32(1), T[np.arange(len(act)), act])


def transition_graph(t, b):
    """Adjacency [S, S] of the graph K9F's plan eliminates: the transitions of all actions (positive entries, no
    self-loops), symmetrised."""
    T, _ = dense_TR(t, b)
    g = (T > 0).any(1)
    np.fill_diagonal(g, False)
    return g | g.T


def min_degree_order(t, b, stop=None):
    """The minimum-degree elimination of plan_chains: the live state of lowest degree goes next (ties: the smallest state),
    its neighbours become a clique.  Returns (order = the states in elimination order, per pivot position its candidates:
    the positions of the neighbours it had when it went, ascending, sizes = those lists' lengths as far as the elimination
    got).  stop: give up once a pivot has more candidates than this; the lists are then None."""
    g = transition_graph(t, b)
    S = len(g)
    deg = g.sum(1)
    alive = np.ones(S, bool)
    order, nbs = [], []
    for step in range(S - 1):
        v = int(np.argmin(np.where(alive, deg, S + 1)))
        nb = np.flatnonzero(g[v])
        order.append(v)
        nbs.append(nb)
        if stop is not None and len(nb) > stop:
            return order, None, [len(x) for x in nbs]
        alive[v] = False
        g[np.ix_(nb, nb)] = True
        g[nb, nb] = False
        g[v, :] = False
        g[:, v] = False
        deg[nb] = g[nb].sum(1)
    order.append(int(np.flatnonzero(alive)[0]))
    pos = np.empty(S, np.int64)
    pos[order] = np.arange(S)
    return order, [sorted(pos[nb].tolist()) for nb in nbs] + [[]], [len(x) for x in nbs]


def min_degree_max_candidates(t, b, stop=None):
    """(largest candidate list of a pivot in the minimum-degree elimination, the first pivot's count).  stop: give up above
    this count."""
    sizes = min_degree_order(t, b, stop)[2]
    return max(sizes, default=0), (sizes[0] if sizes else None)


def schedule_rounds(cands, width=K9F_NW):
    """The rounds of K9F's plan as cmdp_chain.h describes them: a pivot may go once every lower pivot that lists it as a
    candidate has gone; of those that may, lowest position first, a round takes up to `width` that share at most one
    candidate with every pivot already in it.  The last position is no pivot.  Returns the rounds as lists of positions."""
    S = len(cands)
    sets = [set(c) for c in cands]
    waiting = np.zeros(S, np.int64)   # lower pivots that list this position and have not gone
    for c in cands:
        waiting[np.asarray(c, np.int64)] += 1
    todo, rounds = set(range(S - 1)), []
    while todo:
        rnd = []
        for p in sorted(x for x in todo if waiting[x] == 0):
            if len(rnd) < width and all(len(sets[p] & sets[q]) <= 1 for q in rnd):
                rnd.append(p)
        for p in rnd:
            todo.remove(p)
            waiting[np.asarray(cands[p], np.int64)] -= 1
        rounds.append(rnd)
    return rounds


def plan_mirror(t):
    """The eight arrays of plan_chains for the batch `t`, from the two mirrors above and ChainFast's layout (cmdp_chain.h):
    cptr of instance b at state_off[b] + b, rank and piv at state_off[b], cbase / rbase the starts of its blocks in cand /
    rptr; an instance without a plan (fewer than 2 states, a pivot with more than K9F_MAXC candidates) takes no room."""
    off, B = t["state_off"], int(t["B"])
    NS = int(off[-1])
    p = dict(rank=np.full(NS, -1, np.int32), cptr=np.zeros(NS + B, np.int32), cbase=np.zeros(B, np.int64), cand=[],
             nrounds=np.full(B, -1, np.int32), rbase=np.zeros(B, np.int64), rptr=[], piv=np.zeros(NS, np.int32))
    for b in range(B):
        so, S = int(off[b]), int(off[b + 1] - off[b])
        p["cbase"][b], p["rbase"][b] = len(p["cand"]), len(p["rptr"])
        if S < 2:
            continue
        order, cands, _ = min_degree_order(t, b, stop=K9F_MAXC)
        if cands is None:
            continue
        rounds = schedule_rounds(cands)
        p["nrounds"][b] = len(rounds)
        p["rank"][so + np.asarray(order)] = np.arange(S)
        p["cptr"][so + b: so + b + S + 1] = np.concatenate([[0], np.cumsum([len(c) for c in cands])])
        p["cand"] += [x for c in cands for x in c]
        p["piv"][so: so + S - 1] = [x for r in rounds for x in r]
        p["rptr"] += np.concatenate([[0], np.cumsum([len(r) for r in rounds])]).tolist()
    p["cand"] = np.asarray(p["cand"], np.uint16)
    p["rptr"] = np.asarray(p["rptr"], np.int32)
    return p


# ---- references -----------------------------------------------------------------------------------------------------------
def gth_numpy(P, order=None, stats=None):
    """Stationary distribution by GTH elimination in float64, the sums serial in index order (cumsum), products and sums
    rounded separately, exactly as the reference's numba routine and the oracle do it.  The diagonal is never read: the
    chain solved has P[i, i] = 1 - the off-diagonal sum of its row.  Products with a zero factor are skipped (adding them
    is exact).  order: eliminate the states in this order instead.  stats: dict that receives `max_col`, the most
    non-zeros any pivot's column holds below the diagonal."""
    a = np.array(P, np.float64)
    n = len(a)
    if order is not None:
        a = a[np.ix_(order, order)]
    nn = n
    max_col = 0
    for i in range(n - 1):
        row = a[i, i + 1:]
        scale = np.cumsum(row)[-1]
        if scale <= 0.0:
            nn = i + 1
            break
        a[i + 1:, i] /= scale
        rj = np.flatnonzero(a[i + 1:, i]) + i + 1
        ck = np.flatnonzero(row) + i + 1
        max_col = max(max_col, len(rj))
        if 2 * len(rj) * len(ck) > (n - i - 1) ** 2:
            a[i + 1:, i + 1:] += np.outer(a[i + 1:, i], row)
        elif len(rj) and len(ck):
            a[np.ix_(rj, ck)] += np.outer(a[rj, i], a[i, ck])
    x = np.zeros(n)
    x[nn - 1] = 1.0
    for i in range(nn - 2, -1, -1):
        x[i] = np.cumsum(x[i + 1: nn] * a[i + 1: nn, i])[-1]
    x[:nn] /= np.cumsum(x[:nn])[-1]
    if stats is not None:
        stats["max_col"] = max_col
    if order is not None:
        out = np.zeros(n)
        out[order] = x
        return out
    return x


ORDERS = ("index", "reverse", "random1", "random2")


def ordered_gth(kind):
    """GTH of a class matrix under one of the four elimination orders of the order-sensitivity measurement."""
    def solve(P):
        n = len(P)
        if kind == "index":
            return gth_numpy(P)
        order = np.arange(n)[::-1] if kind == "reverse" else np.random.default_rng(n + (7 if kind == "random1" else 77)).permutation(n)
        return gth_numpy(P, order)
    return solve


@contextlib.contextmanager
def _host_gth(solve):
    import colosseum_amd.markov_chain as mc

    keep = mc.gth_batch
    mc.gth_batch = lambda mats: [solve(np.asarray(m, np.float64)) for m in mats]
    try:
        yield mc
    finally:
        mc.gth_batch = keep


def reference(t, b, act, start, solve=None):
    """(average reward typed as the reference types it, number of recurrent classes): colosseum_amd.markov_chain's
    `get_average_reward` / `recurrent_classes` (pinned to the reference's outputs by tests/test_oracle_pinned.py) with the
    device GTH replaced by `solve` (default: the oracle's GTH).  CPU only."""
    from oracle import oracle as O

    T, R = dense_TR(t, b)
    S, A = R.shape
    pol = np.zeros((S, A), np.float32)
    pol[np.arange(S), act] = 1
    with _host_gth(solve or O.gth) as mc:
        value = mc.get_average_reward(T, R, pol, [(int(start), 1.0)])
        classes = mc.recurrent_classes(mc.get_transition_probabilities(T, pol))
    return value, classes


@functools.lru_cache(maxsize=None)
def suite_reference(name, b, second=False):
    d = suite(name)
    value, classes = reference(d["t"], b, (d["acts2"] if second else d["acts"])[b], d["starts"][b])
    return value, len(classes)
