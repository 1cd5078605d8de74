"""Generated episodic MDPs for the finite-horizon kernels -- K4 `k_episodic<DP_VI | DP_PE>` (backward induction), K5E
`k_diam_episodic` (the episodic diameter on the time-augmented state space) and K6 `k_value_norm` --, per-instance calls of
the C oracle on raw arrays, float64 references with the tolerance a float32 evaluation has to meet against them, and one
checker per kernel that compares every element of every instance.  Host only: no GPU is touched here.

Generator, CSR slicing, policies and row probabilities are those of helpers_dp_shapes; the sparse float64 matrix and the
shape of `admissible` those of helpers_diam."""
import functools

import numpy as np

import helpers_diam as D
import helpers_dp_shapes as H

EPS = 1e-3                 # the reference's stopping threshold of the episodic diameter
U2 = 2.0 ** -23            # twice the unit roundoff of float32: every bound below is written with it (see episodic_f64)
LDS_BUDGET = H.LDS_BUDGET  # kLdsBudget
K4_MAX_S = LDS_BUDGET // 8                     # 2 * 4 * max_S <= 160 KiB
START_WEIGHTS = {1: [1.0], 2: [0.3, 0.7], 3: [0.2, 0.3, 0.5]}   # float32 on the way in: none of them dyadic but 1


def k5e_fits(Hh, max_S):
    """The LDS rule of cmdp_diameter_episodic: 4 * H * max_S <= 160 KiB - 1024."""
    return 4 * Hh * max_S <= LDS_BUDGET - 1024


# ---- the generator -----------------------------------------------------------------------------------------------------
def reach_layers(S, A, csr, start_state, Hh):
    """(reach[H - 1][S], within[S]): reach[h][j] says that row (h, j) of the time-augmented transition tensor is filled
    -- layer 0 the starting states, layer h <= H - 2 every column a filled row of layer h - 1 lists, explicit zeros
    included (`cmdp_diameter_episodic`, `oracle_episodic_reach`) --, within[j] that state j is a starting state or listed
    by a filled row, i.e. reached within H - 1 transitions."""
    from scipy.sparse import csr_matrix

    ptr, col, _ = csr
    G = csr_matrix((np.ones(len(col)), np.asarray(col, np.int64), np.asarray(ptr, np.int64)), shape=(S * A, S))
    reach = np.zeros((Hh - 1, S), bool)
    reach[0, np.asarray(start_state, np.int64)] = True
    for h in range(1, Hh - 1):
        reach[h] = (G.T @ np.repeat(reach[h - 1], A).astype(np.float64)) > 0
    within = reach.any(0) | ((G.T @ np.repeat(reach[Hh - 2], A).astype(np.float64)) > 0)
    return reach, within


def generate_episodic(A, sizes, nnz, Hh, seed, zeros=False, rewards="unit", unsorted_row=False, k5e=True):
    """(tables, starts): tables for BatchedMDP(tables=..., with_env=False) with H = Hh, and starts = (start_off int64 [B + 1],
    start_state int32, start_prob float32) per instance.

    Rows are those of helpers_dp_shapes.generate (ascending columns, 1 .. nnz entries and one row of exactly nnz, explicit
    zeros on request, near-one-hot rows) with a backbone laid over them: under action a < 2 state s lists the successor
    (2 s + 1 + a) mod S -- in place of a randomly drawn entry where the row did not list it -- with probability at least
    0.8: the peak of a near-one-hot row is moved onto it, any other row is scaled by 0.2 and the entry given 0.8 more.
    The backbone is a binary heap, so every state lies within ceil(log2 S) + 1 transitions of state 0.
    rewards: "unit" U[0, 1), "neg" U[-1, 0), "sym" U[-1, 1).  unsorted_row reverses the last row of two or more entries.
    State 0 is a starting state of every instance; instance b has min(3 - b % 3, S - 1) of them (one where S <= 2), the
    others drawn at random, in random order, with the weights 1 | 0.3, 0.7 | 0.2, 0.3, 0.5.

    Asserted per instance by a layered search (k5e=False leaves it out: a batch K5E never sees, whose horizon is shorter
    than its backbone is deep): every state is reached from a starting state within H - 1 transitions; where S > 2 some
    rows (h, j), h <= H - 2, are filled and some are not.  Asserted always: every backbone entry has at least 0.8, and the
    batch's largest row has exactly nnz entries."""
    t = H.generate(A, sizes, nnz, min(A * nnz, nnz + 2), seed, zeros=zeros, rewards="neg" if rewards == "neg" else "unit")
    rng = np.random.default_rng(seed + 7919)
    ptr, col, val, off = t["csr_ptr"], t["csr_col"], t["csr_val"], t["state_off"]
    for b, S in enumerate(sizes):
        for s in range(S):
            for a in range(min(A, 2)):
                r = (int(off[b]) + s) * A + a
                lo, hi = int(ptr[r]), int(ptr[r + 1])
                c = (2 * s + 1 + a) % S
                cols, p = col[lo:hi], val[lo:hi].astype(np.float64)
                if c not in cols:
                    cols[int(rng.integers(hi - lo))] = c
                    order = np.argsort(cols)
                    cols[:], p = cols[order], p[order]
                i, peak = int(np.flatnonzero(cols == c)[0]), int(p.argmax())
                if p[peak] > 0.99:
                    p[[i, peak]] = p[[peak, i]]
                else:
                    p = 0.2 * p
                    p[i] += 0.8
                val[lo:hi] = p.astype(np.float32)
    if unsorted_row:
        r = int(np.flatnonzero(np.diff(ptr) >= 2)[-1])
        col[ptr[r]:ptr[r + 1]] = col[ptr[r]:ptr[r + 1]][::-1].copy()
        val[ptr[r]:ptr[r + 1]] = val[ptr[r]:ptr[r + 1]][::-1].copy()
    if rewards == "sym":
        t["R"] = rng.uniform(-1.0, 1.0, len(t["R"])).astype(np.float32)
        t["rewards_range"] = (-1.0, 1.0)
    t["H"] = int(Hh)
    soff, sst, sp = [0], [], []
    for b, S in enumerate(sizes):
        n = min(3 - b % 3, max(1, S - 1))
        st = np.concatenate([[0], rng.choice(np.arange(1, S), n - 1, replace=False)]) if n > 1 else np.zeros(1, np.int64)
        sst.extend(rng.permutation(st).tolist())
        sp.extend(START_WEIGHTS[n])
        soff.append(soff[-1] + n)
    starts = (np.asarray(soff, np.int64), np.asarray(sst, np.int32), np.asarray(sp, np.float32))
    assert int(np.diff(ptr).max()) == nnz and int(np.diff(ptr).min()) >= 1
    for b, S in enumerate(sizes):
        _, _, csr, _ = H.instance(t, b)
        st = instance_starts(starts, b)[0]
        assert 0 in st and len(set(st.tolist())) == len(st)
        if k5e:
            reach, within = reach_layers(S, A, csr, st, Hh)
            assert within.all(), (b, "a state is not reached within H - 1 transitions")
            assert S <= 2 or (reach.any() and not reach.all()), (b, "the reach mask is all of one kind")
        lp, c, v = csr
        for a in range(min(A, 2)):
            rows = np.arange(S) * A + a
            want = (2 * np.arange(S) + 1 + a) % S
            for s in range(S):
                e = slice(int(lp[rows[s]]), int(lp[rows[s] + 1]))
                assert v[e][c[e] == want[s]].sum() >= np.float32(0.8), (b, s, a)
    return t, starts


def instance_starts(starts, b):
    """(start states, float32 weights) of instance b."""
    soff, sst, sp = starts
    return sst[int(soff[b]):int(soff[b + 1])], sp[int(soff[b]):int(soff[b + 1])]


# name -> arguments of generate_episodic; sizes ragged, no batch size a multiple of anything
SPECS = {
    "small": dict(A=2, sizes=[5, 1, 64, 3, 65], nnz=3, Hh=7, seed=1),
    # S = 257 and 300 above 256, S = 63 below 64 with S * A = 189 below 256, S = 2
    "stride": dict(A=3, sizes=[257, 2, 300, 63], nnz=4, Hh=11, seed=2, zeros=True, rewards="sym"),
    "A5nnz9": dict(A=5, sizes=[70, 1, 9], nnz=9, Hh=9, seed=3, rewards="neg", unsorted_row=True),   # K4 and K6 only
    "h2": dict(A=2, sizes=[3, 1, 2], nnz=3, Hh=2, seed=4),            # every state a successor of a starting state
    "restart": dict(A=2, sizes=[300, 40], nnz=3, Hh=10, seed=5),      # the backbone is 8 deep: episodes often end without a hit
    "k4_edge": dict(A=2, sizes=[K4_MAX_S, 7], nnz=2, Hh=3, seed=6, k5e=False),   # 2 * 4 * 20480 = 160 KiB; K4 only
    "k5e_edge": dict(A=2, sizes=[318, 5], nnz=3, Hh=128, seed=7),     # 4 * 128 * 318 = 160 KiB - 1024
}
K4_BATCHES = ("small", "stride", "A5nnz9")
K5E_BATCHES = ("small", "stride", "h2", "restart", "k5e_edge")


@functools.lru_cache(maxsize=None)
def batch(name):
    """(tables, starts) of a named batch, generated once per process; nobody writes into them."""
    return generate_episodic(**SPECS[name])


def with_largest(name, S):
    """The named batch with its first (largest) instance generated at S states instead."""
    spec = dict(SPECS[name])
    spec["sizes"] = [S] + spec["sizes"][1:]
    return generate_episodic(**spec)


def layer_policies(t, Hh, kind, seed):
    """One float32 policy [H, S_b, A] per instance, every layer and instance drawn on its own."""
    per_layer = [H.policies(t, kind, seed + 1000 * h) for h in range(Hh)]
    return [np.stack([per_layer[h][b] for h in range(Hh)]) for b in range(int(t["B"]))]


def random_values(t, seed):
    """A flat float32 V of mixed signs and magnitudes 0.1 .. 1e3: no value-iteration result."""
    rng = np.random.default_rng(seed)
    n = int(t["state_off"][-1])
    return (rng.uniform(-1.0, 1.0, n) * 10.0 ** rng.uniform(-1.0, 3.0, n)).astype(np.float32)


# ---- the C oracle, instance by instance on raw arrays ---------------------------------------------------------------------
def oracle_k4(t, Hh, pis=None, R=None):
    """[(Q[H + 1, S, A], V[H + 1, S])] per instance; pis per-instance [H, S, A] or None (the maximum), R a flat override."""
    from oracle import oracle as O

    out = []
    for b in range(int(t["B"])):
        S, A, csr, Rb = H.instance(t, b)
        if R is not None:
            Rb = np.asarray(R, np.float32)[int(t["state_off"][b]) * A: int(t["state_off"][b + 1]) * A]
        out.append(O.episodic(S, A, Hh, csr, Rb, None if pis is None else pis[b]))
    return out


def oracle_k6(t, V):
    from oracle import oracle as O

    off = t["state_off"]
    return [np.float32(O.value_norm(*H.instance(t, b)[:3], V[int(off[b]):int(off[b + 1])])) for b in range(int(t["B"]))]


def oracle_k5e(t, starts, Hh=None, eps=EPS, max_sweeps=1_000_000):
    """[(diameter float32, per_target, return code)] per instance, every target run to diff < eps (use_running_max = 0)."""
    from oracle import oracle as O

    Hh = int(t["H"]) if Hh is None else Hh
    out = []
    for b in range(int(t["B"])):
        S, A, csr, _ = H.instance(t, b)
        d, per, rc = O.diameter_episodic_csr(S, A, Hh, csr, *instance_starts(starts, b), eps, False, max_sweeps)
        out.append((np.float32(d), per, rc))
    return out


# ---- float64 references --------------------------------------------------------------------------------------------------
def episodic_f64(S, A, Hh, csr, R, pi=None):
    """Backward induction in float64 on the float32-valued tables: (Q[H + 1, S, A], V[H + 1, S], bq[H + 1], bv[H + 1]) with
    bq[h] / bv[h] the largest |Q~_h - Q_h| / |V~_h - V_h| a float32 evaluation in the kernel's operation order may show.

    `backup_state<MODE, true, false, true>` with gamma = 1 computes, for a row of k <= K entries,
        acc = fl(sum_j fl(p_j v_j))     k products, k - 1 sums (the first sum, to 0, is exact; the product by gamma = 1 too)
        q   = fl(R + acc)               one sum
        VI: v = max_a q (exact)         PE: v = fl(sum_a fl(q_a pi_a)), A products and A - 1 sums in action order.
    With the unit roundoff u = 2^-24 and float32 inputs v~ of layer h + 1 within bv[h + 1] of the float64 ones,
        |acc~ - acc| <= k u sum_j p_j |v~_j| + sum_j p_j |v~_j - v_j| <= k u s m + s bv[h + 1],
    where s = sum_j p_j <= 1 + K u (float32 probabilities of a row that sums to 1) and
    m = bv[h + 1] + max(max|V_h+1|, max|Q_h|) bounds every float32 operand; the sum with R adds u |q~| <= u (1 + ..) m.
    So |Q~_h - Q_h| <= bv[h + 1] + (k + 1) u m + terms of second order, and every such term (K u bv, u^2 m, ...) is covered
    by writing 2^-23 for u and K + 2 for k + 1, as helpers_dp_shapes.f64_bound does:
        bq[h] = bv[h + 1] + (K + 2) 2^-23 m.
    The maximum over actions is non-expansive: bv[h] = bq[h] for VI.  For PE the A products and A - 1 sums of non-negative
    weights that sum to 1 within A u add A u max|q~|: bv[h] = bq[h] + A 2^-23 m.  Layer H is exactly zero: bq[H] = bv[H] = 0,
    and the bounds accumulate over the H layers below it."""
    P = D._sparse_P(S, A, csr)
    K = int(np.diff(csr[0]).max())
    R64 = np.asarray(R, np.float32).astype(np.float64).reshape(S, A)
    Q, V = np.zeros((Hh + 1, S, A)), np.zeros((Hh + 1, S))
    bq, bv = np.zeros(Hh + 1), np.zeros(Hh + 1)
    if pi is not None:
        pi = np.asarray(pi, np.float32).astype(np.float64).reshape(Hh, S, A)
    for h in range(Hh - 1, -1, -1):
        Q[h] = R64 + (P @ V[h + 1]).reshape(S, A)
        V[h] = Q[h].max(1) if pi is None else (Q[h] * pi[h]).sum(1)
        m = bv[h + 1] + max(np.abs(V[h + 1]).max(), np.abs(Q[h]).max())
        bq[h] = bv[h + 1] + (K + 2) * U2 * m
        bv[h] = bq[h] + (A * U2 * m if pi is not None else 0.0)
    return Q, V, bq, bv


def value_norm_f64(S, A, csr, V):
    """(norm, lo, hi): max_{i,a} sqrt(sum_j P[i,a,j] (V[j] - Ev[j,a])^2), Ev = P V, in float64 on the float32 tables and V,
    and the interval a float32 evaluation in the kernel's operation order lies in.

    k_value_norm computes, with rows of at most K entries and u = 2^-24,
        Ev~[j,a] = fl(sum_k fl(p_k V_k))                 K products, K - 1 sums: |Ev~ - Ev| <= K u s max|V| =: e_Ev
        d~_j     = fl(V_j - Ev~[j,a])                    |d~_j - d_j| <= e_Ev + u |d~_j| =: e_j
        x~       = fl(sum_j fl(p_j fl(d~_j d~_j)))       two products per entry, k - 1 sums:
                   |x~ - x| <= sum_j p_j e_j (2 |d_j| + e_j) + (k + 2) u sum_j p_j d~_j^2 =: delta      (x = sum_j p_j d_j^2)
        n~       = fl(sqrt(x~))                          correctly rounded: n~ in [sqrt(x - delta) (1 - u), sqrt(x + delta) (1 + u)]
    (s = sum p <= 1 + K u and the other second-order terms are covered by writing 2^-23 for u throughout, as in
    episodic_f64, and |d~_j| <= |d_j| + e_j).  The square root is not Lipschitz at 0, so the bound is an interval, not a
    distance; the maximum over the rows is monotone, so the result lies in [max lo_r, max hi_r]."""
    ptr, col, val = csr
    P = D._sparse_P(S, A, csr)
    K = int(np.diff(ptr).max())
    V64 = np.asarray(V, np.float32).astype(np.float64)
    Ev = (P @ V64).reshape(S, A)
    rows = np.repeat(np.arange(S * A), np.diff(ptr))
    p = np.asarray(val, np.float64)
    d = V64[col] - Ev[col, rows % A]
    x = np.bincount(rows, p * d * d, S * A)
    e = K * U2 * np.abs(V64).max() + U2 * np.abs(d)
    delta = np.bincount(rows, p * e * (2 * np.abs(d) + e), S * A) + (K + 2) * U2 * np.bincount(rows, p * (np.abs(d) + e) ** 2, S * A)
    lo = np.sqrt(np.maximum(x - delta, 0.0)) * (1 - U2)
    hi = np.sqrt(x + delta) * (1 + U2)
    return float(np.sqrt(x).max()), float(lo.max()), float(hi.max())


def episodic_diameter_f64(S, A, Hh, csr, start_state, start_prob, eps=EPS, max_sweeps=5000, stop=0.5):
    """The sweep of `_episodic_diameter_calculation` in float64, all S targets side by side (ETs[H, S, target]) and in the
    reference's update order: layer H - 1 from the start row (every state, the target too), then layers H - 2 .. 0 in
    place, layer h - 1 from this sweep's layer h, the target's own entry skipped, unfilled rows 0, an entry of the target's
    column counted with 1 + 0.  Returns the trajectory as arrays [n, targets]: diff (max |ETs_n - ETs_n-1|), r (cur_diam =
    max_s min_{h: ETs > 0} ETs[h, s]) and vabs (max ETs) after every sweep, until every target has diff < stop * eps."""
    P = D._sparse_P(S, A, csr)
    reach = reach_layers(S, A, csr, start_state, Hh)[0]
    st = np.asarray(start_state, np.int64)
    sp = np.asarray(start_prob, np.float32).astype(np.float64)
    tg = np.arange(S)
    E = np.zeros((Hh, S, S))
    diff, r, vabs = [], [], []
    for _ in range(int(max_sweeps)):
        last = sp @ (1.0 + E[0][st])
        dmax = np.abs(E[Hh - 1] - last).max(0)
        E[Hh - 1][:] = last
        for h in range(Hh - 1, 0, -1):
            X = 1.0 + E[h]
            X[tg, tg] = 1.0
            new = np.where(reach[h - 1][:, None], (P @ X).reshape(S, A, S).min(1), 0.0)
            new[tg, tg] = E[h - 1][tg, tg]
            dmax = np.maximum(dmax, np.abs(new - E[h - 1]).max(0))
            E[h - 1] = new
        diff.append(dmax)
        r.append(np.where(E > 0, E, np.inf).min(0).max(0))
        vabs.append(E.max((0, 1)))
        if (dmax < stop * eps).all():
            break
    return dict(diff=np.array(diff), r=np.array(r), vabs=np.array(vabs))


def admissible_episodic(traj, eps, K, Hh):
    """helpers_diam.admissible for ONE target of the episodic sweep: [(sweep, lo, hi)] for every sweep a correct float32
    solve may stop at, with the interval its result then lies in.  No number in it is chosen.

    One backup -- ETs[h - 1, j] = min_a (p_es + sum_{c != es} p_c (1 + ETs[h, c])), and the start row of the same form --
    is, for a row of k <= K entries (K the larger of the longest row and the number of starting states), k sums 1 + ETs, k
    products, k - 1 sums and the sum with p_es, all of non-negative terms: evaluated in float32 it departs from the exact
    backup of the same operands by at most (k + 2) u (1 + max ETs) s, s = sum p <= 1 + K u, covered by
        d_n = (K + 2) 2^-23 (1 + max_{j <= n} max ETs_j)      (2^-23 for u = 2^-24, as in episodic_f64).
    The backup is a minimum of averages, hence non-expansive; but within a sweep layer h - 1 reads THIS sweep's layer h,
    so the error of layer H - 1 (one backup of the previous sweep's layer 0) is handed down and grows by d_n per layer:
    after sweep n the float32 and float64 iterates are within E_n = E_n-1 + H d_n = H sum_{j <= n} d_j in every layer.
    The stopping values diff_n = max |ETs_n - ETs_n-1| are then within 2 E_n of each other, the float32 subtraction
    adding a relative u: the float32 solve stops at its first sweep with diff < eps, so its stopping sweep m has
        diff64_m < eps (1 + 2^-23) + 2 E_m      and      no j < m with diff64_j < eps (1 - 2^-23) - 2 E_j.
    cur_diam is a maximum of minima over the positive entries, and an entry is positive in float32 exactly where it is in
    float64 (a filled row sums to at least its probabilities, about 1; every other entry is an exact 0), so the result lies
    in [r64_m - E_m, r64_m + E_m].  Where 2 E_j reaches eps first, every sweep up to the end of the trajectory (diff64 <
    eps / 2) is a candidate, which only narrows what passes."""
    diff, r, vabs = (np.asarray(traj[k], np.float64) for k in ("diff", "r", "vabs"))
    d = (K + 2) * U2 * (1.0 + np.maximum.accumulate(vabs))
    E = Hh * np.cumsum(d)
    sure = np.flatnonzero(diff < eps * (1 - U2) - 2 * E)
    last = int(sure[0]) if len(sure) else len(diff) - 1
    return [(m + 1, r[m] - E[m], r[m] + E[m]) for m in range(last + 1) if diff[m] < eps * (1 + U2) + 2 * E[m]]


SWEEPS64 = {}   # batch -> largest number of float64 sweeps a target needs to its first diff < eps


@functools.lru_cache(maxsize=None)
def reference_k5e(name):
    """Per instance of a named batch: (final float64 value per target, [admissible (sweep, lo, hi) list per target])."""
    t, starts = batch(name)
    Hh, out = int(t["H"]), []
    for b in range(int(t["B"])):
        S, A, csr, _ = H.instance(t, b)
        st, sp = instance_starts(starts, b)
        traj = episodic_diameter_f64(S, A, Hh, csr, st, sp)
        assert (traj["diff"][-1] < EPS).all(), (name, b, "a target needs more than 5000 float64 sweeps")
        SWEEPS64[name] = max(SWEEPS64.get(name, 0), int((traj["diff"] >= EPS).sum(0).max()) + 1)
        K = max(int(np.diff(t["csr_ptr"]).max()), len(st))
        out.append((traj["r"][-1], [admissible_episodic({k: v[:, j] for k, v in traj.items()}, EPS, K, Hh) for j in range(S)]))
    if name == "restart":   # the return to the start distribution carries weight: many targets take longer than an episode
        assert (out[0][0] > Hh).mean() >= 0.25, float((out[0][0] > Hh).mean())
    return out


# ---- the checkers: every element of every instance, the worst error / bound returned and not asserted -----------------------
def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def split(t, flat, b, lead, rows):
    """Instance b's part of a flat result of `lead` layers, per row (rows=True) or per state."""
    off = t["state_off"] * (int(t["A"]) if rows else 1)
    return flat[lead * int(off[b]): lead * int(off[b + 1])]


def reference_k4(t, Hh, pis=None, R=None):
    """Per instance: (oracle Q, oracle V, float64 Q, float64 V, bq, bv) at horizon Hh."""
    orc = oracle_k4(t, Hh, pis, R)
    out = []
    for b in range(int(t["B"])):
        S, A, csr, Rb = H.instance(t, b)
        if R is not None:
            Rb = split(t, np.asarray(R, np.float32), b, 1, True)
        out.append(orc[b] + episodic_f64(S, A, Hh, csr, Rb, None if pis is None else pis[b]))
    return out


def check_k4(t, Hh, Q, V, ref, parts=("oracle", "f64")):
    """Flat Q [(H + 1) S A per instance] and V [(H + 1) S] against `ref` (reference_k4): bit-equal to the oracle, within
    bq[h] / bv[h] of float64 in every layer, layer H exactly zero.  Returns the worst error / bound."""
    assert len(Q) == (Hh + 1) * int(t["state_off"][-1]) * int(t["A"]) and len(V) == (Hh + 1) * int(t["state_off"][-1])
    worst = 0.0
    for b, (oQ, oV, Q64, V64, bq, bv) in enumerate(ref):
        S, A = V64.shape[1], Q64.shape[2]
        q = split(t, Q, b, Hh + 1, True).reshape(Hh + 1, S, A)
        v = split(t, V, b, Hh + 1, False).reshape(Hh + 1, S)
        if "oracle" in parts:
            assert np.array_equal(_bits(q), _bits(oQ)), ("Q differs from the oracle", b, np.argwhere(_bits(q) != _bits(oQ))[:3])
            assert np.array_equal(_bits(v), _bits(oV)), ("V differs from the oracle", b, np.argwhere(_bits(v) != _bits(oV))[:3])
        if "f64" in parts:
            assert not _bits(q[Hh]).any() and not _bits(v[Hh]).any(), ("layer H is not zero", b)
            for h in range(Hh):
                eq, ev = np.abs(q[h] - Q64[h]).max(), np.abs(v[h] - V64[h]).max()
                assert eq <= bq[h], ("Q outside its float64 bound", b, h, eq, bq[h])
                assert ev <= bv[h], ("V outside its float64 bound", b, h, ev, bv[h])
                worst = max(worst, eq / bq[h], ev / bv[h])
    return worst


def reference_k6(t, V):
    """Per instance: (oracle value, float64 value, lo, hi)."""
    orc = oracle_k6(t, V)
    return [(orc[b],) + value_norm_f64(*H.instance(t, b)[:3], split(t, V, b, 1, False)) for b in range(int(t["B"]))]


def check_k6(t, out, ref, parts=("oracle", "f64")):
    assert len(out) == int(t["B"])
    worst = 0.0
    for b, (o, n64, lo, hi) in enumerate(ref):
        got = np.float32(out[b])
        if "oracle" in parts:
            assert _bits(got) == _bits(o), ("value norm differs from the oracle", b, got, o)
        if "f64" in parts:
            assert lo <= float(got) <= hi, ("value norm outside its float64 interval", b, float(got), lo, hi)
            room = (hi - n64) if got >= n64 else (n64 - lo)
            worst = max(worst, abs(float(got) - n64) / room if room > 0 else 0.0)
    return worst


@functools.lru_cache(maxsize=None)
def oracle_k5e_named(name):
    return oracle_k5e(*batch(name))


def check_k5e(name, per, diam, parts=("oracle", "f64")):
    """per_target (flat) and diameter [B] of a named batch: per_target bit-equal to the oracle's, diameter the float32
    maximum of the instance's per_target, every value in an admissible interval.  Returns (the worst distance to the
    centre of the nearest admissible interval over that interval's half width, the largest union of intervals relative to
    the value (or to 1), the largest float64 sweep count)."""
    t, _ = batch(name)
    assert len(per) == int(t["state_off"][-1]) and len(diam) == int(t["B"])
    worst = width = 0.0
    for b in range(int(t["B"])):
        p = split(t, per, b, 1, False)
        assert _bits(np.float32(diam[b])) == _bits(p.max()), ("diameter is not the maximum of per_target", b)
        if "oracle" in parts:
            od, operr, rc = oracle_k5e_named(name)[b]
            assert rc == 0
            assert np.array_equal(_bits(p), _bits(operr)), ("per_target differs from the oracle", b, np.flatnonzero(_bits(p) != _bits(operr))[:5])
            assert _bits(np.float32(diam[b])) == _bits(od)
        if "f64" in parts:
            for j, iv in enumerate(reference_k5e(name)[b][1]):
                v = float(p[j])
                assert any(lo <= v <= hi for _, lo, hi in iv), ("outside every admissible interval", name, b, j, v, iv[:3])
                worst = max(worst, min(abs(v - (lo + hi) / 2) / ((hi - lo) / 2) for _, lo, hi in iv))
                width = max(width, (max(hi for _, _, hi in iv) - min(lo for _, lo, _ in iv)) / max((iv[0][1] + iv[0][2]) / 2, 1.0))
    return worst, width, SWEEPS64.get(name, 0)
