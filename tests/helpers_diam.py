"""Generated communicating MDPs for the continuous-diameter kernels (K2 / K3 in DIAM mode, K5S, K5T, K5C, K5D), float64
references of the per-target solves, the tolerance a float32 solve has to meet against them, and a host mirror of which
diameter kernel `pick_diameter_path` / `pick_diameter_cluster` / `pick_diameter_lanes` (colosseum_amd/csrc/cmdp_dp_plan.h)
choose for `cmdp_diameter` / `diameter_lanes` and of the launches `DiamGroups` (cmdp.hip) packs.  Host only: no GPU is touched."""
import functools
import re

import numpy as np

import helpers_dp_shapes as H

DP_PLAN_H = H.DP_PLAN_H
CUS = 256                 # compute units of the MI355X: the K5S width rule and the K5C grid depend on them, and the
                          # many-group batches are sized by them (on another part the statistic check says so and fails)
LDS_BUDGET = H.LDS_BUDGET
EPS = 1e-3

# ---- the compiled fixed-width shapes -----------------------------------------------------------------------------------
SHAPES = [(2, 2), (2, 4), (2, 8), (3, 2), (3, 4), (3, 8), (4, 2), (4, 4), (4, 8)]
# max row nnz of the batch of every shape (fixed_width_K rounds it up to K): 2; 3 and 4; 5, 7 and 8 ...
NNZ = {(2, 2): 2, (2, 4): 3, (2, 8): 5, (3, 2): 2, (3, 4): 4, (3, 8): 7, (4, 2): 2, (4, 4): 3, (4, 8): 8}
# ... and of its many-group batch: the other values of the same K, so that every nnz of 2 .. 8 occurs (6 only here: the
# three K = 8 shapes cannot hold the four values 5 .. 8 in their shape batches alone)
WIDE_NNZ = {(2, 2): 2, (2, 4): 4, (2, 8): 6, (3, 2): 2, (3, 4): 3, (3, 8): 8, (4, 2): 2, (4, 4): 4, (4, 8): 5}


def parse_fixed_width(path=DP_PLAN_H):
    """[(A, K)] of `CMDP_FIXED_WIDTH_SHAPES` in cmdp_dp_plan.h: one X(P, A, K) per shape."""
    src = open(path).read()
    body = re.search(r"#define CMDP_FIXED_WIDTH_SHAPES\(X, P\)((?:[^\n]*\\\n)*[^\n]*)", src).group(1)
    out = []
    for args in re.findall(r"\bX\(([^)]*)\)", body):
        p, a, k = [x.strip() for x in args.split(",")]
        assert p == "P", args
        out.append((int(a), int(k)))
    return out


def fixed_width_K(nnz):
    return 2 if nnz <= 2 else (4 if nnz <= 4 else (8 if nnz <= 8 else 0))


# ---- the statistic CMDP_STAT_DIAMETER_KERNEL (include/cmdp.h) ------------------------------------------------------------
K2, K3, K5S_ELL, K5S_CSR, K5C, K5T = 1, 2, 3, 4, 5, 6
FAMILY_NAME = {K2: "K2", K3: "K3", K5S_ELL: "K5S-ELL", K5S_CSR: "K5S-CSR", K5C: "K5C", K5T: "K5T"}
OPT_AUTO, OPT_K5S, OPT_K5S_CSR, OPT_K5T = 0, 3, 4, 6   # CMDP_OPT_DP_KERNEL


def code(family, n=0, flag=0):
    return family * 1000 + n * 10 + flag


def decode(c):
    return c // 1000, c % 1000 // 10, c % 10


def kernel_id(c, A, K):
    """The compiled kernel a statistic value names on a batch of shape (A, K): the template arguments that matter."""
    fam, n, flag = decode(int(c))
    if fam == K2:
        return ("K2", "lds" if flag else "hbm")
    if fam == K3:
        return ("K3",)
    if fam == K5S_CSR:
        return ("K5S-CSR", n)
    if fam == K5C:
        return ("K5C", n, A, K, "xcd" if flag else "agent")
    return (FAMILY_NAME[fam], n, A, K)


def all_kernels():
    """The compiled set: 27 K5S-ELL, 54 K5C, 9 K5T, the CSR walker, both workgroup forms and the Gauss-Seidel form."""
    out = {("K2", "lds"), ("K2", "hbm"), ("K3",), ("K5S-CSR", 8)}
    for A, K in SHAPES:
        out |= {("K5S-ELL", nw, A, K) for nw in (4, 8, 16)}
        out |= {("K5C", cl, A, K, sc) for cl in (8, 16, 32) for sc in ("xcd", "agent")}
        out.add(("K5T", 6, A, K))
    return out


def launch_groups(sizes, ws_mb=24576, lo=0, hi=None):
    """Groups of 64 targets per launch of `diameter_lanes` for the targets [lo, hi) of the flat state space (`DiamGroups` of
    cmdp.hip with 4 bytes per element and no extra bytes per group): a launch takes groups while their value arrays (512
    bytes per state and group) fit the workspace, and at least one."""
    off = np.concatenate([[0], np.cumsum(sizes)])
    hi = int(off[-1]) if hi is None else hi
    vb = []
    for b, S in enumerate(sizes):
        a, z = max(lo, int(off[b])) - int(off[b]), min(hi, int(off[b + 1])) - int(off[b])
        vb += [2 * int(S) * 64 * 4] * len(range(a, z, 64))
    out, g0 = [], 0
    while g0 < len(vb):
        g1, used = g0, 0
        while g1 < len(vb) and (g1 == g0 or used + vb[g1] <= ws_mb << 20):
            used += vb[g1]
            g1 += 1
        out.append(g1 - g0)
        g0 = g1
    return out


def select_diam(stats, scheme, forced=OPT_AUTO, relabel=False, n_groups=1, cus=CUS, env=None):
    """The CMDP_STAT_DIAMETER_KERNEL value of a diameter call on a batch with `stats` (helpers_dp_shapes.shape_stats):
    scheme 1 Jacobi / 2 Gauss-Seidel, `forced` the handle's CMDP_OPT_DP_KERNEL, `relabel` whether the largest instance
    reaches CMDP_OPT_DIAMETER_RELABEL_MIN_STATES, `n_groups` the groups of the call's last launch (launch_groups), `env`
    the CMDP_* environment switches.  cmdp_diameter_range always takes the lanes kernels: pass forced >= 3 for it.
    (H.UNSUPPORTED, reason) when the workgroup kernels cannot hold the instance.
    Mirrors cmdp_dp_plan.h: `lanes` is pick_diameter_path, the K5C line pick_diameter_cluster (of a handle that is not
    backing off; the flag is the XCD-scope first pass, which diameter_lanes skips under CMDP_K5C_SCOPE=agent), the rest
    pick_diameter_lanes, where `relabel` stands for the handle's ell_relabelled (equal unless CMDP_K5S_CLUSTER=0)."""
    env = env or {}
    A, nnz, _, S, _ = stats
    lanes = scheme == 1 and (forced in (OPT_K5S, OPT_K5S_CSR, OPT_K5T) or 2 * 4 * S + 4 * 4 * (H.DP_BLOCK // 64) > LDS_BUDGET)
    if not lanes:
        fam, key = H.select(stats, "VI", scheme, H.WORKGROUP)
        if fam == H.UNSUPPORTED:
            return fam, key
        return code(K2, 0, int(key == "lds")) if fam == "K2" else code(K3)
    K = fixed_width_K(nnz)
    fixed_ok = (A, K) in parse_fixed_width()
    ell_ok = fixed_ok and forced not in (OPT_K5S_CSR, OPT_K5T)
    k5c = int(env.get("CMDP_K5C", -1))
    cl = k5c if k5c > 0 else 16
    if ell_ok and k5c != 0 and cus % (8 * cl) == 0 and relabel and n_groups > 0 and cl in (8, 16, 32):
        return code(K5C, cl, int(env.get("CMDP_K5C_SCOPE") != "agent"))
    if fixed_ok and forced == OPT_K5T:
        return code(K5T, 6)
    if fixed_ok and forced != OPT_K5S_CSR:
        nw = int(env.get("CMDP_K5S_NW", 0)) or (16 if n_groups <= cus or relabel else 8)
        return code(K5S_ELL, nw if nw in (4, 16) else 8)
    return code(K5S_CSR, 8)


# ---- the generator -----------------------------------------------------------------------------------------------------
def generate_communicating(A, sizes, nnz, seed, p_min=0.05, zeros=False, ring_weight=0.7):
    """tables for BatchedMDP(tables=..., with_env=False), H = 0, one communicating instance per entry of `sizes`.

    Every state s has one row, of a randomly drawn action, that holds the ring successor (s + 1) mod S with probability
    at least ring_weight * (1 - n * p_min) + p_min (n the row's entries): the rows contain the cycle 0 -> 1 -> ... -> 0
    through all states, so every instance is communicating whatever the other entries are.  A row has 1 .. min(nnz, S)
    distinct columns in ascending order -- the ring row of the first state of every instance with S >= nnz exactly nnz, so
    the batch's max row nnz is nnz --, drawn uniformly over the states, the state itself with probability 0.3 (self-loops).
    One-entry ring rows reach the ring successor with probability exactly 1.  Every non-zero probability is at least
    p_min (p = p_min + (1 - n * p_min) * w, w on the simplex); zeros=True sets one entry of some rows, never the ring
    entry, to an explicit 0.0."""
    assert nnz >= 1 and nnz * p_min < 1.0
    rng = np.random.default_rng(seed)
    ptr, col, val = [0], [], []
    for S in sizes:
        for s in range(S):
            ring = (s + 1) % S
            a_ring = int(rng.integers(A))
            for a in range(A):
                n_max = min(nnz, S)
                n = n_max if (s == 0 and a == a_ring) else int(rng.integers(1, n_max + 1))
                cols = {ring} if a == a_ring else set()
                if n > len(cols) and rng.random() < 0.3:
                    cols.add(s)
                while len(cols) < n:
                    cols.add(int(rng.integers(S)))
                cols = sorted(cols)
                w = rng.dirichlet(np.full(n, 0.8))
                zero_at = -1
                if zeros and n >= 2 and rng.random() < 0.25:
                    cand = [i for i, c in enumerate(cols) if not (a == a_ring and c == ring)]
                    zero_at = cand[int(rng.integers(len(cand)))]
                    w[zero_at] = 0.0
                    w = w / w.sum()
                if a == a_ring:
                    w = (1.0 - ring_weight) * w
                    w[cols.index(ring)] += ring_weight
                live = n - (zero_at >= 0)
                p = p_min + (1.0 - live * p_min) * w
                if zero_at >= 0:
                    p[zero_at] = 0.0
                col.extend(cols)
                val.extend(p.astype(np.float32).tolist())
                ptr.append(ptr[-1] + n)
    n_states = int(np.sum(sizes))
    return dict(B=len(sizes), A=A, H=0, rewards_range=(0.0, 1.0),
                state_off=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64),
                csr_ptr=np.asarray(ptr, np.int64), csr_col=np.asarray(col, np.int32), csr_val=np.asarray(val, np.float32),
                R=np.zeros(n_states * A, np.float32))


def chunk_states(A, K):
    """U: the states whose A*K entries one 64-lane load of the fixed-width kernels fetches."""
    return 64 // (A * K)


def shape_sizes(A, K):
    """1, 2, a size just below U (where U > 2), 64, 65 (a last group of one target) and 333 states -- no multiple of any U
    or of 64, the largest and not the last, and with the rest more than a workspace of 1 MB holds in one launch; the last
    instance (3 states) ends inside a chunk, whose 64-lane entry load runs on into the tail padding of the fixed-width
    rows."""
    U = chunk_states(A, K)
    return [2, 333, 1] + ([U - 1] if U > 2 else []) + [65, 64, 3]


def shape_batch(A, K, seed=None):
    """The batch of one fixed-width shape; the three-action batches carry explicit zeros."""
    seed = 100 * A + K if seed is None else seed
    return generate_communicating(A, shape_sizes(A, K), NNZ[A, K], seed, zeros=A == 3)


def wide_sizes(groups=CUS + 2):
    """More groups than compute units in one launch (K5S then runs 8 wavefronts per group): 131, 65 and 97 states -- three,
    two and two groups, and more than 8 * U states for every U -- and one-group instances of 1 .. 12 states."""
    return [131, 65, 97] + [1 + i % 12 for i in range(groups - 7)]


def wide_batch(A, K, groups=CUS + 2):
    return generate_communicating(A, wide_sizes(groups), WIDE_NNZ[A, K], 1000 + 100 * A + K)


def strongly_connected(S, A, csr):
    """Graph search over the edges of positive probability."""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components

    ptr, col, val = csr
    rows = np.repeat(np.arange(S * A) // A, np.diff(ptr))
    keep = np.asarray(val) > 0
    g = csr_matrix((np.ones(int(keep.sum())), (rows[keep], np.asarray(col)[keep])), shape=(S, S))
    return connected_components(g, directed=True, connection="strong")[0] == 1


# ---- float64 references ------------------------------------------------------------------------------------------------
def _sparse_P(S, A, csr):
    from scipy.sparse import csr_matrix

    ptr, col, val = csr
    return csr_matrix((np.asarray(val, np.float64), np.asarray(col, np.int64), np.asarray(ptr, np.int64)), shape=(S * A, S))


def jacobi_f64(S, A, csr, target, eps, max_sweeps, scheme=1, stop=0.5):
    """`_continuous_diam_calculation` (colosseum/hardness/measures/diameter.py:76-96) in float64: the row of the target
    absorbing with reward 0, every other reward -1, gamma 1, V_0 = 0, Jacobi sweeps (scheme 2: Gauss-Seidel sweeps in
    state order, as the reference's dense branch and k_dp_wave_gs run them).  `target` is one state or an array of them,
    solved side by side.  Returns the whole trajectory as arrays [n, targets]: diff[n] = max|V_n+1 - V_n|, r = -min V and
    vabs = max|V| after every sweep.  The sweeps go on until every target has diff < stop * eps -- beyond the stopping
    sweep of any float32 solve `admissible` accepts -- or max_sweeps."""
    tg = np.atleast_1d(np.asarray(target, np.int64))
    T = len(tg)
    cols = np.arange(T)
    V = np.zeros((S, T))
    diff, r, vabs = [], [], []
    if scheme == 1:
        P = _sparse_P(S, A, csr)
    else:
        ptr, col, val = csr
        kmax = int(np.diff(ptr).max())
        pc = np.zeros((S * A, kmax), np.int64)
        pv = np.zeros((S * A, kmax))
        for k in range(kmax):
            has = np.diff(ptr) > k
            pc[has, k] = np.asarray(col)[ptr[:-1][has] + k]
            pv[has, k] = np.asarray(val, np.float64)[ptr[:-1][has] + k]
        pc, pv = pc.reshape(S, A, kmax), pv.reshape(S, A, kmax, 1)
        is_target = [cols[tg == s] for s in range(S)]
    for _ in range(int(max_sweeps)):
        if scheme == 1:
            Vn = (-1.0 + (P @ V).reshape(S, A, T)).max(1)
            Vn[tg, cols] = V[tg, cols]
        else:
            Vn = V.copy()
            for s in range(S):
                v = (-1.0 + (pv[s] * Vn[pc[s]]).sum(1)).max(0)
                v[is_target[s]] = Vn[s, is_target[s]]
                Vn[s] = v
        diff.append(np.abs(Vn - V).max(0))
        r.append(-Vn.min(0))
        vabs.append(np.abs(Vn).max(0))
        V = Vn
        if (diff[-1] < stop * eps).all():
            break
    return dict(diff=np.array(diff), r=np.array(r), vabs=np.array(vabs))


def hitting_f64(S, A, csr, target):
    """Exact optimal expected hitting times h[s] of `target` (h[target] = 0, h[s] = 1 + min_a sum_j P[s, a, j] h[j]) by
    float64 policy iteration with one linear solve per policy.  The first policy follows a breadth-first search backwards
    from the target (it reaches the target with probability 1, so its system is regular); an action is only replaced by
    a strictly better one, as in helpers_dp_shapes.vi_f64."""
    P = H.dense_P(S, A, csr).reshape(S, A, S)
    if S == 1:
        return np.zeros(1)
    dist = np.full(S, -1)
    dist[target] = 0
    act = np.zeros(S, np.int64)
    frontier = [target]
    while frontier:
        nxt = []
        for j in frontier:
            for s, a in zip(*np.nonzero(P[:, :, j] > 0)):
                if dist[s] < 0:
                    dist[s], act[s] = dist[j] + 1, a
                    nxt.append(s)
        frontier = nxt
    assert (dist >= 0).all(), "the target is not reachable from every state"
    others = np.arange(S) != target
    idx = np.arange(S)
    for _ in range(1000):
        Ppi = P[idx, act]
        h = np.zeros(S)
        h[others] = np.linalg.solve(np.eye(S - 1) - Ppi[np.ix_(others, others)], np.ones(S - 1))
        Q = 1.0 + P @ h
        best = Q.argmin(1)
        better = Q[idx, best] < Q[idx, act] - 1e-12 * max(1.0, h.max())
        better[target] = False
        if not better.any():
            return h
        act = np.where(better, best, act)
    raise AssertionError("float64 policy iteration did not settle")


def gs_chain(S, A, csr):
    """The factor by which one float32 Gauss-Seidel sweep can exceed the per-backup error d: state s is backed up from
    values of which those of states j < s are already this sweep's, so its error is at most
    c_s d with c_s = 1 + max_a sum_{j < s} P[s, a, j] c_j (a maximum of averages passes on at most the average of the
    errors it is given).  Returns max_s c_s, computed from the tables."""
    ptr, col, val = csr
    c = np.ones(S)
    for s in range(S):
        best = 0.0
        for a in range(A):
            lo, hi = int(ptr[s * A + a]), int(ptr[s * A + a + 1])
            cc, vv = np.asarray(col[lo:hi]), np.asarray(val[lo:hi], np.float64)
            best = max(best, float((vv[cc < s] * c[cc[cc < s]]).sum()))
        c[s] = 1.0 + best
    return float(c.max())


def admissible(traj, eps, K, chain=1.0):
    """Which stopping sweeps, and which results, a correct float32 solve of ONE target may show, given the float64
    trajectory `traj` (diff, r, vabs: one value per sweep) of the same tables.  No number in it is chosen.

    The backup V -> max_a (-1 + sum_j p_j V_j) is a maximum over averages, hence non-expansive in the sup norm.  Evaluated
    in float32 on rows of at most K entries whose float32 probabilities sum to 1 within K u, it departs from the exact
    backup of the same iterate by at most d_n = (K + 2) 2^-23 max_{j <= n} |V_j| (the per-backup bound of
    helpers_dp_shapes.f64_bound: K products, K - 1 sums, the product by gamma and the sum with the reward; a Gauss-Seidel
    sweep by `chain` times that, see gs_chain).  So after n sweeps from the same V_0 the float32 and the float64 iterates
    are within E_n = sum_{j <= n} d_j, and their values diff_n = max|V_n - V_n-1| within 2 E_n.  (The float32 difference
    itself is exact: the values are 0 or <= -1, and near the threshold the two operands are within a factor of two.)
    The float32 solve stops at its FIRST sweep with diff < eps and returns -min V of that sweep, so its stopping sweep m has
        diff64_m < eps + 2 E_m      and      no j < m with diff64_j < eps - 2 E_j,
    and its result lies in [r64_m - E_m, r64_m + E_m].  Returns [(m, lo, hi, E_m)] for every such m (sweeps count from 1).
    Where 2 E_j reaches eps before diff64 has fallen below eps - 2 E_j the second condition excludes nothing; then the
    sweeps of the trajectory as far as it was computed (jacobi_f64: to diff64 < eps / 2) are the candidates, which only
    narrows what passes."""
    diff, r, vabs = (np.asarray(traj[k], np.float64) for k in ("diff", "r", "vabs"))
    d = chain * (K + 2) * 2.0 ** -23 * np.maximum.accumulate(vabs)
    E = np.cumsum(d)
    sure = np.flatnonzero(diff < eps - 2 * E)
    last = int(sure[0]) if len(sure) else len(diff) - 1
    ms = [m for m in range(last + 1) if diff[m] < eps + 2 * E[m]]
    return [(m + 1, r[m] - E[m], r[m] + E[m], E[m]) for m in ms]


def accepts(intervals, value):
    return any(lo <= float(value) <= hi for _, lo, hi, _ in intervals)


@functools.lru_cache(maxsize=None)
def _reference(key, scheme, eps):
    t = BATCHES[key]()
    out = []
    for b in range(int(t["B"])):
        S, A, csr, _ = H.instance(t, b)
        traj = jacobi_f64(S, A, csr, np.arange(S), eps, 5000, scheme)
        assert (traj["diff"].min(0) < eps).all(), (key, b, "a target needs more than 5000 float64 sweeps")
        SWEEPS64[key, scheme, eps] = max(SWEEPS64.get((key, scheme, eps), 0), int((traj["diff"] >= eps).sum(0).max()) + 1)
        chain = gs_chain(S, A, csr) if scheme == 2 else 1.0
        nnz = int(np.diff(t["csr_ptr"]).max())
        out.append([admissible({k: v[:, j] for k, v in traj.items()}, eps, nnz, chain) for j in range(S)])
    return out


SWEEPS64 = {}   # (batch, scheme, eps) -> largest number of float64 sweeps a target of the batch needs to reach diff < eps

# the batches of the suite by name: built on demand, their float64 references computed once per process
BATCHES = {}
for _A, _K in SHAPES:
    BATCHES["shape", _A, _K] = functools.partial(shape_batch, _A, _K)
    BATCHES["wide", _A, _K] = functools.partial(wide_batch, _A, _K)
BATCHES["hbm"] = lambda: generate_communicating(4, [450], 8, 77, ring_weight=0.9)    # K2 streams the CSR from HBM
BATCHES["limit"] = lambda: generate_communicating(3, [7, 70, 3], 4, 80)            # the sweep-limit tests
BATCHES["k5d"] = lambda: generate_communicating(3, [2, 150, 65, 7, 64], 4, 81)     # the sparse float64 diameter
BATCHES["A5"] = lambda: generate_communicating(5, [70, 1, 9], 4, 78)               # no fixed-width shape: five actions
BATCHES["nnz9"] = lambda: generate_communicating(3, [70, 1, 9], 9, 79)             # ... nine entries in a row


@functools.lru_cache(maxsize=None)
def batch(key):
    return BATCHES[key]()


def reference(key, scheme=1, eps=EPS):
    """Per instance and target of batch `key`: the admissible (sweep, lo, hi, E) list of the float64 trajectory."""
    return _reference(key, scheme, eps)


@functools.lru_cache(maxsize=None)
def oracle(key, scheme=1, eps=EPS, max_sweeps=1_000_000):
    """[(diameter, per_target)] per instance from the C oracle."""
    from oracle import oracle as O

    t = batch(key)
    out = []
    for b in range(int(t["B"])):
        S, A, csr, _ = H.instance(t, b)
        out.append(O.diameter_continuous(S, A, csr, eps, scheme, max_sweeps))
    return out


def check_f64(key, per, scheme=1, eps=EPS):
    """Every per-target value of `per` (flat, the batch's state order) lies in an admissible interval.  Returns the
    findings of the batch, none of them asserted:
      the largest number of sweeps a target's float64 solve takes to its first diff < eps (SWEEPS64),
      the largest E_m over the admissible sweeps m of every target,
      the largest distance of a value to the float64 r of the NEAREST admissible sweep (the float32 solve's own stopping
        sweep is not reported by the library, so this is a lower bound of its distance to the float64 value there),
      the largest width of a target's union of intervals relative to its float64 value at the first admissible sweep (or
        to 1 where that is smaller): how coarse the check is."""
    ref = reference(key, scheme, eps)
    off = batch(key)["state_off"]
    worst = [SWEEPS64[key, scheme, eps], 0.0, 0.0, 0.0]
    for b, targets in enumerate(ref):
        for j, iv in enumerate(targets):
            v = float(per[int(off[b]) + j])
            assert accepts(iv, v), (key, scheme, b, j, v, iv[:3])
            worst[1] = max(worst[1], max(e for _, _, _, e in iv))
            worst[2] = max(worst[2], min(abs(v - (lo + hi) / 2) for _, lo, hi, _ in iv))
            r = max((iv[0][1] + iv[0][2]) / 2, 1.0)
            worst[3] = max(worst[3], (max(hi for _, _, hi, _ in iv) - min(lo for _, lo, _, _ in iv)) / r)
    return tuple(worst)
