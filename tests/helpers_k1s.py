"""Generated batches for the stochastic-dynamics rollout K1S (csrc/cmdp_k1s.h): raw sampler tables in the `tables=` layout
of colosseum_amd.batched (what `_det` of test_gpu_rollout_plans.py builds for deterministic rows), with a parameter for
every quantity `plan_k1s` branches on -- entries per row, successor-set size, cumulative-probability patterns, reward
values and what the reward is a function of, start states, state counts.  Host only: nothing here touches a GPU."""
import numpy as np

TOTALS = (1.0, 0.75, 1.5, 3.0)   # totals of the cumulative vectors: the sampler scales the uniform by the last value
LAUNCHES = (1, 31, 32, 33, 700, 9001)   # mid-episode / mid-Philox-block starts, the chunk edge, one flush crossing (7 680)


def _pattern(rng, n, total):
    """A non-decreasing cumulative vector of n entries ending (to rounding) at `total`.  From three entries on at least one
    entry has zero width -- a repeated value, or a leading 0 -- and at least two have not, so that the draw matters."""
    w = rng.random(n) + 0.05
    if n >= 3:
        keep = rng.choice(n, 2, replace=False)
        zero = rng.random(n) < 0.3
        zero[rng.choice(np.setdiff1d(np.arange(n), keep))] = True
        zero[keep] = False
        w[zero] = 0.0
    return np.cumsum(w * (total / w.sum()))


def patterns(rng, n_pat, entries):
    """n_pat distinct cumulative vectors with lengths in entries = (min, max): the first has max entries, the second min."""
    lo, hi = entries
    out, seen = [], set()
    first = int(rng.integers(len(TOTALS)))   # (a batch with one pattern does not always get the total 1)
    while len(out) < n_pat:
        n = hi if len(out) == 0 else lo if len(out) == 1 else int(rng.integers(lo, hi + 1))
        c = _pattern(rng, n, TOTALS[(first + len(out)) % len(TOTALS)])
        if c.tobytes() not in seen:
            seen.add(c.tobytes())
            out.append(c)
    return out


def tables(seed, B, S, A=2, H=0, entries=(2, 3), succ=3, n_pat=1, n_rew=3, reward_by="state", n_start=1, self_loop=0.0,
           rewards_range=(0.0, 1.0), templates=None, absorbing=False):
    """B instances of S states (a scalar, or a list of B sizes: ragged) and A actions.

    entries      (min, max) entries per row; every row takes one of the batch's n_pat cumulative vectors
    succ         size of a state's successor set: the entries of its A rows name `succ` distinct states (fewer when the
                 instance or the state's rows are too small to hold as many), all of which occur
    n_rew        distinct reward values, k / 7 -- not dyadic, so the order of the float64 sum matters
    reward_by    "state": a function of the successor state; "row": of (state, action); "neither": drawn per entry
    n_start      start states per instance, with unequal probabilities
    self_loop    probability that an entry leads back to its own state
    templates    None: every instance draws its own tables; T: instance b is a copy of instance b % T (few row shapes in a
                 large batch; needs a scalar S)
    absorbing    state 0 only leads to itself and all entries but the narrowest of every other row lead to it"""
    rng = np.random.default_rng(seed)
    sizes = [int(S)] * B if np.isscalar(S) else [int(x) for x in S]
    assert len(sizes) == B and reward_by in ("state", "row", "neither")
    assert templates is None or np.isscalar(S)
    pats = patterns(rng, n_pat, entries)
    vals = np.arange(n_rew) / 7.0
    seen = dict(pat=0, state=0, row=0)   # the first n_pat rows / n_rew states / n_rew rows of the batch cover every value

    def cover(what, n):
        k = seen[what]
        seen[what] += 1
        return k if k < n else int(rng.integers(n))

    def instance(Sb):
        lens, nxt, cum, rew = [], [], [], []
        code_state = np.array([cover("state", n_rew) for _ in range(Sb)])
        for s in range(Sb):
            others = [int(x) for x in rng.choice(Sb, min(Sb, succ + 2), replace=False) if x != s and not (absorbing and x == 0)]
            head = ([s] if self_loop > 0 else []) + ([0] if absorbing and s != 0 else [])
            sset = [0] if absorbing and s == 0 else (head + others)[:succ]
            # every member occurs (unless absorbing): handed out first, in the order the rows are drawn
            need = [] if absorbing else list(rng.permutation(sset))
            for a in range(A):
                c = pats[cover("pat", n_pat)]
                code_row = cover("row", n_rew)
                away = int(np.argmin(np.diff(c, prepend=0.0)))   # absorbing: every entry but the narrowest leads to state 0
                for k in range(len(c)):
                    if absorbing and k != away:
                        x = 0
                    elif self_loop > 0 and s in sset and rng.random() < self_loop:
                        x = s
                    else:
                        x = need.pop() if need and rng.random() < 0.7 else sset[rng.integers(len(sset))]
                    if x in need:
                        need.remove(x)
                    nxt.append(x)
                    rew.append(vals[code_state[x] if reward_by == "state" else code_row if reward_by == "row"
                                    else rng.integers(n_rew)])
                lens.append(len(c))
                cum.append(c)
            tail = sum(lens[-A:])
            if need and tail >= len(sset):   # the draw above did not name every member: overwrite the state's first entries
                for j, x in enumerate(sset):
                    e = len(nxt) - tail + j
                    nxt[e] = x
                    if reward_by == "state":
                        rew[e] = vals[code_state[x]]
        st = rng.choice(Sb, n_start, replace=n_start > Sb)
        p = rng.random(n_start) + 0.1
        return lens, nxt, np.concatenate(cum), rew, st, np.cumsum(p / p.sum())

    made = [instance(sizes[b]) for b in range(templates or B)]
    inst = [made[b % len(made)] for b in range(B)]
    lens = np.concatenate([i[0] for i in inst])
    rew = np.concatenate([i[3] for i in inst]).astype(np.float64)
    n_st = [len(i[4]) for i in inst]
    R = len(lens)
    return dict(
        B=B, A=A, H=H, rewards_range=tuple(float(x) for x in rewards_range),
        state_off=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64),
        sp_ptr=np.concatenate([[0], np.cumsum(lens)]).astype(np.int64),
        sp_next=np.concatenate([i[1] for i in inst]).astype(np.int32), sp_cum=np.concatenate([i[2] for i in inst]),
        sp_reward=rew, sp_rkind=np.zeros(len(rew), np.uint8), sp_rp0=rew, sp_rp1=np.zeros(len(rew)),
        sp_seed=np.zeros(R, np.int32), start_off=np.concatenate([[0], np.cumsum(n_st)]).astype(np.int64),
        start_state=np.concatenate([i[4] for i in inst]).astype(np.int32), start_cum=np.concatenate([i[5] for i in inst]),
        start_seed=np.zeros(B, np.int32))


def keys(B, seed=0):
    """Philox keys of a batch: distinct, with bits in both 32-bit halves."""
    return (np.arange(B, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(seed * 7919 + 11)).astype(np.uint64)


def describe(t):
    """What the generator actually produced, counted from the tables (the tests check their premises against it)."""
    A, ptr = int(t["A"]), t["sp_ptr"]
    n = np.diff(ptr)
    rows = [t["sp_cum"][ptr[r]:ptr[r + 1]] for r in range(len(n))]
    state_of_row = np.repeat(np.arange(len(n) // A), A)
    succ = [set() for _ in range(len(n) // A)]
    for r in range(len(n)):
        succ[state_of_row[r]].update(t["sp_next"][ptr[r]:ptr[r + 1]].tolist())
    return dict(entries=(int(n.min()), int(n.max())), n_pat=len({c.tobytes() for c in rows}),
                max_succ=max(len(x) for x in succ), n_rew=len(np.unique(t["sp_reward"])),
                totals=sorted({float(c[-1]) for c in rows}), ties=any(len(c) > 1 and (np.diff(c) == 0).any() for c in rows),
                max_starts=int(np.diff(t["start_off"]).max()))
