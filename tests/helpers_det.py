"""Generated batches for the deterministic LDS-resident rollouts K1L / K1P / K1T / K1U (csrc/cmdp_kernels.h, cmdp_k1t.h,
cmdp_k1u.h): raw sampler tables in the `tables=` layout of colosseum_amd.batched, with a parameter for every quantity the
planners of csrc/cmdp_rollout_plan.h branch on -- rows per instance, distinct reward values, whether the instances are
action swaps of the first one -- and for what the kernels' episode and counter logic depends on: horizon, start states,
an absorbing state.  Host only: nothing here touches a GPU."""
import numpy as np

from helpers_k1s import keys   # noqa: F401  (the Philox keys of a batch, shared with the K1S cases)

# Back to back on one handle: launches start mid-episode and mid-Philox-block (four actions per block), some are shorter
# than one group of 8 transitions, and the last crosses one flush period of the packed kernels (7 680 / 3 584 transitions)
LAUNCHES = (1, 7, 8, 9, 63, 700, 9001)


def reward_values(rng, n_rew, rewards_range):
    """n_rew distinct float64 values spread over the range, one per equal bin of it (so negative ones occur whenever the
    range has a negative part wider than a bin), each with a full random mantissa: sums of them round, so the order of a
    float64 sum is visible."""
    lo, hi = float(rewards_range[0]), float(rewards_range[1])
    v = lo + (hi - lo) * (np.arange(n_rew) + 0.25 + 0.5 * rng.random(n_rew)) / n_rew
    return rng.permutation(v)


def tables(seed, B, S, A=2, H=0, n_rew=3, permuted=True, start="fixed", absorbing=False, rewards_range=(0.0, 1.0)):
    """B instances of S states and A actions, every row with one successor, one start state per instance.

    permuted     instance b is instance 0 with the two actions swapped in a random half of the states (A = 2): what K1T /
                 K1U need.  False: every instance draws its own successors and reward codes
    n_rew        distinct reward values (see reward_values); every one occurs in the table, for `permuted` in instance 0
    start        "fixed": one non-zero start state for all instances (state 0 when S = 1); "per_instance": 1 + b mod
                 (S - 1), so that neighbouring instances start in different states
    absorbing    every row of every instance leads to state 0"""
    rng = np.random.default_rng(seed)
    assert start in ("fixed", "per_instance") and (not permuted or A == 2)
    assert n_rew <= (S * A if permuted else B * S * A)
    vals = reward_values(rng, n_rew, rewards_range)

    def draw():
        n = np.zeros((S, A), np.int64) if absorbing else rng.integers(0, S, (S, A))
        return n, rng.integers(0, n_rew, (S, A))

    base_n, base_r = draw()
    if permuted:
        base_r.flat[rng.permutation(S * A)[:n_rew]] = np.arange(n_rew)
        if n_rew > 1 and base_r[0, 0] == base_r[0, 1]:   # the rows of state 0 differ: a swap of them shows in the reward sum
            k = int(np.flatnonzero(base_r.reshape(-1) != base_r[0, 0])[0])   # (exchanging two rows keeps every value)
            base_r.flat[1], base_r.flat[k] = base_r.flat[k], base_r.flat[1]
    nxt, code = [], []
    for b in range(B):
        if permuted:
            swap = (rng.random(S) < 0.5) & (b > 0)
            n, r = np.where(swap[:, None], base_n[:, ::-1], base_n), np.where(swap[:, None], base_r[:, ::-1], base_r)
        else:
            n, r = (base_n, base_r) if b == 0 else draw()
        nxt.append(n.reshape(-1))
        code.append(r.reshape(-1))
    code = np.concatenate(code)
    if not permuted:   # every value occurs somewhere in the batch
        code[rng.permutation(len(code))[:n_rew]] = np.arange(n_rew)
    rew = vals[code]
    R = B * S * A
    first = 0 if S == 1 else 1 + int(rng.integers(S - 1))
    st = np.full(B, first) if start == "fixed" or S == 1 else 1 + np.arange(B) % (S - 1)
    return dict(
        B=B, A=A, H=H, rewards_range=tuple(float(x) for x in rewards_range),
        state_off=(np.arange(B + 1) * S).astype(np.int64),
        sp_ptr=np.arange(R + 1, dtype=np.int64), sp_next=np.concatenate(nxt).astype(np.int32),
        sp_cum=np.ones(R), sp_reward=rew, sp_rkind=np.zeros(R, np.uint8), sp_rp0=rew, sp_rp1=np.zeros(R),
        sp_seed=np.zeros(R, np.int32), start_off=np.arange(B + 1, dtype=np.int64),
        start_state=st.astype(np.int32), start_cum=np.ones(B), start_seed=np.zeros(B, np.int32))


def describe(t):
    """What the generator actually produced, counted from the tables (the tests check their premises against it)."""
    B, A = int(t["B"]), int(t["A"])
    S = int(t["state_off"][1])
    nxt, rew = t["sp_next"].reshape(B, S, A), t["sp_reward"].reshape(B, S, A)
    same = (nxt == nxt[0]).all(axis=2) & (rew == rew[0]).all(axis=2)
    swapped = (nxt == nxt[0][:, ::-1]).all(axis=2) & (rew == rew[0][:, ::-1]).all(axis=2)
    scaled = np.unique(rew) * 2.0 ** 20
    return dict(rows=S * A, n_rew=len(np.unique(rew)), n_rew_instance0=len(np.unique(rew[0])),
                negative_rewards=int((np.unique(rew) < 0).sum()), dyadic_rewards=int((scaled == np.round(scaled)).sum()),
                start_states=sorted(set(t["start_state"].tolist())), swaps_only=bool((same | swapped).all()),
                swapped_states=int((swapped & ~same).sum()), max_row_index=int(nxt.max()) * A + A - 1,
                all_lead_to_0=bool((nxt == 0).all()))
