"""Every compiled form of the deterministic LDS-resident rollouts -- K1L (k_rollout_lds<PACKED>), K1P (k_rollout_pipe), K1T
(k_rollout_tmpl) and K1U (k_rollout_tmpl_stream<PACK10> + k_trace_hist) -- on generated batches: bit for bit against the
lane-per-instance kernel K1 and against the CPU oracle, every instance.

The planners of csrc/cmdp_rollout_plan.h choose packed or unpacked tables, the pipeline or the fused walker, a chunk length
and the instances per workgroup; on a 256-CU device small batches always get one or two instances per workgroup and the
roomy chunk length.  CMDP_K1L_G / CMDP_K1T_G / CMDP_K1U_G set the instances per workgroup and CMDP_K1T_CH the chunk length
of K1T, so that small batches reach every form, and every case first asserts through the plan query (cmdp_det_plan, whose
`form` is computed by the function the launcher branches on) that it landed where it says.  The same assertions, the
planner's refusal edges, an LDS invariant and the plans at other CU counts run without a GPU through cmdp_det_plan_desc.
helpers_det has the generator.

Where the kernels' own limits shape the matrix:
  * the unpacked K1L needs more than 16 bits for row base + reward code, that is more than 256 rows: its geometry cases
    use 257 .. 265 rows (S x A = 257 x 1, 129 x 2, 87 x 3, 53 x 5), and its largest group is the LDS capacity of its
    candidate (43 at two workgroups per CU), not the 64 lanes;
  * reward sums cannot differ between instances of a batch with ONE reward value: those cases skip that assertion;
  * oracle.batch_rollout has no masked reset: the cases with one run per-instance oracle environments through the same
    script of resets and launches."""
import functools
import os
import types

import numpy as np
import pytest

import helpers_det as D
from colosseum_amd import _lib as L
from colosseum_amd.batched import BatchedMDP, det_plan_of_tables
from oracle import oracle as O

ENV = dict(pipe="CMDP_K1L_PIPE", k1l_G="CMDP_K1L_G", k1t_G="CMDP_K1T_G", k1u_G="CMDP_K1U_G", k1t_ch="CMDP_K1T_CH")
KNOBS = tuple(ENV.values()) + ("CMDP_K1S_G",)   # the environment cmdp_create reads
CUS = 256   # the MI355X; the planned G of the knob-less batches holds for it only
LDS = 160 * 1024
# kernel -> (CMDP_OPT_ROLLOUT_KERNEL, its part of the plan, what cmdp_lds_plan calls it, the knob of its G, lane limit)
KERNEL = {"k1l": (L.ROLLOUT_LDS, "k1lp", "k_rollout_lds", "k1l_G", 64), "k1p": (L.ROLLOUT_LDS, "k1lp", "k_rollout_pipe", "k1l_G", 64),
          "k1t": (L.ROLLOUT_LDS_TEMPLATE, "k1t", "k_rollout_tmpl", "k1t_G", 128),
          "k1u": (L.ROLLOUT_LDS_TEMPLATE_STREAM, "k1u", "k_rollout_tmpl_stream", "k1u_G", 256)}
PIPE = {"k1l": 0, "k1p": 1}
CAPACITY = 1000   # a G knob no plan has room for: G = capacity
MASKED_AFTER = 2   # the masked reset comes after the launches of 1 and 7 transitions
FLAVOUR_G = {"k1l": 20, "k1p": 20, "k1t": 50, "k1u": 100}


def _ragged_B(G):
    """2 G + r instances, 0 < r < G (G = 1: three groups of one)"""
    return 3 if G == 1 else 2 * G + max(1, G // 3)


def _case(kernel, gen, want, G=None, extra=(), masked=False, **knobs):
    """(kernel, generator arguments, knobs, expected plan fields of the kernel, extra launches, masked reset)"""
    if kernel in PIPE:
        knobs.setdefault("pipe", PIPE[kernel])
    if G:
        knobs[KERNEL[kernel][3]] = G
        want = dict(want, G="capacity" if G == CAPACITY else G)
    if "permuted" not in gen:
        gen = dict(gen, permuted=kernel in ("k1t", "k1u"))
    return types.SimpleNamespace(kernel=kernel, gen=gen, knobs=knobs, want=want, extra=tuple(extra), masked=masked)


UNPACKED = dict(n_rew=256)   # with more than 256 rows: 9 + 8 bits
PACKED_SHAPES = ((5, 1), (6, 2), (7, 3), (5, 5), (7, 1), (6, 3), (7, 5))   # (S, A): row counts 5 .. 35, odd ones among them
UNPACKED_SHAPES = ((257, 1), (129, 2), (87, 3), (53, 5))                    # 257 .. 265 rows
FORM = {"k1l": "k1l_packed", "k1p": "k1p"}


def _cases():
    c = {}
    # ---- group geometry: G instances per workgroup, ragged last group, rows of later groups misaligned for the 16-byte loads
    for label, kernel, shapes, more, Gs in (("k1l_packed", "k1l", PACKED_SHAPES, {}, (1, 2, 3, 7, 8, 33, 64)),
                                            ("k1p", "k1p", PACKED_SHAPES, {}, (1, 2, 3, 7, 8, 33, 64)),
                                            ("k1l_unpacked", "k1l", UNPACKED_SHAPES, UNPACKED, (1, 2, 3, 7, 8, 33, CAPACITY))):
        for i, G in enumerate(Gs):
            S, A = shapes[i % len(shapes)]
            B = _ragged_B(43 if G == CAPACITY else G)
            gen = dict(seed=100 + i, B=B, S=S, A=A, H=(0, 12)[i % 2], start=("fixed", "per_instance")[i // 2 % 2], **more)
            c[f"geometry_{label}_G{'cap' if G == CAPACITY else G}"] = _case(kernel, gen, dict(form=label), G=G)
        S, A = shapes[1]
        c[f"geometry_{label}_full_groups"] = _case(kernel, dict(seed=120, B=21, S=S, A=A, H=5, **more), dict(form=label), G=7)
    for kernel, cap in (("k1t", 128), ("k1u", 256)):   # (K1T / K1U: one instance per workgroup, and all that fit)
        c[f"geometry_{kernel}_G1"] = _case(kernel, dict(seed=130, B=3, S=7, H=4), {}, G=1)
        c[f"geometry_{kernel}_Gcap"] = _case(kernel, dict(seed=131, B=_ragged_B(cap), S=6, H=0, start="per_instance"), dict(G=cap), G=CAPACITY)
    # ---- episode flavours: T0, one reset per group of 8 (H >= 8), T1 (H < 8), T2 without episodes, and -- after a masked reset
    #      that leaves the instances of one workgroup at different in-episode times -- T2 with terminations
    vary = {0: {}, 1: dict(start="per_instance"), 3: dict(rewards_range=(-2.5, 4.0)), 8: dict(start="per_instance"), 9: {},
            20: dict(rewards_range=(0.3, 1.7))}
    for label, kernel, more in (("k1l_packed", "k1l", dict(S=6)), ("k1l_unpacked", "k1l", dict(S=129, **UNPACKED)), ("k1p", "k1p", dict(S=6)),
                                ("k1t", "k1t", dict(S=6)), ("k1u", "k1u", dict(S=6))):
        G = FLAVOUR_G[kernel]
        want = dict(form=label) if kernel in PIPE else {}
        for H, v in vary.items():
            c[f"episodes_{label}_H{H}"] = _case(kernel, dict(seed=200 + H, B=_ragged_B(G), H=H, **more, **v), want, G=G)
        for H, v in ((9, dict(start="per_instance")), (5, dict(rewards_range=(-2.5, 4.0)))):
            c[f"episodes_{label}_H{H}_masked"] = _case(kernel, dict(seed=230 + H, B=_ragged_B(G), H=H, **more, **v), want, G=G, masked=True)
    # ---- packing boundary: bits of a row base + bits of a reward code = 15 (K1P / K1T / K1U fill the 16-bit word), 16 (K1L
    #      alone, packed), 17 (K1L unpacked); one reward value (no code bits)
    for kernel in KERNEL:
        G = FLAVOUR_G[kernel]
        want = dict(form=FORM[kernel], succ_bits=8, n_codes=128, code_shift=8 + PIPE[kernel]) if kernel in PIPE else {}
        c[f"bits15_{kernel}"] = _case(kernel, dict(seed=300, B=_ragged_B(G), S=128, n_rew=128, H=7, permuted=True), want, G=G)
        want = dict(form=FORM[kernel], succ_bits=6, n_codes=1) if kernel in PIPE else {}
        c[f"one_reward_{kernel}"] = _case(kernel, dict(seed=301, B=_ragged_B(G), S=20, n_rew=1, H=11, permuted=True), want, G=G)
    for kernel in PIPE:
        c[f"one_row_{kernel}"] = _case(kernel, dict(seed=302, B=46, S=1, A=1, n_rew=1, H=3), dict(form=FORM[kernel], succ_bits=1), G=20)
    c["bits16_S128_rewards256"] = _case("k1l", dict(seed=303, B=46, S=128, n_rew=256, H=0), dict(form="k1l_packed", succ_bits=8, code_shift=8), G=20)
    c["bits16_S129_rewards128"] = _case("k1l", dict(seed=304, B=46, S=129, n_rew=128, H=6), dict(form="k1l_packed", succ_bits=9, code_shift=9), G=20)
    c["bits17_S129_rewards129"] = _case("k1l", dict(seed=305, B=46, S=129, n_rew=129, H=0), dict(form="k1l_unpacked", succ_bits=9, code_shift=0), G=20)
    c["bits17_S129_rewards256"] = _case("k1l", dict(seed=306, B=46, S=129, n_rew=256, H=14, rewards_range=(-2.5, 4.0)),
                                        dict(form="k1l_unpacked", succ_bits=9, code_shift=0), G=20)
    # ---- the unpacked form's flush period of 32 768 transitions; absorbing: one 16-bit half collects a whole period
    c["unpacked_flush"] = _case("k1l", dict(seed=310, B=46, S=129, H=0, **UNPACKED), dict(form="k1l_unpacked", ch=256), G=20, extra=(33_001,))
    c["unpacked_flush_absorbing"] = _case("k1l", dict(seed=311, B=46, S=300, A=1, H=0, absorbing=True, **UNPACKED),
                                          dict(form="k1l_unpacked", ch=256), G=20, extra=(33_001,))
    # ---- chunk lengths: LDS is tight (one instance of ~20 KB per workgroup, room for 8), so the shorter rings are planned
    for kernel, S, ch in (("k1l", 3270, 128), ("k1l", 3292, 112), ("k1l", 3300, 64), ("k1p", 3280, 32), ("k1p", 3305, 16)):
        c[f"chunk_{kernel}_ch{ch}"] = _case(kernel, dict(seed=400 + ch, B=20, S=S, H=(0, 25)[ch % 32 == 0]), dict(form=FORM[kernel], ch=ch, G=1, capacity=8))
    c["chunk_k1l_ch64_G8"] = _case("k1l", dict(seed=410, B=20, S=3300, H=0), dict(form="k1l_packed", ch=64, capacity=8), G=8)
    for ch in (32, 16):
        c[f"chunk_k1t_ch{ch}"] = _case("k1t", dict(seed=420 + ch, B=_ragged_B(50), S=40, H=(0, 9)[ch == 16]), dict(ch=ch), G=50, k1t_ch=ch)
    # ---- K1U: the 10-bit trace up to 1 024 rows, the wide one above, the histogram's LDS at its limit (637 states: 638 and
    #      639 were planned too until k1u_S639 of this file ran -- their counters fit 160 KB, but not next to the kernel's
    #      static arrays, and every launch failed); two segments
    for S, form in ((512, "pack10"), (513, "wide"), (637, "wide")):
        c[f"k1u_S{S}"] = _case("k1u", dict(seed=500 + S, B=233, S=S, H=(0, 40)[S == 513]), dict(form=form, pack10=form == "pack10"), G=100,
                               extra=(32_761,))
    c["k1u_G250"] = _case("k1u", dict(seed=510, B=597, S=9, H=17, rewards_range=(0.3, 1.7)), dict(form="pack10"), G=250)
    # ---- overflow lists at capacity: every transition arrives in state 0, so its one or two rows wrap their 8-bit counters
    #      30 (K1L / K1P) or 14 (K1T) times per flush period
    for kernel in PIPE:
        for A in (1, 2):
            c[f"overflow_{kernel}_A{A}"] = _case(kernel, dict(seed=600 + A, B=46, S=5, A=A, H=0, absorbing=True), dict(form=FORM[kernel]), G=20,
                                                 extra=(2 * 7680 + 1,))
    c["overflow_k1t"] = _case("k1t", dict(seed=610, B=116, S=5, H=0, absorbing=True), dict(ch=64), G=50, extra=(2 * 3584 + 1,))
    c["overflow_k1t_ch16"] = _case("k1t", dict(seed=611, B=116, S=5, H=0, absorbing=True), dict(ch=16), G=50, k1t_ch=16, extra=(2 * 3584 + 1,))
    # ---- no G knob: the planner's own G > 1 (1 100 instances over 256 CUs) -- the knob path and the planned path are one code
    for kernel, G in (("k1l", 3), ("k1p", 5), ("k1t", 5), ("k1u", 5)):
        c[f"planned_{kernel}"] = _case(kernel, dict(seed=700, B=1100, S=6, H=6, permuted=True), dict(G=G))
    return c


CASES = _cases()


# ---- batches one step past a limit: name -> (tables, knobs, kernels whose plan must be refused, BatchedMDP keywords) -------
def _edit(t, **changes):
    return dict(t, **changes)


def _non_swap():
    t = D.tables(seed=801, B=30, S=10, H=5)
    nxt = t["sp_next"].copy()
    r = 7 * 20 + 5   # one row of instance 7 leads elsewhere: no longer a swap of instance 0
    nxt[r] = (nxt[r] + 1) % 10
    return _edit(t, sp_next=nxt)


def _two_starts():
    t = D.tables(seed=802, B=12, S=6, H=4)
    off = t["start_off"].copy()
    off[5:] += 1   # instance 4 gets a second start state, state 2, with half the probability
    return _edit(t, start_off=off, start_state=np.insert(t["start_state"], 5, 2).astype(np.int32), start_cum=np.insert(t["start_cum"], 4, 0.5))


def _ragged_states():
    t = D.tables(seed=803, B=12, S=6, H=0, permuted=False)
    R = len(t["sp_next"]) - 2   # the last instance loses its last state
    cut = {k: t[k][:R] for k in ("sp_next", "sp_cum", "sp_reward", "sp_rkind", "sp_rp0", "sp_rp1", "sp_seed")}
    so = t["state_off"].copy()
    so[-1] -= 1
    return _edit(t, state_off=so, sp_ptr=t["sp_ptr"][:R + 1], **dict(cut, sp_next=np.minimum(cut["sp_next"], 4).astype(np.int32)))


def _stochastic_row():
    t = D.tables(seed=804, B=12, S=6, H=0)
    ptr = t["sp_ptr"].copy()
    ptr[31:] += 1   # row 30 gets a second entry
    dup = lambda a: np.insert(a, 30, a[30])   # noqa: E731
    return _edit(t, sp_ptr=ptr, sp_next=dup(t["sp_next"]), sp_cum=np.insert(t["sp_cum"], 30, 0.5), sp_reward=dup(t["sp_reward"]),
                 sp_rkind=dup(t["sp_rkind"]), sp_rp0=dup(t["sp_rp0"]), sp_rp1=dup(t["sp_rp1"]))


P = dict(rng_mode=L.RNG_PHILOX)
ALL = ("k1l", "k1p", "k1t", "k1u")
REFUSED = {
    "rewards257": (lambda: D.tables(seed=810, B=12, S=129, n_rew=257, H=0, permuted=False), {}, ALL, P),
    "bits16_k1p": (lambda: D.tables(seed=303, B=46, S=128, n_rew=256, H=0, permuted=True), dict(pipe=1), ALL, P),
    "bits16_k1t_k1u": (lambda: D.tables(seed=304, B=46, S=129, n_rew=128, H=6, permuted=True), {}, ("k1t", "k1u"), P),
    "S3311_k1l": (lambda: D.tables(seed=811, B=20, S=3311, H=0, permuted=False), dict(pipe=0), ALL, P),
    "S3314": (lambda: D.tables(seed=812, B=20, S=3314, H=0, permuted=False), {}, ALL, P),
    "actions3_k1t": (lambda: D.tables(seed=813, B=30, S=10, A=3, H=5, permuted=False), {}, ("k1t", "k1u"), P),
    "non_swap_row_k1t": (_non_swap, {}, ("k1t", "k1u"), P),
    "S638_k1u": (lambda: D.tables(seed=814, B=70, S=638, H=0), {}, ("k1u",), P),
    "S640_k1u": (lambda: D.tables(seed=814, B=70, S=640, H=0), {}, ("k1u",), P),
    "two_start_states": (_two_starts, {}, ALL, P),
    "ragged_states": (_ragged_states, {}, ALL, P),
    "stochastic_row": (_stochastic_row, {}, ALL, P),
    "mt_compat_two_start_states": (_two_starts, {}, ALL, dict(rng_mode=L.RNG_MT_COMPAT)),
}
REFUSED_ROLLOUT = ("rewards257", "non_swap_row_k1t")   # ... whose automatic rollout is held against the oracle


@functools.lru_cache(maxsize=None)
def _tables(name):
    return D.tables(**CASES[name].gen) if name in CASES else REFUSED[name][0]()


@functools.lru_cache(maxsize=None)
def _oracle(name, n_steps):
    t = _tables(name)
    return O.batch_rollout(t, 0, int(t["B"]), n_steps, rng_mode=1, philox_keys=D.keys(int(t["B"])), want_visits=True)


def _launches(name):
    return D.LAUNCHES + (CASES[name].extra if name in CASES else ())


def _mask(B):
    return (np.arange(B) % 3 == 0).astype(np.uint8)


def _script(name):
    """("reset", mask or None) / ("rollout", n) legs of a case"""
    legs = [("reset", None)] + [("rollout", n) for n in _launches(name)]
    if name in CASES and CASES[name].masked:
        legs.insert(1 + MASKED_AFTER, ("reset", "every_third"))
    return tuple(legs)


@functools.lru_cache(maxsize=None)
def _oracle_script(name):
    """A case with a masked reset on per-instance oracle environments: per rollout leg (last_obs, reward_sum), then visits."""
    t, script = _tables(name), _script(name)
    B, A, S = int(t["B"]), int(t["A"]), int(t["state_off"][1])
    keys, mask = D.keys(B), _mask(B)
    n_legs = sum(op == "rollout" for op, _ in script)
    last, rsum, vs, vsa = np.zeros((n_legs, B), np.int32), np.zeros((n_legs, B), np.float64), [], []
    for b in range(B):
        rows = slice(b * S * A, (b + 1) * S * A)
        m = types.SimpleNamespace(
            sp_ptr=np.arange(S * A + 1), sp_next=t["sp_next"][rows], sp_cum=t["sp_cum"][rows], sp_rkind=t["sp_rkind"][rows],
            sp_rp0=t["sp_reward"][rows], sp_rmean=t["sp_reward"][rows], sp_seed=t["sp_seed"][rows], start_states=t["start_state"][b:b + 1],
            start_probs=np.ones(1), n_states=S, n_actions=A, H=int(t["H"]), rewards_range=t["rewards_range"], start_seed=0,
            deterministic_rewards=True)
        e = O.OracleEnv(m, rng_mode=1, philox_key=int(keys[b]))
        k = 0
        for op, arg in script:
            if op == "reset":
                if arg is None or mask[b]:
                    e.reset()
            else:
                r = e.rollout(arg, trace=False)
                last[k, b], rsum[k, b] = r["last_obs"], r["reward_sum"]
                k += 1
        v = e.visits()
        vs.append(np.asarray(v[0]).ravel())
        vsa.append(np.asarray(v[1]).ravel())
    return last, rsum, np.concatenate(vs), np.concatenate(vsa)


def _check_plan(name, plan):
    """The part of the plan the case's kernel runs by: eligible, the fields the case names, and the form the kernel implies."""
    c = CASES[name]
    p = plan[KERNEL[c.kernel][1]]
    assert p["ok"], (name, plan)
    want = dict(c.want)
    if want.get("G") == "capacity":
        want["G"] = p["capacity"]
    if c.kernel in PIPE:
        want.update(pipe=bool(PIPE[c.kernel]), packed=want.get("form", FORM[c.kernel]) != "k1l_unpacked")
        assert p["form"] in (("k1p",) if c.kernel == "k1p" else ("k1l_packed", "k1l_unpacked"))
    if c.kernel == "k1u":
        assert p["form"] == ("pack10" if p["pack10"] else "wide") and p["ch"] == (72 if p["pack10"] else 64)
    assert {k: p[k] for k in want} == want, (name, p)
    assert 1 <= p["G"] <= p["capacity"] <= KERNEL[c.kernel][4]
    return p


# ---- host only: the generator and the planners on the bare description ------------------------------------------------------
def test_generator_covers_what_it_claims():
    d = D.describe(_tables("episodes_k1t_H3"))
    assert d["swaps_only"] and d["swapped_states"] > 100 and d["n_rew"] == d["n_rew_instance0"] == 3 and d["negative_rewards"] >= 1
    assert d["dyadic_rewards"] == 0 and len(d["start_states"]) == 1 and d["start_states"][0] != 0
    d = D.describe(_tables("episodes_k1l_packed_H8"))
    assert not d["swaps_only"] and len(d["start_states"]) == 5 and 0 not in d["start_states"]
    assert D.describe(_tables("episodes_k1t_H8"))["start_states"] == [1, 2, 3, 4, 5]   # K1T reads the start state per instance
    assert D.describe(_tables("bits17_S129_rewards256")) ["n_rew"] == 256 and D.describe(_tables("bits15_k1u"))["n_rew_instance0"] == 128
    assert D.describe(_tables("rewards257"))["n_rew"] == 257
    assert D.describe(_tables("k1u_S512"))["max_row_index"] == 1023 and D.describe(_tables("k1u_S513"))["max_row_index"] == 1025
    assert D.describe(_tables("one_reward_k1t"))["n_rew"] == 1 and D.describe(_tables("one_row_k1l"))["rows"] == 1
    assert not D.describe(_tables("non_swap_row_k1t"))["swaps_only"]
    for name, c in CASES.items():
        d = D.describe(_tables(name))
        assert d["n_rew"] == c.gen.get("n_rew", 3) and d["dyadic_rewards"] == 0 and d["rows"] == c.gen["S"] * c.gen.get("A", 2)
        assert d["swaps_only"] or not c.gen["permuted"]
        assert d["all_lead_to_0"] == (bool(c.gen.get("absorbing")) or c.gen["S"] == 1)
        lo, hi = c.gen.get("rewards_range", (0.0, 1.0))
        assert lo < _tables(name)["sp_reward"].min() and _tables(name)["sp_reward"].max() < hi and (d["negative_rewards"] > 0) == (lo < 0)
    assert {c.gen.get("rewards_range") for c in CASES.values()} >= {None, (-2.5, 4.0), (0.3, 1.7)}
    for kernel in KERNEL:   # every kernel sees both other ranges and per-instance start states
        mine = [c.gen for c in CASES.values() if c.kernel == kernel]
        assert {g.get("rewards_range") for g in mine} >= {(-2.5, 4.0), (0.3, 1.7)} and any(g.get("start") == "per_instance" for g in mine)


@pytest.mark.parametrize("name", list(CASES))
def test_plan_of_description(name):
    """The case lands in the form it names (cmdp_det_plan_desc: no handle, no device), and its workgroup fits LDS: at the
    capacity the plan reports it stays within the budget of its candidate, one more instance would not, unless the
    capacity is the kernel's lane limit."""
    c, t = CASES[name], _tables(name)
    p = _check_plan(name, det_plan_of_tables(t, CUS, **c.knobs))
    part, knob, lanes = KERNEL[c.kernel][1], KERNEL[c.kernel][3], KERNEL[c.kernel][4]
    full = det_plan_of_tables(t, CUS, **dict(c.knobs, **{knob: CAPACITY}))[part]
    less = det_plan_of_tables(t, CUS, **dict(c.knobs, **{knob: full["capacity"] - 1}))[part]
    assert full["G"] == full["capacity"] == p["capacity"] and less["G"] == full["G"] - 1
    budget = LDS // full.get("per_cu", 1)
    assert p["lds_bytes"] <= full["lds_bytes"] <= budget
    assert full["capacity"] == lanes or 2 * full["lds_bytes"] - less["lds_bytes"] > budget
    if c.kernel == "k1u":
        assert p["hist_lds_bytes"] <= LDS


def test_every_form_is_in_the_matrix():
    plans = {name: det_plan_of_tables(_tables(name), CUS, **c.knobs)[KERNEL[c.kernel][1]] for name, c in CASES.items()}
    of = lambda kernel, key: {plans[n][key] for n, c in CASES.items() if c.kernel == kernel}   # noqa: E731
    assert of("k1l", "form") | of("k1p", "form") == set(L.K1LP_FORMS.values()) and of("k1u", "form") == set(L.K1U_FORMS.values())
    assert of("k1u", "pack10") == {True, False}
    assert of("k1l", "ch") == {256, 128, 112, 64} and of("k1p", "ch") == {64, 32, 16} and of("k1t", "ch") == {64, 32, 16}
    assert of("k1u", "ch") == {72, 64} and of("k1l", "per_cu") == {1, 2}
    groups = {}   # form -> the (G, capacity) pairs it runs at
    for n, c in CASES.items():
        groups.setdefault(plans[n]["form"] if c.kernel in PIPE else c.kernel, set()).add((plans[n]["G"], plans[n]["capacity"]))
    assert set(groups) == {"k1l_packed", "k1l_unpacked", "k1p", "k1t", "k1u"}
    for form, seen in groups.items():
        assert any(G == 1 for G, cap in seen) and any(G == cap for G, cap in seen), (form, seen)
    assert {(64, 64)} <= groups["k1l_packed"] & groups["k1p"] and (128, 128) in groups["k1t"] and (256, 256) in groups["k1u"]
    masked = {(c.kernel, plans[n].get("form")) for n, c in CASES.items() if c.masked}
    assert masked == {("k1l", "k1l_packed"), ("k1l", "k1l_unpacked"), ("k1p", "k1p"), ("k1t", None), ("k1u", "pack10")}


@pytest.mark.parametrize("name", list(REFUSED))
def test_planner_refuses_one_past_the_limit(name):
    make, knobs, kernels, kw = REFUSED[name]
    plan = det_plan_of_tables(_tables(name), CUS, **knobs, **kw)
    for kernel in ALL:
        p = plan[KERNEL[kernel][1]]
        if kernel in kernels:
            assert not p["ok"] and p["G"] == 0 and p.get("form") is None, (name, kernel, p)
        else:
            assert p["ok"], (name, kernel, p)


def test_the_batch_before_every_limit_is_planned():
    """The other side of the refusals: the last size that still has a plan."""
    big = lambda S: D.tables(seed=811, B=20, S=S, H=0, permuted=False)   # noqa: E731
    assert det_plan_of_tables(big(3310), CUS, pipe=0)["k1lp"]["ch"] == 64 and not det_plan_of_tables(big(3311), CUS, pipe=0)["k1lp"]["ok"]
    p = det_plan_of_tables(big(3313), CUS)["k1lp"]
    assert (p["form"], p["ch"], p["capacity"]) == ("k1p", 16, 8) and not det_plan_of_tables(big(3314), CUS)["k1lp"]["ok"]
    p = det_plan_of_tables(D.tables(seed=814, B=70, S=637, H=0), CUS)   # 64 odd strides of dwords + start_of[64], resets_of[64]
    assert p["k1u"]["ok"] and p["k1u"]["hist_lds_bytes"] == 64 * 4 * 637 + 512 <= LDS < 64 * 4 * 639 + 512
    p = det_plan_of_tables(D.tables(seed=814, B=70, S=638, H=0), CUS)
    assert p["k1t"]["ok"] and not p["k1u"]["ok"]
    assert det_plan_of_tables(D.tables(seed=810, B=12, S=129, n_rew=256, H=0, permuted=False), CUS)["k1lp"]["form"] == "k1l_unpacked"
    t = D.tables(seed=802, B=12, S=6, H=4)
    assert det_plan_of_tables(t, CUS, rng_mode=L.RNG_MT_COMPAT) == det_plan_of_tables(t, CUS)   # no MT19937 stream: planned alike
    assert det_plan_of_tables(t, CUS, k1t_ch=16)["k1t"]["ch"] == 16 and not det_plan_of_tables(t, CUS, k1t_ch=48)["k1t"]["ok"]
    with pytest.raises(L.CmdpError) as e:
        det_plan_of_tables(dict(t, sp_next=t["sp_next"] + 6), CUS)
    assert e.value.code == L.ERR_INVALID


# (B, S) -> cus -> (K1L / K1P form, ch, G, workgroups per CU), (K1T ch, G, automatic), (K1U ok, G, automatic): with fewer CUs
# the batch needs rounds of workgroups, and the cost models trade chunk length and kernel for fewer of them
PLANS_BY_CUS = {
    (200, 6): {1: (("k1l_packed", 256, 50, 2), (64, 100, True), (True, 200, True)),
               4: (("k1p", 64, 50, 1), (64, 50, False), (True, 50, False)),
               256: (("k1p", 64, 1, 1), (64, 1, False), (True, 1, False))},
    (200, 600): {1: (("k1p", 32, 40, 1), (32, 100, True), (True, 200, True)),
                 4: (("k1p", 64, 25, 1), (64, 50, True), (True, 50, False)),
                 256: (("k1p", 64, 1, 1), (64, 1, False), (True, 1, False))},
    (200, 1500): {1: (("k1p", 32, 17, 1), (64, 40, True), (False, 0, False)),
                  4: (("k1p", 32, 17, 1), (64, 25, True), (False, 0, False)),
                  256: (("k1p", 64, 1, 1), (64, 1, False), (False, 0, False))},
    (2000, 40): {1: (("k1l_packed", 256, 63, 2), (64, 125, True), (True, 250, True)),
                 4: (("k1l_packed", 256, 63, 2), (64, 125, True), (True, 250, True)),
                 256: (("k1p", 64, 8, 1), (64, 8, False), (True, 8, False))},
}


@pytest.mark.parametrize("shape", list(PLANS_BY_CUS))
def test_plans_at_other_cu_counts(shape):
    B, S = shape
    t = D.tables(seed=900, B=B, S=S, H=0)
    for cus, (lp, kt, ku) in PLANS_BY_CUS[shape].items():
        p = det_plan_of_tables(t, cus)
        assert (p["k1lp"]["form"], p["k1lp"]["ch"], p["k1lp"]["G"], p["k1lp"]["per_cu"]) == lp, (shape, cus, p["k1lp"])
        assert p["k1t"]["ok"] and (p["k1t"]["ch"], p["k1t"]["G"], p["k1t"]["automatic"]) == kt, (shape, cus, p["k1t"])
        assert (p["k1u"]["ok"], p["k1u"]["G"], p["k1u"]["automatic"]) == ku, (shape, cus, p["k1u"])
        for part in ("k1lp", "k1t", "k1u"):   # even_groups never plans more than fit
            assert p[part]["G"] <= p[part]["capacity"] and p[part]["lds_bytes"] <= LDS // p[part].get("per_cu", 1)


def test_absorbing_cases_fill_the_overflow_lists():
    """The premise of the counter-wrap cases, from the oracle's visit counts: the rows of state 0 take all but a handful of
    the transitions, so a flush period wraps the 8-bit counters of an instance 30 (14) times, and the unpacked form's
    16-bit half of an only row collects a whole period of 32 768."""
    names = [n for n, c in CASES.items() if c.gen.get("absorbing")]
    assert len(names) == 7
    for name in names:
        t = _tables(name)
        A, S, total = int(t["A"]), int(t["state_off"][1]), int(sum(_launches(name)))
        _, _, _, vsa = _oracle(name, total)
        assert (vsa.reshape(int(t["B"]), S * A)[:, :A].sum(axis=1) >= total - 1).all()


# ---- GPU ------------------------------------------------------------------------------------------------------------------
def _create(tables, knobs, **kw):
    saved = {k: os.environ.pop(k, None) for k in KNOBS}
    os.environ.update({ENV[k]: str(v) for k, v in knobs.items()})
    try:
        return BatchedMDP(tables=tables, philox_keys=D.keys(int(tables["B"])), **(kw or P))
    finally:
        for k in KNOBS:
            os.environ.pop(k, None)
        os.environ.update({k: v for k, v in saved.items() if v is not None})


def _run(tables, knobs, which, script, check=None):
    """The legs of the script on one handle: per rollout leg (last_obs, reward_sum), then visits, state and starts."""
    env = _create(tables, knobs)
    try:
        env.set_rollout_kernel(which)
        if check is not None:
            check(env)
        last, rsum, h_seen = [], [], None
        for op, arg in script:
            if op == "reset":
                env.reset(None if arg is None else _mask(env.B))
                h_seen = env.state()[1] if arg is not None else h_seen
            else:
                out = env.rollout(arg)
                last.append(out["last_obs"])
                rsum.append(out["reward_sum"])
        vs, vsa = env.visits()
        cur, h, need_reset = env.state()
        last_start = env.last_start()
        return dict(last=last, rsum=rsum, vs=vs, vsa=vsa, cur=cur, h=h, need_reset=need_reset, last_start=last_start,
                    previous_start=env.previous_start, h_after_mask=h_seen)
    finally:
        env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_forced_kernel_equals_k1_and_oracle(need_gpu, name):
    c, t, script = CASES[name], _tables(name), _script(name)
    which, part, kernel_name = KERNEL[c.kernel][:3]
    total = int(sum(_launches(name)))

    def check(env):
        plan = env.det_plan()
        p = _check_plan(name, plan)
        assert plan == det_plan_of_tables(t, CUS, **c.knobs)   # (a 256-CU device)
        lp = env.lds_plan()
        assert (lp["eligible"], lp["kernel"], lp["instances_per_workgroup"], lp["chunk"]) == (True, kernel_name, p["G"], p["ch"])

    s = _run(t, c.knobs, which, script, check)
    g = _run(t, c.knobs, L.ROLLOUT_GLOBAL, script)
    for i in range(len(s["last"])):
        assert np.array_equal(s["last"][i], g["last"][i]), (name, i)
        assert np.array_equal(s["rsum"][i], g["rsum"][i]), (name, i)
    for k in ("vs", "vsa", "cur", "h", "need_reset", "last_start", "previous_start"):
        assert np.array_equal(s[k], g[k]), (name, k)
    if c.masked:   # one workgroup holds instances at different in-episode times: the per-lane flavour, with terminations
        G = det_plan_of_tables(t, CUS, **c.knobs)[part]["G"]
        assert len(set(s["h_after_mask"][:G].tolist())) > 1 and int(t["H"]) > 0
        last, rsum, vs, vsa = _oracle_script(name)
        for i in range(len(s["last"])):
            assert np.array_equal(s["last"][i], last[i]), (name, i)
        rsum_total = rsum.sum(axis=0)
        last = last[-1]
    else:
        last, rsum_total, vs, vsa = _oracle(name, total)   # every instance
    assert np.array_equal(s["last"][-1], last) and np.array_equal(s["cur"], last)
    assert np.array_equal(s["vs"], vs) and np.array_equal(s["vsa"], vsa)
    assert vs.sum() >= t["B"] * total and vsa.sum() == t["B"] * total
    np.testing.assert_allclose(np.sum(s["rsum"], axis=0), rsum_total, rtol=1e-12, atol=0)
    # one launch from reset: the float64 sum in the oracle's order
    last, rsum, vs, vsa = _oracle(name, total)
    one = _run(t, c.knobs, which, (("reset", None), ("rollout", total)))
    assert np.array_equal(one["rsum"][0], rsum) and np.array_equal(one["last"][0], last)
    assert np.array_equal(one["vs"], vs) and np.array_equal(one["vsa"], vsa)
    assert len(np.unique(rsum)) > 1 or c.gen.get("n_rew", 3) == 1


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(REFUSED))
def test_refused_batches_fail_when_forced(need_gpu, name):
    make, knobs, kernels, kw = REFUSED[name]
    t = _tables(name)
    env = _create(t, knobs, **kw)
    try:
        plan = env.det_plan()
        assert plan == det_plan_of_tables(t, CUS, **knobs, **kw)
        env.reset()
        for which in sorted({KERNEL[k][0] for k in kernels}):
            env.set_rollout_kernel(which)
            with pytest.raises(L.CmdpError) as e:
                env.rollout(64)
            assert e.value.code == L.ERR_UNSUPPORTED, (name, which)
    finally:
        env.close()
    if name in REFUSED_ROLLOUT:
        a = _run(t, knobs, L.ROLLOUT_AUTO, _script(name))
        last, rsum, vs, vsa = _oracle(name, int(sum(D.LAUNCHES)))
        assert np.array_equal(a["last"][-1], last) and np.array_equal(a["vs"], vs) and np.array_equal(a["vsa"], vsa)
        np.testing.assert_allclose(np.sum(a["rsum"], axis=0), rsum, rtol=1e-12, atol=0)


@pytest.mark.gpu
def test_previous_start_after_terminations_on_every_lds_kernel(need_gpu):
    """K1 records the start state of the reset before the latest one at every termination (BaseMDP's bookkeeping, which the
    logged loop reads).  With a start state other than 0 the LDS-resident kernels, K1E among them, have to leave the same
    behind: they left 0 until the episodic cases of this file ran."""
    name = "episodes_k1t_H9"
    t, script = _tables(name), _script(name)
    assert int(t["start_state"][0]) != 0 and len(set(t["start_state"].tolist())) == 1
    g = _run(t, {}, L.ROLLOUT_GLOBAL, script)
    assert (g["previous_start"] == t["start_state"]).all() and (g["last_start"] == t["start_state"]).all()
    for which in (L.ROLLOUT_LDS, L.ROLLOUT_LDS_TEMPLATE, L.ROLLOUT_LDS_TEMPLATE_STREAM, L.ROLLOUT_EPISODE_PARALLEL):
        s = _run(t, {}, which, script)
        for k in ("last", "rsum", "vs", "vsa", "cur", "h", "need_reset", "last_start", "previous_start"):
            assert np.array_equal(s[k], g[k]), (which, k)
    before = _run(t, {}, L.ROLLOUT_LDS, script[:2])   # one transition, no termination yet: the handle's initial 0
    assert (before["previous_start"] == 0).all()
