"""Test helper: the twins of helpers_psrlc / helpers_psrlo with the reference's min_steps_before_new_episode
(posterior_sampling.py:346-358).  tests/test_psrlc_gate.py holds them against the reference's own runs (golden G24) step for
step, which is what entitles tests/test_gpu_psrlc_gate.py to use them as the reference of the device's gate on the GPU box."""
import numpy as np

from helpers_psrlc import PSRLCTwin, StampedRule
from helpers_psrlo import PSRLOTwin


class _Gate:
    """is_episode_end with the gate: `time` is mdp.h read before the step (agent_mdp_interaction.py:243, :259)."""

    min_steps = 0
    last_change = 0

    def is_episode_end(self, s, a, time):
        if time - self.last_change < self.min_steps:
            return False
        self.last_change = time
        return super().is_episode_end(s, a)


class GatedPSRLCTwin(_Gate, PSRLCTwin):
    def __init__(self, *a, min_steps=0, **kw):
        super().__init__(*a, **kw)
        self.min_steps, self.last_change = int(min_steps), 0


class GatedPSRLOTwin(_Gate, PSRLOTwin):
    def __init__(self, *a, min_steps=0, **kw):
        super().__init__(*a, **kw)
        self.min_steps, self.last_change = int(min_steps), 0


class GatedStampedRule(StampedRule):
    """The device's form of the rule with the gate (csrc/cmdp_psrlc.h: PcGate): the counters move on every visit, the rule is
    evaluated only by a check that passes."""

    def __init__(self, S, A, min_steps):
        super().__init__(S, A)
        self.min_steps, self.last_change = int(min_steps), 0

    def visit(self, s, a, time):
        rule = super().visit(s, a)
        if time - self.last_change < self.min_steps:
            return False
        self.last_change = time
        return rule


def gate_schedule(pairs, S, A, min_steps, h0=0, rule=None):
    """The gated rule fed a trajectory's (s, a) pairs from in-run time `h0` on: (ended [n] bool, the rule).  An episode that
    ends is followed by its episode_end_update, as in the walk."""
    rule = rule or GatedStampedRule(S, A, min_steps)
    ended = np.zeros(len(pairs), bool)
    for t, (s, a) in enumerate(pairs):
        ended[t] = rule.visit(int(s), int(a), h0 + t)
        if ended[t]:
            rule.episode_end_update()
    return ended, rule
