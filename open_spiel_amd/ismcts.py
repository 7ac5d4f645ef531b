"""ISMCTSBot: information-set MCTS (open_spiel/python/algorithms/ismcts.py) for kuhn_poker and leduc_poker on the device.

    bot = ISMCTSBot("leduc_poker", uct_c=2.0, max_simulations=1000, seed=7)
    policy, action = bot.step_with_policy(state)     # state: a mirror State (anything with history()), or a history

The search is StateBatch.ismcts_search (osg_ismcts_search of include/osg_abi.h) over a 1-row batch into which the state's
history is replayed; the evaluator is RandomRolloutEvaluator(n_rollouts) on the device and the resampler the games' own
ResampleFromInfostate.  Every draw of a search comes from the stream Rng(seed, index, 0); `index` advances by one per
search, so successive calls are independent and a run is reproducible from (seed, first index).  For many states at once
call StateBatch.ismcts_search directly.

Not offered (ValueError): use_observation_string, allow_inconsistent_action_sets, an evaluator other than the built-in
random rollouts, a resampler callback.
"""
import enum

import torch

from .engine import Context, StateBatch

UNLIMITED_NUM_WORLD_SAMPLES = -1
INVALID_ACTION = -1


class ISMCTSFinalPolicyType(enum.Enum):
    NORMALIZED_VISITED_COUNT = 1
    MAX_VISIT_COUNT = 2
    MAX_VALUE = 3


class ChildSelectionPolicy(enum.Enum):
    UCT = 1
    PUCT = 2


class ISMCTSBot:
    def __init__(self, game, uct_c, max_simulations, max_world_samples=UNLIMITED_NUM_WORLD_SAMPLES, seed=0,
                 final_policy_type=ISMCTSFinalPolicyType.MAX_VISIT_COUNT, child_selection_policy=ChildSelectionPolicy.UCT,
                 n_rollouts=1, evaluator=None, use_observation_string=False, allow_inconsistent_action_sets=False,
                 index=0, max_nodes=0, ctx=None):
        if evaluator is not None:
            raise ValueError("ISMCTSBot evaluates with RandomRolloutEvaluator(n_rollouts) on the device; custom evaluators are not offered")
        if use_observation_string:
            raise ValueError("ISMCTSBot keys nodes by InformationStateString; use_observation_string is not offered")
        if allow_inconsistent_action_sets:
            raise ValueError("allow_inconsistent_action_sets is not offered (the legal actions of kuhn_poker and leduc_poker "
                             "follow from the information state)")
        self.game_string = str(game)
        self.ctx = ctx if ctx is not None else Context(torch.cuda.current_device() if torch.cuda.is_available() else 0)
        self.uct_c = float(uct_c)
        self.max_simulations = int(max_simulations)
        self.max_world_samples = int(max_world_samples)
        self.final_policy_type = ISMCTSFinalPolicyType(getattr(final_policy_type, "value", final_policy_type))
        self.child_selection_policy = ChildSelectionPolicy(getattr(child_selection_policy, "value", child_selection_policy))
        self.n_rollouts = int(n_rollouts)
        self.seed, self.index, self.max_nodes = int(seed), int(index), int(max_nodes)
        self._batch = StateBatch(self.ctx, self.game_string, 1)
        self.last_search = None   # the dict of the last ismcts_search (host copies)

    def set_resampler(self, cb):
        raise ValueError("ISMCTSBot resamples with the games' own ResampleFromInfostate; resampler callbacks are not offered")

    def reset(self):
        self.last_search = None

    def _load(self, state):
        history = [int(a) for a in (state.history() if hasattr(state, "history") else state)]
        self._batch.reset()
        for a in history:
            self._batch.apply_actions([a])
        return int(self._batch.current_player().cpu()[0])

    def _search(self, state):
        """(policy list in the reference's order, sampled action) of one search; None at a chance node."""
        if self._load(state) == -1:
            return None
        r = self._batch.ismcts_search(self.uct_c, self.max_simulations, self.n_rollouts, max(self.max_world_samples, 0),
                                      self.final_policy_type, self.child_selection_policy is ChildSelectionPolicy.PUCT,
                                      self.max_nodes, self.seed, self.index)
        self.index += 1
        r = {k: v.cpu().numpy()[0] for k, v in r.items()}
        self.last_search = r
        if r["status"] != 0:
            raise AssertionError("ISMCTSBot: " + {1: "the root was never visited (max_simulations = 1 only evaluates it)",
                                                  2: "the node table is full (max_nodes)",
                                                  3: "the state is not one of the game"}[int(r["status"])])
        legal = [a for a in range(len(r["policy"])) if (int(self._batch.legal_actions_mask_bits().cpu()[0, 0]) >> a) & 1]
        if int(r["nodes"]) == 0:   # a single legal action: no search
            return [(legal[0], 1.0)], int(r["sampled_action"])
        expanded = sorted((a for a in legal if r["expansion_rank"][a] >= 0), key=lambda a: r["expansion_rank"][a])
        order = expanded + [a for a in legal if r["expansion_rank"][a] < 0]
        return [(a, float(r["policy"][a])) for a in order], int(r["sampled_action"])

    def run_search(self, state):
        found = self._search(state)
        return [(INVALID_ACTION, 1.0)] if found is None else found[0]

    def get_policy(self, state):
        return self.run_search(state)

    def step_with_policy(self, state):
        found = self._search(state)
        return ([(INVALID_ACTION, 1.0)], INVALID_ACTION) if found is None else found

    def step(self, state):
        return self.step_with_policy(state)[1]
