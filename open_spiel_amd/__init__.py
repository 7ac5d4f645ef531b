"""open_spiel_amd — MI355X-native batched game-step and search engine.

A from-scratch HIP (gfx950) implementation of OpenSpiel's data-parallel hot
path: batched LegalActions / ApplyAction / IsTerminal / Returns /
ObservationTensor for tic_tac_toe, connect_four, hex, kuhn_poker and
leduc_poker, random-rollout evaluation, MCTS, information-set MCTS and alpha-beta search over batches of roots, and
tabular CFR / Discounted CFR / external-sampling MCCFR / extensive-form fictitious play /
magnetic mirror descent / extensive-form regret minimization, payoff tensors / policy aggregation / PSRO over populations of policies, and PSRO's
meta-strategy solvers (projected replicator dynamics, regret matching) on batches of normal-form meta-games, and
AlphaZero self-play (policy targets, moves, trajectories and a replay buffer on the device), and Deep CFR (traversals,
sampled advantages and reservoir buffers on the device; the networks are torch's), and NFSP / DQN self-play (episodes,
transitions, supervised rows, the replay ring and the reservoirs on the device).
The C-ABI is include/osg_abi.h.
"""
from ._abi import OsgError, describe, lib  # noqa: F401


def _load_torch_runtime_first():
    """PyTorch-ROCm ships its own HIP/HSA runtime under torch/lib.  Two HSA runtimes in one
    process do not work (the second one finds no device), so whenever torch is installed its
    runtime is loaded BEFORE libosg_hip.so / the pybind module, which then bind to the same
    libamdhip64.so.7 by SONAME."""
    try:
        import torch  # noqa: F401
    except ImportError:
        pass


def __getattr__(name):
    if name == "pyspiel_hip":
        import importlib
        _load_torch_runtime_first()
        return importlib.import_module(".pyspiel_hip", __name__)
    # torch-backed classes are imported lazily so that `import open_spiel_amd`
    # (and the ABI symbol check) works without touching torch.
    if name in ("Context", "Game", "StateBatch", "SolvedGame", "TabularSolver", "DCFRSolver", "LCFRSolver", "XFPSolver", "MMDSolver", "EFRSolver"):
        from . import engine
        return getattr(engine, name)
    if name == "PSROSolver":
        from . import psro
        return psro.PSROSolver
    if name in ("meta_solvers", "solve_meta_games", "solve_alpharank"):   # (the reference-named solvers: by the module)
        import importlib
        module = importlib.import_module(".meta_solvers", __name__)
        return module if name == "meta_solvers" else getattr(module, name)
    if name in ("ISMCTSBot", "ISMCTSFinalPolicyType", "ChildSelectionPolicy"):
        from . import ismcts
        return getattr(ismcts, name)
    if name in ("SelfPlay", "ReplayBuffer", "TrainInput"):
        from . import alpha_zero
        return getattr(alpha_zero, name)
    if name in ("DeepCFRSolver", "ReservoirBuffer", "deep_cfr"):   # (ReservoirBuffer: Deep CFR's; AlphaZero's ring is ReplayBuffer)
        import importlib
        module = importlib.import_module(".deep_cfr", __name__)
        return module if name == "deep_cfr" else getattr(module, name)
    if name in ("NFSPSolver", "TransitionRing", "nfsp"):
        import importlib
        module = importlib.import_module(".nfsp", __name__)
        return module if name == "nfsp" else getattr(module, name)
    if name in ("BatchedEnvironment", "TimeStep", "StepType", "ObservationType"):
        from . import vector_env
        return getattr(vector_env, name)
    raise AttributeError(name)
