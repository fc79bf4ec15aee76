"""The reference's seven learners as one table, keyed by their directory names under ``isaacgymenvs/``
(``experiments.sh`` runs each over 16 POMDP settings).  They differ in five things only, each read from the
directory's ``main.py`` / ``model.py`` (line numbers per row below): the actor (MLP or LSTM), whether the "new to
RPO" branch of ``model.py`` is live (``rpo_alpha`` in the update), which observation the policy acts on, which the
critic values and bootstraps on, and the names of the run and of the checkpoints.  Every learner's actor trains on
the POMDP observations.

``acts_on`` / ``critic_on`` are ``"clean"`` or ``"pomdp"``.  ``critic_on == "pomdp"`` is the single-stream routing
of PPO/main.py:87-96 and RPO/main.py:87-96: ``next_obs = POMDP.observation(next_obs)`` replaces the observation
itself, so the stored ``obs``, the policy input, the values and the GAE bootstrap are all the corrupted one and no
separate ``pomdps`` buffer exists.  In every variant the first observation of a run is the clean ``envs.reset()``
result (``pomdp = next_obs`` before the loop, main.py:80-82) and the POMDP wrapper is called once per step.

The names are format strings over ``P`` (``args.POMDP``) and ``p`` (``args.pomdp_prob``): ``run`` is both the
``SummaryWriter`` directory and the final checkpoint prefix, ``best`` the best-reward checkpoint prefix.
``tests/golden/learner_variants.json`` holds the same table as data, generated from the reference's text.
"""
from collections import namedtuple

Variant = namedtuple("Variant", "recurrent rpo_alpha acts_on critic_on run best")

# experiments.sh order (its `cd` lines 4, 31, 58, 85, 112, 139, 166)
VARIANTS = {
    # PPO/model.py:34-36 (RPO branch commented out); main.py:91 getAction(next_obs), :96 next_obs = POMDP...;
    # :106 train(obs, ...); names :39, :112, :114
    "PPO": Variant(False, 0.0, "pomdp", "pomdp", "PPO_{P}_{p}", "PPO_best_{P}_{p}"),
    # RPO/model.py:14, 34-36 (live); main.py:91, :96, :106; names :39, :112, :114
    "RPO": Variant(False, 0.5, "pomdp", "pomdp", "RPO_{P}_{p}", "RPO_best_{P}_{p}"),
    # PPO-LSTM/model.py:63-65 (commented out); main.py:98 getAction(next_obs, ...), :103 pomdp = POMDP...,
    # :112 train(obs, pomdps, ...); names :39, :118, :121
    "PPO-LSTM": Variant(True, 0.0, "clean", "clean", "PPO_LSTM_{P}_{p}", "PPO_LSTM_best_{P}_{p}"),
    # RPO-LSTM_Critic/model.py:14, 63-65 (live); main.py:98 getAction(pomdp, ...), :103, :112; names :39, :118, :121
    "RPO-LSTM_Critic": Variant(True, 0.5, "pomdp", "clean", "RPO_LSTM_Critic_{P}_{p}",
                               "RPO_LSTM_Critic_best_{P}_{p}"),
    # PPO_Critic/model.py:34-36 (commented out); main.py:93 getAction(pomdp), :98, :107 train(obs, pomdps, ...);
    # names :37, :113 (best_{P}_{p}: no learner prefix), :115
    "PPO_Critic": Variant(False, 0.0, "pomdp", "clean", "PPO_Critic_{P}_{p}", "best_{P}_{p}"),
    # RPO_Critic/model.py:14, 34-36 (live); main.py:93, :98, :107; names :37, :113, :115
    "RPO_Critic": Variant(False, 0.5, "pomdp", "clean", "RPO_Critic_{P}_{p}", "RPO_Critic_best_{P}_{p}"),
    # RPO-LSTM/model.py:14, 63-65 (live); main.py:98 getAction(next_obs, ...), :103, :112; names :39, :118, :121
    "RPO-LSTM": Variant(True, 0.5, "clean", "clean", "RPO_LSTM_{P}_{p}", "best_reward_{P}_{p}"),
}
LEARNERS = tuple(VARIANTS)

# experiments.sh: the same 16 settings for every learner
GRID = (("flicker", (0.1, 0.2, 0.3, 0.4, 0.5)),
        ("random_noise", (0.05, 0.1, 0.15, 0.2, 0.25, 0.23)),
        ("flickering_and_random_noise", (0.05, 0.1, 0.15, 0.2, 0.25)))


def legacy_variant(algo, rollout_obs):
    """``train.py --algo {rpo_lstm, ppo} --rollout_obs {clean, pomdp}`` as a row: each actor's default ``rpo_alpha``
    (None), the critic on the clean observations with the separate ``pomdps`` storage, the names those flags have
    always written.  Not one of the reference's seven (``--algo ppo --rollout_obs clean`` matches none of them)."""
    recurrent = algo == "rpo_lstm"
    return Variant(recurrent, None, rollout_obs, "clean", ("RPO_LSTM" if recurrent else "PPO") + "_{P}_{p}",
                   "best_reward_{P}_{p}")


def names(learner, pomdp, prob):
    """(run and final-checkpoint name, best-checkpoint name) of ``learner`` (a key of ``VARIANTS``, or a row) at
    this POMDP setting."""
    v = VARIANTS[learner] if isinstance(learner, str) else learner
    return v.run.format(P=pomdp, p=prob), v.best.format(P=pomdp, p=prob)


def single_stream(v):
    """PPO / RPO: the corrupted observation replaces the observation (no separate ``pomdps`` storage)."""
    return v.critic_on == "pomdp"
