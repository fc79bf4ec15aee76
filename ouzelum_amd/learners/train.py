"""Recurrent PPO / RPO-LSTM training driver on the HIP env (RPO-LSTM/main.py:28-124, PPO/main.py).

    python -m ouzelum_amd.learners.train --env Landing --num_envs 4096 --POMDP flicker --pomdp_prob 0.1

The reference's loop, once for every learner: a T-step rollout with the LSTM carry reset on done (``Rollout``, which
``scripts/bench_learner.py`` times too), one PPO update per rollout, best/final checkpoints under the reference's file
names.  What differs between learners is a row of ``variants.py``: the actor (MLP / LSTM), ``rpo_alpha`` in the
update, which observation the policy acts on and the critic values, and the names of the run directory, the final
and the best checkpoint.  ``--learner NAME`` picks one of the reference's seven by its directory name (``PPO``,
``RPO``, ``PPO-LSTM``, ``RPO-LSTM_Critic``, ``PPO_Critic``, ``RPO_Critic``, ``RPO-LSTM``), so curves and checkpoints
lie over the reference's; ``--algo`` / ``--rollout_obs`` (the older flags, not to be combined with ``--learner``) make
a row of their own (``variants.legacy_variant``): the actor acts on the clean observations and trains on the
learner-side POMDP ones (App. B item 10), ``--rollout_obs pomdp`` gives the RPO-LSTM_Critic routing.

The reference's TensorBoard scalars (PPO/main.py:101-109: ``charts/episodic_return``, ``charts/episodic_length``,
``average/average_reward``) go to a TensorBoard event file in ``<logdir>/<run>/`` (the reference's
``SummaryWriter("../runs/<run>")``; written by ``tbevents.py``, tensorboard itself is not installed), by default one
point per rollout: the mean return / length of the episodes that finished in it, from the env's in-kernel
[sum, count] (``ouz_episode_stats``), all-reduced over RCCL when launched with torchrun (one process per GPU, env ids
sharded).  Every logged column also goes to ``<logdir>/<run>.csv``.

The per-step episode bookkeeping is one ``ouz_episode_step`` launch (``wrappers.EpisodeRecorder``), and
``--learner NAME --episode_log per_episode`` writes the reference's points: one ``charts/episodic_return`` /
``charts/episodic_length`` pair per episode that ends in rollout steps 0-2, env ids ascending, at that step's
``global_step`` (PPO/main.py:98-103).  The rollout loop reads nothing back for them: the kernel appends the records
on the device, and the host reads the count and ``records[:count]`` once per rollout, after the synchronize the
loop already has.  ``--play`` runs the row's networks from ``--checkpoint``; with ``--learner NAME`` on the
observations NAME's rollout feeds its policy, logging ``reward/play``.

The update's knobs are flags at the reference's values (``--lr``, ``--update_epochs``, ``--num_minibatches``,
``--gamma``, ``--gae_lambda``, ``--clip_coef``, ``--vf_coef``, ``--max_grad_norm``, ``--no_norm_adv``, ``--ent_coef``,
``--clip_vloss``, ``--target_kl``, ``--anneal_lr``, ``--rpo_alpha``); the losses stay on the HIP kernels with any of
them.  ``--run_tag TAG`` appends ``_TAG`` to the run and checkpoint names, so a tuned run does not overwrite the
reference-named one.  The new per-update values (``entropy``, ``v_clipfrac``, ``epochs_run``) go to the returned
history only: the CSV columns and the event tags are the reference's.

``--normalize_input`` / ``--normalize_value`` turn on the learner's running normalisation of observations and value
targets (off by default).  Checkpoints then carry a fifth file, ``<name>_normalizers``, and ``--play``
with the same flags loads its statistics and applies them without updating them.

``--value_bootstrap`` (off by default) keeps the critic's value at episode ends caused by the time
limit: the rollout then stores the env's ``time_outs`` beside the dones and GAE runs as ``ouz_gae_bootstrap``; the
returned history carries ``timeout_frac``.  ``--max_episode_length N`` is the task YAML's ``maxEpisodeLength``.
``--play`` ignores ``--value_bootstrap``.

``--fused_rollout`` (off by default) collects the rollout with ``FusedRollout``: one kernel launch per
<= 32 steps that holds the env step, the learner-side corruption, the input normalisation, the MLP actor, the sample
and the log-prob (``ouz_policy_rollout``).  For the MLP learners (PPO, RPO, PPO_Critic, RPO_Critic, ``--algo ppo``) on
Ouzelum, QuadFault and Landing; refused otherwise.  The actions are drawn by the kernel's counter RNG (keyed by
``--seed``, the global env id and the step), not by torch's generator, so a fused run is another sample of the same
policy, reproducible and independent of the rank count.  ``--play --fused_rollout`` runs chunks of <= 32 steps.

``--fused_lstm_rollout`` (off by default) is the same for the LSTM learners (PPO-LSTM, RPO-LSTM,
RPO-LSTM_Critic, ``--algo rpo_lstm``) on the same tasks, with ``FusedLSTMRollout``: the trunk, the LSTM cell with its
done-masked carry and the head run inside the kernel (``ouz_policy_rollout_lstm``).  Refused for the MLP learners.
"""
import argparse
import csv
import os
import time

import numpy as np
import torch
import torch.distributed as dist

from ..distributed import init_from_env, shard
from ..vec_task import make
from .fused import store
from .ppo import PPOLearner
from .tbevents import EventWriter
from .variants import LEARNERS, VARIANTS, legacy_variant, names, single_stream
from .wrappers import RECORD_DTYPE, EpisodeRecorder, ExtractObsWrapper, POMDPWrapper, merge_records

COLUMNS = ("global_step", "average_reward", "episodes", "episodic_return", "episodic_length", "pg_loss", "v_loss",
           "approx_kl", "clipfrac", "env_steps_per_s")


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--algo", default="rpo_lstm", choices=["rpo_lstm", "ppo"])
    p.add_argument("--env", default="Landing")              # RPO-LSTM/main.py:18 (every reference learner)
    p.add_argument("--seed", default=0, type=int)
    p.add_argument("--num_envs", type=int, default=4096)
    p.add_argument("--rollout_steps", type=int, default=16)
    p.add_argument("--total_steps", type=int, default=30000000)
    p.add_argument("--POMDP", default="flicker")
    p.add_argument("--pomdp_prob", type=float, default=0.1)
    p.add_argument("--rollout_obs", default="clean", choices=["clean", "pomdp"])
    p.add_argument("--logdir", default="runs")
    p.add_argument("--checkpoint_dir", default="checkpoints")
    p.add_argument("--no_checkpoints", action="store_true")
    p.add_argument("--quiet", action="store_true")
    p.add_argument("--play", action="store_true", help="run a saved policy (RPO-LSTM/play.py) instead of training")
    p.add_argument("--checkpoint", default=None, help="checkpoint prefix (agent.save's filename)")
    p.add_argument("--learner", default=None, choices=list(LEARNERS),
                   help="one of the reference's seven learners (variants.py); not with --algo / --rollout_obs")
    p.add_argument("--gemm_dtype", default="f32", choices=["f32", "bf16"],
                   help="operand type of the update's large trunk products (bf16: f32 master weights and f32 "
                        "accumulation; the rollout and --play stay f32)")
    p.add_argument("--episode_log", default="rollout_mean", choices=["rollout_mean", "per_episode"],
                   help="charts/* points: one mean per rollout, or the reference's one per episode (with --learner)")
    # the update's knobs (PPOLearner's keywords; defaults: the reference's values, agent.py:14-25); --play ignores them
    p.add_argument("--lr", type=float, default=0.0026)
    p.add_argument("--update_epochs", type=int, default=4)
    p.add_argument("--num_minibatches", type=int, default=2)
    p.add_argument("--gamma", type=float, default=0.99)
    p.add_argument("--gae_lambda", type=float, default=0.95)
    p.add_argument("--clip_coef", type=float, default=0.2)
    p.add_argument("--vf_coef", type=float, default=2)
    p.add_argument("--max_grad_norm", type=float, default=1)
    p.add_argument("--no_norm_adv", action="store_true", help="no advantage normalisation per minibatch")
    p.add_argument("--ent_coef", type=float, default=0.0, help="entropy bonus (on the HIP loss path)")
    p.add_argument("--clip_vloss", action="store_true", help="the clipped value loss (on the HIP loss path)")
    p.add_argument("--target_kl", type=float, default=None, help="stop an update after the epoch whose approx-kl exceeds it")
    p.add_argument("--anneal_lr", action="store_true", help="lr * (1 - update / num_updates), as CleanRL")
    p.add_argument("--rpo_alpha", type=float, default=None, help="overrides the learner row's value in training; --play ignores it like the rest of the update's "
                        "flags, so a policy trained with another alpha plays with the row's value")
    p.add_argument("--run_tag", default=None, help="appended to the run and checkpoint names (default: the reference's names)")
    # running normalisation; with --play: load the checkpoint's statistics and apply them unchanged
    p.add_argument("--normalize_input", action="store_true",
                   help="running mean / variance normalisation of each network's observations (clipped to +-5)")
    p.add_argument("--normalize_value", action="store_true",
                   help="the critic learns the returns normalised by their running mean / variance")
    # the critic's value kept at time-limit episode ends; --play ignores it like the update's knobs
    p.add_argument("--value_bootstrap", action="store_true",
                   help="GAE keeps gamma * V(terminal observation) where an episode ended by its time limit")
    p.add_argument("--max_episode_length", type=int, default=None,
                   help="the task YAML's maxEpisodeLength (default: the task's own)")
    # the rollout as one launch per <= 32 steps with the MLP actor inside the kernel
    p.add_argument("--fused_rollout", action="store_true",
                   help="env step, corruption, normalisation, MLP actor and sample in one kernel (the MLP learners on "
                        "Ouzelum / QuadFault / Landing); with --play: chunks of <= 32 steps")
    # the same with the recurrent actor inside the kernel
    p.add_argument("--fused_lstm_rollout", action="store_true",
                   help="env step, corruption, normalisation, LSTM actor (carry included) and sample in one kernel (the "
                        "LSTM learners on Ouzelum / QuadFault / Landing); with --play: chunks of <= 32 steps")
    args = p.parse_args(argv)
    for flag, refusal in (("fused_rollout", fused_rollout_refusal), ("fused_lstm_rollout", fused_lstm_rollout_refusal)):
        if getattr(args, flag):
            why = refusal(VARIANTS[args.learner] if args.learner is not None
                          else legacy_variant(args.algo, args.rollout_obs), args.env)
            if why:
                p.error(why)
    if args.learner is not None:
        # given explicitly (their defaults say nothing): a second look at the same argv with no defaults
        probe = argparse.ArgumentParser(add_help=False)
        probe.add_argument("--algo", default=None)
        probe.add_argument("--rollout_obs", default=None)
        given, _ = probe.parse_known_args(argv)
        for flag in ("algo", "rollout_obs"):
            if getattr(given, flag) is not None:
                p.error(f"--learner decides the actor and the observation routing: it cannot be combined with --{flag}")
    elif args.episode_log != "rollout_mean":
        p.error("--episode_log per_episode needs --learner (the --algo loop keeps the per-rollout means)")
    return args


def variant_of(args):
    """The table row the flags select: ``--learner``'s, or the one ``--algo`` / ``--rollout_obs`` describe."""
    return VARIANTS[args.learner] if args.learner is not None else legacy_variant(args.algo, args.rollout_obs)


def learner_kwargs(args, v):
    """PPOLearner's update keywords from the flags; ``--rpo_alpha`` overrides the row's value.  The normalisation
    keywords are passed only when their flag is given (the constructor's default is off)."""
    kw = {"lr": args.lr, "update_epochs": args.update_epochs, "num_minibatches": args.num_minibatches,
          "gamma": args.gamma, "gae_lambda": args.gae_lambda, "clip_coef": args.clip_coef, "vf_coef": args.vf_coef,
          "max_grad_norm": args.max_grad_norm, "norm_adv": not args.no_norm_adv, "ent_coef": args.ent_coef,
          "clip_vloss": args.clip_vloss, "target_kl": args.target_kl,
          "rpo_alpha": v.rpo_alpha if args.rpo_alpha is None else args.rpo_alpha}
    kw.update(normalization_kwargs(args))
    if getattr(args, "value_bootstrap", False):
        kw["value_bootstrap"] = True
    return kw


def env_kwargs(args):
    """``make``'s keywords from the flags: ``--max_episode_length`` only when given (the task's own otherwise)."""
    n = getattr(args, "max_episode_length", None)
    return {} if n is None else {"max_episode_length": int(n)}


def normalization_kwargs(args):
    """``--normalize_input`` / ``--normalize_value`` as PPOLearner keywords (training and ``--play``)."""
    return {k: True for k in ("normalize_input", "normalize_value") if getattr(args, k, False)}


def run_names(args, v):
    """(run, best checkpoint) names: the reference's (variants.names), with ``--run_tag`` appended when given."""
    name, best = names(v, args.POMDP, args.pomdp_prob)
    if args.run_tag:
        name, best = f"{name}_{args.run_tag}", f"{best}_{args.run_tag}"
    return name, best


def annealed_fraction(update_index, num_updates):
    """``--anneal_lr``: the learning-rate fraction before update ``update_index`` (from 0) of ``num_updates``."""
    return 1.0 - update_index / num_updates


def write_episode_points(tb, records, g0, step_envs):
    """The reference's per-episode points (PPO/main.py:98-103) from a rollout's records sorted by (tag, env id):
    ``charts/episodic_return`` then ``charts/episodic_length`` per record, at the ``global_step`` after the
    increment of rollout step ``tag``: ``g0 + (tag + 1) * step_envs`` (``g0``: the value before the rollout,
    ``step_envs``: envs over all ranks)."""
    for tag, _, ret, length in records.tolist():
        gs = g0 + (tag + 1) * step_envs
        tb.add_scalar("charts/episodic_return", ret, gs)
        tb.add_scalar("charts/episodic_length", length, gs)


def gather_records(rec, world):
    """Every rank's record buffer and count in ONE fixed-size all-gather (issued on the device, before the loop's
    synchronize); returns a function that, after the synchronize, gives the merged records of all ranks."""
    flat = torch.cat([rec.records.reshape(-1), rec.count.reshape(-1)])
    out = torch.empty((world, flat.numel()), dtype=flat.dtype, device=flat.device)
    dist.all_gather_into_tensor(out, flat)

    def merged():
        counts = out[:, -1].cpu().tolist()
        if max(counts) > rec.capacity:
            raise RuntimeError(f"episode records overflowed: {max(counts)} appended, capacity {rec.capacity}")
        return merge_records([np.ascontiguousarray(out[r, :4 * c].cpu().numpy()).view(RECORD_DTYPE).reshape(-1)
                              for r, c in enumerate(counts)])
    return merged


class Rollout:
    """The rollout of every learner: the (T, N) storage, the state carried from one rollout to the next, and the
    step loop in the routing of the row ``v`` (variants.py).  ``envs`` hands out observation tensors
    (``ExtractObsWrapper``), with or without an ``EpisodeRecorder`` around it.  Resets ``envs``: the first
    observation of a run is the clean one in every routing (main.py:80-82).  ``watch=True`` (needs the recorder)
    also keeps in ``seen`` what no learner stores: ``acted_on`` (T, N, d: what the policy was given at each step),
    ``dones`` (T, N: ``next_done`` after each step) and ``r`` / ``l`` (T, N: info["r"] / info["l"] after each step)."""

    def __init__(self, envs, pomdp_w, agent, v, T, watch=False):
        self.envs, self.pomdp_w, self.agent, self.v, self.T = envs, pomdp_w, agent, v, T
        self.single = single_stream(v)
        N, device = agent.num_envs, agent.device
        obs_shape = envs.observation_space.shape
        self.obs = torch.zeros((T, N) + obs_shape, device=device)
        self.pomdps = None if self.single else torch.zeros((T, N) + obs_shape, device=device)
        self.actions = torch.zeros((T, N) + envs.action_space.shape, device=device)
        self.logprobs = torch.zeros((T, N), device=device)
        self.rewards = torch.zeros((T, N), device=device)
        self.dones = torch.zeros((T, N), device=device)
        self.seen = None
        if watch:
            self.seen = {"acted_on": torch.zeros((T, N) + obs_shape, device=device),
                         "dones": torch.zeros((T, N), dtype=torch.int64, device=device),
                         "r": torch.zeros((T, N), device=device),
                         "l": torch.zeros((T, N), dtype=torch.int32, device=device)}
        self.next_obs = envs.reset()
        self.pomdp = self.next_obs.clone()
        if self.single:
            self.next_obs = self.pomdp        # a tensor of its own: the env overwrites its observation buffer in place
        self.next_done = torch.zeros(N, device=device)
        # the env's time-out flags beside the dones, only for a learner with value_bootstrap, in
        # the env's byte dtype: timeouts[k] came with obs[k], as dones[k] did.  next_timeout is a tensor of the
        # rollout's own: the env overwrites its time_outs buffer in place on the next step.
        self.bootstrap = bool(getattr(agent, "value_bootstrap", False))
        self.timeouts = self.next_timeout = None
        if self.bootstrap:
            self.timeouts = torch.zeros((T, N), dtype=torch.bool, device=device)
            self.next_timeout = torch.zeros(N, dtype=torch.bool, device=device)
        self.lstm_state = agent.initial_state()
        self.init_state = None

    def collect(self, per_episode=False):
        """T steps on from where the last call stopped.  ``per_episode`` (needs the recorder) appends the records of
        the episodes that end in steps 0-2 (PPO/main.py:98: ``if 0 <= step <= 2``)."""
        envs, pomdp_w, agent, seen, single = self.envs, self.pomdp_w, self.agent, self.seen, self.single
        obs, pomdps, actions, logprobs, rewards, dones = (self.obs, self.pomdps, self.actions, self.logprobs,
                                                          self.rewards, self.dones)
        acts_on_pomdp = self.v.acts_on == "pomdp"
        next_obs, pomdp, next_done, lstm_state = self.next_obs, self.pomdp, self.next_done, self.lstm_state
        self.init_state = (lstm_state[0].clone(), lstm_state[1].clone()) if lstm_state is not None else None
        if per_episode:
            envs.begin_rollout()
        # with value_bootstrap: the time-out flags that came with next_obs go into the same store call as the dones (the
        # env's own buffer after the first step, copied before the next step overwrites it); without it the call is
        # as it was
        timeouts, next_to = self.timeouts, self.next_timeout
        tmo_dst = tmo_src = ()
        for step in range(self.T):
            if timeouts is not None:
                tmo_dst, tmo_src = (timeouts[step],), (next_to,)
            if single:
                store((obs[step], dones[step], *tmo_dst), (next_obs, next_done, *tmo_src))
                act_in = next_obs
            else:
                store((pomdps[step], obs[step], dones[step], *tmo_dst),
                      (pomdp, next_obs, next_done, *tmo_src))                                # one multi-tensor copy
                act_in = pomdp if acts_on_pomdp else next_obs
            if seen is not None:
                seen["acted_on"][step].copy_(act_in)
            # alias=True: the policy graph's output buffers (actions[step] / logprobs[step] copy them before the next
            # replay); alias=False adds 5 clones per step
            action, logprob, _, lstm_state = agent.act(act_in, lstm_state, next_done, alias=True)
            store((actions[step], logprobs[step]), (action, logprob))
            if per_episode and step <= 2:
                envs.record(step)
            next_obs, rewards[step], next_done, info = envs.step(action)
            if single:
                next_obs = pomdp_w.observation(next_obs)     # PPO/main.py:96
            else:
                pomdp = pomdp_w.observation(next_obs)        # RPO-LSTM/main.py:103
            if timeouts is not None:
                next_to = info["time_outs"]
            if seen is not None:
                store((seen["dones"][step], seen["r"][step], seen["l"][step]), (next_done, info["r"], info["l"]))
        if timeouts is not None:
            self.next_timeout.copy_(next_to)
        self.next_obs, self.pomdp, self.next_done, self.lstm_state = next_obs, pomdp, next_done, lstm_state

    def update(self):
        """One PPO update on the rollout just collected; the actor trains on the POMDP stream."""
        kw = {"timeouts": self.timeouts, "next_timeout": self.next_timeout} if self.bootstrap else {}
        return self.agent.train(self.obs, self.obs if self.single else self.pomdps, self.actions, self.next_obs,
                                self.next_done, self.init_state, self.logprobs, self.rewards, self.dones, **kw)


FUSED_TASKS = ("Ouzelum", "QuadFault", "Landing")   # the tasks whose step takes the policy's action


def fused_rollout_refusal(v, task):
    """Why ``--fused_rollout`` cannot serve the row ``v`` on ``task`` (None: it can)."""
    if v.recurrent:
        return ("--fused_rollout evaluates the 13 -> 256 -> 256 -> 4 MLP actor inside the rollout kernel: it serves "
                "PPO, RPO, PPO_Critic and RPO_Critic (and --algo ppo), not the LSTM learners")
    if task not in FUSED_TASKS:
        return (f"--fused_rollout needs a task whose step takes the policy's action ({', '.join(FUSED_TASKS)}), "
                f"not {task}")
    return None


def actor_weights(agent):
    """The MLP actor's tensors as ``QuadVecTask.policy_rollout_plan`` takes them (views: the optimiser updates them in
    place)."""
    m = agent.actor.actor_mean
    return (m[0].weight, m[0].bias, m[2].weight, m[2].bias, m[4].weight, m[4].bias, agent.actor.actor_logstd.view(-1))


class FusedRollout:
    """``Rollout`` as ONE launch per <= 32 steps (``QuadVecTask.policy_rollout_plan``): the env step,
    the learner-side corruption, the input normalisation, the MLP actor, the Gaussian sample and the log-prob all run
    inside the rollout kernel.  The same attributes as ``Rollout`` (``update()`` is shared), held as views of
    (T + 1)-row stores: row k is what came before step k, so ``obs = store[:T]``, ``next_obs = store[T]`` and row 0
    of the next rollout is one copy of row T.  ``dones[k]``, ``timeouts[k]`` and the first clean observation of a run
    follow ``Rollout``.  The episode statistics (``EpisodeRecorder``) are replayed after the launch from the stored
    reward and done rows, of which they are a pure function; ``pomdp_w.calls`` advances by T, so a fused and a
    per-step rollout can alternate.  The eps of env g at the rollout's step k is keyed (``sample_seed``, g,
    ``sample_calls`` + k)."""

    _refusal = staticmethod(fused_rollout_refusal)

    def __init__(self, envs, pomdp_w, agent, v, T, watch=False, sample_seed=0):
        why = self._refusal(v, envs.task_name)
        if why:
            raise ValueError(why)
        self.envs, self.pomdp_w, self.agent, self.v, self.T = envs, pomdp_w, agent, v, T
        self.single = single_stream(v)
        self.recorder = envs if isinstance(envs, EpisodeRecorder) else None
        N, device = agent.num_envs, agent.device
        d = envs.observation_space.shape[0]
        self._clean = torch.zeros((T + 1, N, d), device=device)
        self._pomdp = torch.zeros((T + 1, N, d), device=device)
        self._done = torch.zeros((T + 1, N), device=device)
        self._tmo = torch.zeros((T + 1, N), dtype=torch.bool, device=device)
        self._resets = torch.zeros((T, N), dtype=torch.int64, device=device)
        self.actions = torch.zeros((T, N) + envs.action_space.shape, device=device)
        self.logprobs = torch.zeros((T, N), device=device)
        self.rewards = torch.zeros((T, N), device=device)
        first = envs.reset()                     # the first observation of a run is the clean one in every routing
        self._clean[0].copy_(first)
        self._pomdp[0].copy_(first)
        self.obs = (self._pomdp if self.single else self._clean)[:T]
        self.pomdps = None if self.single else self._pomdp[:T]
        self.dones = self._done[:T]
        self.bootstrap = bool(getattr(agent, "value_bootstrap", False))
        self.timeouts = self._tmo[:T] if self.bootstrap else None
        self.next_timeout = self._tmo[T] if self.bootstrap else None
        self.next_obs = (self._pomdp if self.single else self._clean)[T]
        self.pomdp = self._pomdp[T]
        self.next_done = self._done[T]
        self.lstm_state = self.init_state = None
        self.acts_on_pomdp = v.acts_on == "pomdp"
        self.sample_calls = 0
        self.seen = None
        if watch:
            self.seen = {"acted_on": (self._pomdp if self.acts_on_pomdp else self._clean)[:T], "dones": self._resets,
                         "r": torch.zeros((T, N), device=device),
                         "l": torch.zeros((T, N), dtype=torch.int32, device=device)}
        self._make_plan(sample_seed)
        self._started = False

    def _plan_args(self, sample_seed):
        """The tensors and keywords both policy rollout plans take after the policy's own."""
        T, pomdp_w = self.T, self.pomdp_w
        norm = getattr(self.agent.actor, "obs_norm", None)
        return ((T, (self._pomdp if self.acts_on_pomdp else self._clean)[0],
                 (self._clean[1:], self.rewards, self._resets, self._tmo[1:]), self.actions, self.logprobs),
                dict(pomdp=self._pomdp[1:], norm=None if norm is None else (norm.m, norm.r, norm.clip),
                     acts_on_pomdp=self.acts_on_pomdp, pomdp_mode=pomdp_w.mode, pomdp_prob=pomdp_w.prob,
                     pomdp_seed=pomdp_w.seed, pomdp_row_offset=pomdp_w.row_offset, sample_seed=sample_seed))

    def _make_plan(self, sample_seed):
        args, kw = self._plan_args(sample_seed)
        self._run = self.envs.policy_rollout_plan(actor_weights(self.agent), *args, **kw)

    def _launch(self):
        self._run(self.pomdp_w.calls, self.sample_calls)

    def collect(self, per_episode=False):
        """T steps on from where the last call stopped, in ceil(T / 32) launches."""
        T, rec = self.T, self.recorder
        if self._started:   # row 0 of this rollout: what came after the last step of the previous one
            store((self._clean[0], self._pomdp[0], self._done[0], self._tmo[0]),
                  (self._clean[T], self._pomdp[T], self._done[T], self._tmo[T]))
        self._started = True
        self._launch()
        self.pomdp_w.calls += T
        self.sample_calls += T
        self._done[1:].copy_(self._resets)
        if rec is not None:
            if per_episode:
                rec.begin_rollout()
            for step in range(T):
                if per_episode and step <= 2:
                    rec.record(step)
                rec.update(self.rewards[step], self._resets[step])
                if self.seen is not None:
                    store((self.seen["r"][step], self.seen["l"][step]),
                          (rec.returned_episode_returns, rec.returned_episode_lengths))

    update = Rollout.update


def fused_lstm_rollout_refusal(v, task):
    """Why ``--fused_lstm_rollout`` cannot serve the row ``v`` on ``task`` (None: it can)."""
    if not v.recurrent:
        return ("--fused_lstm_rollout evaluates the 13 -> 512 -> 256 -> LSTM(128) -> 4 recurrent actor inside the "
                "rollout kernel: it serves PPO-LSTM, RPO-LSTM and RPO-LSTM_Critic (and --algo rpo_lstm), not the MLP "
                "learners (--fused_rollout serves those)")
    if task not in FUSED_TASKS:
        return (f"--fused_lstm_rollout needs a task whose step takes the policy's action ({', '.join(FUSED_TASKS)}), "
                f"not {task}")
    return None


def lstm_actor_weights(agent):
    """The LSTM actor's tensors as ``QuadVecTask.lstm_policy_rollout_plan`` takes them (views: the optimiser updates
    them in place)."""
    a = agent.actor
    return (a.network[0].weight, a.network[0].bias, a.network[2].weight, a.network[2].bias, a.lstm.weight_ih_l0,
            a.lstm.weight_hh_l0, a.lstm.bias_ih_l0, a.lstm.bias_hh_l0, a.actor_mean.weight, a.actor_mean.bias,
            a.actor_logstd.view(-1))


class FusedLSTMRollout(FusedRollout):
    """``FusedRollout`` for the recurrent learners (``QuadVecTask.lstm_policy_rollout_plan``): the
    trunk, the LSTM cell and the head run inside the rollout kernel, which carries (h, c) through the launch and
    zeroes the carry of env b before step k where ``dones[k, b]`` is set, as ``LSTMActor.get_states`` does.
    ``init_state`` is the carry the launch started from and ``lstm_state`` the one it left (the last step's done not
    applied: the next launch, like the next ``act``, applies it).  Two (h, c) pairs alternate between rollouts, so the
    update reads an ``init_state`` that no later launch has overwritten."""

    _refusal = staticmethod(fused_lstm_rollout_refusal)

    def _make_plan(self, sample_seed):
        args, kw = self._plan_args(sample_seed)
        agent, w = self.agent, lstm_actor_weights(self.agent)
        self._carry = [agent.initial_state(), agent.initial_state()]
        self._runs = []
        for j in (0, 1):
            (hi, ci), (ho, co) = self._carry[j], self._carry[1 - j]
            self._runs.append(self.envs.lstm_policy_rollout_plan(w, (hi[0], ci[0], self._done[0], ho[0], co[0]),
                                                                 *args, **kw))
        self._flip = 0
        self.lstm_state = self._carry[0]

    def _launch(self):
        j = self._flip
        self.init_state = self._carry[j]
        self._runs[j](self.pomdp_w.calls, self.sample_calls)
        self.lstm_state = self._carry[1 - j]
        self._flip = 1 - j

    def adopt(self, prev):
        """Carry on from where the rollout ``prev`` (of another length) stopped: its last rows, carry and call
        count."""
        store((self._clean[0], self._pomdp[0], self._done[0]), (prev._clean[prev.T], prev._pomdp[prev.T],
                                                                prev._done[prev.T]))
        store(self._carry[0], prev.lstm_state)
        self._flip = 0
        self.lstm_state = self._carry[0]
        self.sample_calls = prev.sample_calls


def make_rollout(args, envs, pomdp_w, agent, v, T, watch=False):
    """``Rollout``, or with ``--fused_rollout`` the one-launch ``FusedRollout`` (refused with its reason for the LSTM
    learners and the tasks without a policy action), or with ``--fused_lstm_rollout`` its recurrent form
    ``FusedLSTMRollout`` (refused for the MLP learners)."""
    if getattr(args, "fused_lstm_rollout", False):
        return FusedLSTMRollout(envs, pomdp_w, agent, v, T, watch=watch, sample_seed=args.seed + 2)
    if getattr(args, "fused_rollout", False):
        return FusedRollout(envs, pomdp_w, agent, v, T, watch=watch, sample_seed=args.seed + 2)
    return Rollout(envs, pomdp_w, agent, v, T, watch=watch)


def train(args, on_rollout=None):
    """``on_rollout(dict)``, if given, is called once per rollout (after the update and the synchronize) with the
    rollout's tensors: ``obs`` and ``pomdps`` storage (``pomdps`` None for the single-stream learners), the bootstrap
    ``next_obs``, ``Rollout.seen``'s ``acted_on`` / ``dones`` / ``r`` / ``l``, ``global_step_before``, ``stats`` and
    the per-episode ``records`` (None with ``--episode_log rollout_mean``)."""
    v = variant_of(args)
    per_episode = args.episode_log == "per_episode"
    rank, world, local = init_from_env()
    device = torch.device("cuda", local)
    torch.cuda.set_device(device)
    np.random.seed(args.seed + rank)
    torch.manual_seed(args.seed + rank)
    N, T = args.num_envs, args.rollout_steps
    off, total = shard(N, rank, world)

    base = make(seed=args.seed, task=args.env, num_envs=N, sim_device=str(device), rl_device=str(device),
                graphics_device_id=-1, headless=True, env_id_offset=off, num_envs_total=total, track_episodes=True,
                **env_kwargs(args))
    envs = EpisodeRecorder(ExtractObsWrapper(base), device, env_id0=off, capacity=3 * N)
    pomdp_w = POMDPWrapper(args.POMDP, args.pomdp_prob, seed=args.seed + 1, row_offset=off)
    agent = PPOLearner(base.observation_space, base.action_space, N, device, recurrent=v.recurrent,
                       rollout_steps=T, gemm_dtype=args.gemm_dtype, **learner_kwargs(args, v))
    name, best = run_names(args, v)
    num_updates = max(1, -(-args.total_steps // (T * N * world)))   # the loop's trips
    ro = make_rollout(args, envs, pomdp_w, agent, v, T, watch=on_rollout is not None)

    writer = tb = None
    if rank == 0:
        os.makedirs(args.logdir, exist_ok=True)
        tb = EventWriter(os.path.join(args.logdir, name))
        fh = open(os.path.join(args.logdir, name + ".csv"), "w", newline="")
        writer = csv.writer(fh)
        writer.writerow(COLUMNS)

    global_step = 0
    max_reward = -float("inf")
    history = []
    t_start = time.perf_counter()
    while global_step < args.total_steps:
        t0 = time.perf_counter()
        g0 = global_step
        ro.collect(per_episode)
        global_step += T * N * world
        if args.anneal_lr:
            agent.set_lr_fraction(annealed_fraction(len(history), num_updates))
        stats = ro.update()
        ep = base.episode_stats()
        mean_rew = ro.rewards.mean()
        merged = None
        if world > 1:
            dist.all_reduce(ep)
            dist.all_reduce(mean_rew)
            mean_rew /= world
            if per_episode:
                merged = gather_records(envs, world)
        torch.cuda.synchronize(device)
        base.check_health()   # raises if a fused rollout's split-wave wait gave up (never on the per-step path)
        records = None
        if per_episode:   # the rollout's only host reads for the points: the count, then records[:count]
            records = merged() if merged is not None else envs.drain()
        sps = N * world * T / (time.perf_counter() - t0)
        row = {"global_step": global_step, "average_reward": float(mean_rew), "episodes": int(ep[1]),
               "episodic_return": float(ep[0] / ep[1]) if float(ep[1]) > 0 else float("nan"),
               "episodic_length": float(ep[2] / ep[1]) if float(ep[1]) > 0 else float("nan"),
               **{k: float(x) for k, x in stats.items()}, "env_steps_per_s": sps}
        history.append(row)
        if on_rollout is not None:
            on_rollout({"obs": ro.obs, "pomdps": ro.pomdps, "next_obs": ro.next_obs, **ro.seen,
                        "global_step_before": g0, "stats": stats, "records": records})
        if rank == 0:
            writer.writerow([row[k] for k in COLUMNS])
            if per_episode:
                write_episode_points(tb, records, g0, N * world)
            elif row["episodes"] > 0:
                tb.add_scalar("charts/episodic_return", row["episodic_return"], global_step)
                tb.add_scalar("charts/episodic_length", row["episodic_length"], global_step)
            tb.add_scalar("average/average_reward", row["average_reward"], global_step)
            tb.flush()
            if not args.quiet:
                print(f"Step: {global_step}, Average rewards {row['average_reward']:.4f}, "
                      f"{sps / 1e6:.2f} M env-steps/s", flush=True)
            if not args.no_checkpoints and row["average_reward"] > max_reward:
                max_reward = row["average_reward"]
                os.makedirs(args.checkpoint_dir, exist_ok=True)
                agent.save(os.path.join(args.checkpoint_dir, best))
    if rank == 0:
        if not args.no_checkpoints:
            agent.save(os.path.join(args.checkpoint_dir, name))
        fh.close()
        tb.close()
    elapsed = time.perf_counter() - t_start
    return {"history": history, "agent": agent, "env": base, "elapsed": elapsed, "events": tb.path if tb else None,
            "env_steps_per_s": global_step / elapsed, "run": name, "best": best}


@torch.no_grad()
def play(args):
    """RPO-LSTM/play.py:25-80: load a checkpoint and run the row's policy, printing the mean reward.  With
    ``--learner NAME`` the policy is fed what NAME's rollout feeds it: the POMDP observation for the five learners
    that act on it, the clean one for PPO-LSTM and RPO-LSTM; the first observation is the clean reset, as in
    training; and the reference's ``reward/play`` scalar (the step's mean reward at ``global_step``,
    RPO-LSTM_Critic/play.py:78-94) goes to an event file under ``--logdir``.  (The reference's RPO/play.py is a stale
    copy that skips the corruption; this follows the table.)  ``--algo`` plays on the clean observation whatever
    ``--rollout_obs`` says, and writes no event file."""
    v = variant_of(args)
    by_name = args.learner is not None
    device = torch.device("cuda", 0)
    N = args.num_envs
    base = make(seed=args.seed, task=args.env, num_envs=N, sim_device=str(device), rl_device=str(device),
                track_episodes=True, **env_kwargs(args))
    env = ExtractObsWrapper(base)
    agent = PPOLearner(base.observation_space, base.action_space, N, device, recurrent=v.recurrent,
                       rollout_steps=args.rollout_steps, tuned_gemms=False, rpo_alpha=v.rpo_alpha,   # inference only
                       **normalization_kwargs(args))   # the checkpoint's statistics, never updated here
    if args.checkpoint:
        agent.load(args.checkpoint)
    pomdp_w = POMDPWrapper(args.POMDP, args.pomdp_prob, seed=args.seed + 1)
    tb = None
    if by_name:
        tb = EventWriter(os.path.join(args.logdir, names(v, args.POMDP, args.pomdp_prob)[0] + "_play"))
    rewards, global_step = [], 0
    fused_cls = (FusedLSTMRollout if getattr(args, "fused_lstm_rollout", False)
                 else FusedRollout if getattr(args, "fused_rollout", False) else None)
    if fused_cls is not None:
        # chunks of <= 32 steps, each one launch (the LSTM carry chained from chunk to chunk); the reward/play points
        # from the stored reward rows
        steps = max(1, args.total_steps // N)
        acts = by_name and v.acts_on == "pomdp"
        if not acts:
            pomdp_w = POMDPWrapper("none", 0.0, seed=args.seed + 1)
        v_play = v._replace(acts_on="pomdp" if acts else "clean", critic_on="clean")
        ro = None
        while steps > 0:
            K = min(steps, 32)
            if ro is None or ro.T != K:
                prev = ro
                ro = fused_cls(env, pomdp_w, agent, v_play, K, sample_seed=args.seed + 2)
                if prev is not None and fused_cls is FusedLSTMRollout:
                    ro.adopt(prev)
                elif prev is not None:   # carry on from the last chunk's final rows
                    store((ro._clean[0], ro._pomdp[0]), (prev._clean[prev.T], prev._pomdp[prev.T]))
                    ro.sample_calls = prev.sample_calls
            ro.collect()
            steps -= K
            for r in ro.rewards.mean(1).tolist():
                global_step += N
                rewards.append(torch.tensor(r))
                if tb is not None:
                    tb.add_scalar("reward/play", r, global_step)
                if not args.quiet:
                    print((f"Step: {global_step}, " if by_name else "") + f"Average rewards {r:.4f}")
        steps = 0
    else:
        steps = max(1, args.total_steps // N)
        act_in = env.reset().clone()
        next_done = torch.zeros(N, device=device)
        lstm = agent.initial_state()
    for _ in range(steps):
        global_step += N
        action, _, _, lstm = agent.act(act_in, lstm, next_done)
        act_in, rew, next_done, _ = env.step(action)
        if by_name and v.acts_on == "pomdp":
            act_in = pomdp_w.observation(act_in)
        rewards.append(rew.mean())
        if tb is not None:
            tb.add_scalar("reward/play", float(rewards[-1]), global_step)
        if not args.quiet:
            print((f"Step: {global_step}, " if by_name else "") + f"Average rewards {float(rewards[-1]):.4f}")
    out = {"mean_reward": float(torch.stack(rewards).mean()), "episode_stats": base.episode_stats().tolist()}
    if tb is not None:
        tb.close()
        out["events"] = tb.path
    return out


def main(argv=None):
    args = parse_args(argv)
    if args.play:
        return play(args)
    out = train(args)
    if dist.is_initialized():
        dist.destroy_process_group()
    return out


if __name__ == "__main__":
    main()
