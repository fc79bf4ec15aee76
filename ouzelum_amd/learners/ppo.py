"""PPO / RPO-LSTM update on MI355X with the rollout size as a parameter.

Mirrors ``RPO-LSTM/agent.py:9-147`` (recurrent, env-wise minibatches, RPO noise) and
``PPO/agent.py`` (feed-forward, sample-wise minibatches): same hyper-parameters
(clip 0.2, gamma 0.99, lambda 0.95, 4 epochs, 2 minibatches, vf_coef 2, grad-norm 1,
Adam lr 2.6e-3 eps 1e-5, advantage normalisation) and the same checkpoint files.
Differences, all MI355X-side:

* N and T are parameters: the reference hard-codes ``values.reshape(16, 4096)``
  (``agent.py:61``), so any other env count crashes there.
* GAE is one HIP launch (``ouz_gae``) instead of a T-step Python loop; values are
  computed without building an autograd graph (the clipped value loss, when ``clip_vloss``
  asks for it, needs their numbers only).
* Minibatch permutations come from device RNG (no H2D copy of a numpy permutation) and the clip fractions stay on the device until the end of
  the update (the reference syncs with ``.item()`` every minibatch).
* The minibatch losses run as HIP kernels on the GPU (``fused.PolicyLossEnt`` / ``ValueLoss`` / ``ValueLossClipped``:
  forward and input gradients in 3 + 2 launches instead of ~60), with or without the update's options (``ent_coef``,
  ``clip_vloss``); ``OUZ_FUSED_LOSS=0`` keeps the torch form.
* The update's knobs (``gamma``, ``gae_lambda``, ``clip_coef``, ``norm_adv``, ``ent_coef``, ``vf_coef``,
  ``clip_vloss``, ``target_kl``, ``max_grad_norm``) are constructor keywords at the reference's values, and
  ``set_lr_fraction`` anneals the learning rate (``train.py --anneal_lr``).
* Under torchrun (one process per GPU, env ids sharded) the learner is data
  parallel: rank 0's initial weights are broadcast and every optimizer step
  all-reduces one flattened gradient bucket over RCCL.  The reference learners are
  single-GPU.
* ``gemm_dtype="bf16"`` (opt-in; DESIGN.md §9.1 "Precision contract"): the update's large trunk products take bf16
  operands with f32 accumulation, from bf16 shadows of the f32 master weights that the optimizer step keeps current.
  Everything without autograd (the rollout policy, the value pass before GAE, ``--play``) keeps the f32 weights.
* ``normalize_input`` / ``normalize_value`` (opt-in): running normalisation of each network's
  observations and of the value targets (``fused.RunningNorm``, f64 statistics on the device).  The calls without
  autograd normalise inside the first layer's kernel; the update normalises its T·N rows once per stream.  The input
  statistics merge a rollout AFTER its update, so the update scores the rollout under the statistics it was
  collected under; the value statistics merge the returns before the targets are formed.
* ``value_bootstrap`` (opt-in): GAE keeps ``gamma * V(terminal observation)`` where an episode ended by
  its time limit (``ouz_gae_bootstrap``: the same one launch, reading the env's ``time_outs`` bytes).  The terminal
  observation's value is already among the update's values, because the env resets lazily.
"""
import contextlib
import os

import numpy as np
import torch
import torch.distributed as dist
import torch.nn as nn

from .. import _lib as L
from .fused import Bf16Shadows, ClipAdam, PolicyLossEnt, RunningNorm, ValueLoss, ValueLossClipped
from .gemm_tuning import enable_tuned_gemms
from .models import Critic, LSTMActor, MLPActor


def _graph_replay_safe():
    """hipGraph replay gives correct results only with the runtime's packet-capture path off (set by
    ``ouzelum_amd/__init__.py`` before the HIP runtime starts)."""
    import warnings
    from .. import GRAPH_REPLAY_SAFE
    if not GRAPH_REPLAY_SAFE and not getattr(_graph_replay_safe, "warned", False):
        warnings.warn("HIP runtime started with DEBUG_CLR_GRAPH_PACKET_CAPTURE on: the rollout policy runs eagerly "
                      "(import ouzelum_amd before initialising the GPU, or set the variable to 0)")
        _graph_replay_safe.warned = True
    return GRAPH_REPLAY_SAFE


def broadcast_params(module, src=0):
    """Same initial weights on every rank (one flattened broadcast)."""
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return
    flat = torch.cat([p.data.reshape(-1) for p in module.parameters()])
    dist.broadcast(flat, src)
    off = 0
    for p in module.parameters():
        n = p.numel()
        p.data.copy_(flat[off:off + n].view_as(p))
        off += n


def allreduce_grads(module):
    """Data-parallel gradient mean over ranks: ONE all-reduce of the flattened gradients per
    optimizer step (the networks are < 1 M parameters, so a single bucket beats per-tensor calls
    on xGMI's per-link ring)."""
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return
    params = [p for p in module.parameters() if p.grad is not None]
    flat = torch.cat([p.grad.reshape(-1) for p in params])
    dist.all_reduce(flat)
    flat /= dist.get_world_size()
    off = 0
    for p in params:
        n = p.numel()
        p.grad.copy_(flat[off:off + n].view_as(p.grad))
        off += n


_TIMEOUT_DTYPES = (torch.bool, torch.uint8)


def gae(rewards, values, dones, next_value, next_done, gamma=0.99, lam=0.95, timeouts=None, next_timeout=None):
    """(returns, advantages), each (T, N) f32, from the HIP kernel (RPO-LSTM/agent.py:40-55).  With ``timeouts``
    (T, N) and ``next_timeout`` (N), the env's ``time_outs`` bytes (torch.bool or torch.uint8, contiguous) aligned
    with ``dones`` / ``next_done``, the successor's value is kept where its done is a time-out
    (``ouz_gae_bootstrap``); both or neither."""
    if (timeouts is None) != (next_timeout is None):
        raise ValueError("timeouts and next_timeout go together: both or neither")
    T, N = rewards.shape
    ts = [t.contiguous().float() for t in (rewards, values, dones, next_value.reshape(N), next_done.reshape(N))]
    for t, name in zip(ts, ("rewards", "values", "dones", "next_value", "next_done")):
        L.require_hip_tensor(t, name)
    if timeouts is not None:
        for t, name, shape in ((timeouts, "timeouts", (T, N)), (next_timeout, "next_timeout", (N,))):
            if t.dtype not in _TIMEOUT_DTYPES or tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError(f"{name} must be a contiguous {shape} torch.bool or torch.uint8 tensor (the env's "
                                 f"bytes), not {tuple(t.shape)} {t.dtype}")
            L.require_hip_tensor(t, name)
    adv = torch.empty_like(ts[0])
    ret = torch.empty_like(ts[0])
    # the reference multiplies by the Python product gamma * lambda (a double), rounded once to f32
    if timeouts is not None:
        L.check(L.lib.ouz_gae_bootstrap(L.ptr(ts[0]), L.ptr(ts[1]), L.ptr(ts[2]), L.ptr(timeouts), L.ptr(ts[3]),
                                        L.ptr(ts[4]), L.ptr(next_timeout), T, N, gamma, float(gamma * lam),
                                        L.ptr(adv), L.ptr(ret), L.stream_ptr(adv.device)), "ouz_gae_bootstrap")
        return ret, adv
    L.check(L.lib.ouz_gae(*(L.ptr(t) for t in ts), T, N, gamma, float(gamma * lam), L.ptr(adv), L.ptr(ret),
                          L.stream_ptr(adv.device)), "ouz_gae")
    return ret, adv


GEMM_DTYPES = ("f32", "bf16")
OBS_CLIP = 5.0   # normalised observations are clamped to +-5; normalised values are not clamped


class PPOLearner:
    def __init__(self, observation_space, action_space, num_envs, device, recurrent=True, rollout_steps=16,
                 lr=0.0026, num_minibatches=2, update_epochs=4, tuned_gemms=True, rpo_alpha=None, gemm_dtype="f32",
                 gamma=0.99, gae_lambda=0.95, clip_coef=0.2, norm_adv=True, ent_coef=0.0, vf_coef=2, clip_vloss=False,
                 target_kl=None, max_grad_norm=1, normalize_input=False, normalize_value=False,
                 value_bootstrap=False):
        """The keywords after ``gemm_dtype`` are the reference update's knobs (agent.py:14-25) at its values; each
        becomes the attribute of its name (``gae_lambda``: ``gae_lamda``, the reference's spelling), which may also
        be set after construction.  ``normalize_input`` / ``normalize_value`` (fixed at construction)
        give each network a running normaliser of its observations (clip 5) and put the critic's output in the
        normalised units of the returns.  ``value_bootstrap`` (off by default): GAE keeps the
        critic's value of the terminal observation where an episode ended by its time limit; ``train`` / ``get_gae``
        then need the rollout's ``timeouts`` / ``next_timeout``."""
        if not isinstance(value_bootstrap, (bool, np.bool_)):
            raise ValueError(f"value_bootstrap must be a bool, not {value_bootstrap!r}")
        if gemm_dtype not in GEMM_DTYPES:
            raise ValueError(f"gemm_dtype must be one of {GEMM_DTYPES}, not {gemm_dtype!r}")
        if gemm_dtype == "bf16" and torch.device(device).type != "cuda":
            raise ValueError("gemm_dtype='bf16' needs a HIP device: the bf16 GEMM mode has no CPU form")
        for name, val in (("clip_coef", clip_coef), ("ent_coef", ent_coef), ("lr", lr)):
            if not val >= 0:
                raise ValueError(f"{name} must be >= 0, not {val!r}")
        if target_kl is not None and not target_kl >= 0:
            raise ValueError(f"target_kl must be None or >= 0, not {target_kl!r}")
        for name, val in (("gamma", gamma), ("gae_lambda", gae_lambda)):
            if not 0 <= val <= 1:
                raise ValueError(f"{name} must lie in [0, 1], not {val!r}")
        self.gemm_dtype = gemm_dtype
        self.value_bootstrap = bool(value_bootstrap)
        self.obs_dim = observation_space
        self.act_dim = action_space
        self.num_envs = num_envs
        self.rollout_steps = rollout_steps
        self.device = torch.device(device)
        self.recurrent = recurrent
        self.clip_coef = clip_coef
        self.gamma = gamma
        self.gae_lamda = gae_lambda
        self.norm_adv = norm_adv
        self.update_epochs = update_epochs
        self.ent_coef = ent_coef
        self.vf_coef = vf_coef
        self.clip_vloss = clip_vloss
        self.target_kl = target_kl
        self.max_grad_norm = max_grad_norm
        self.lr0 = lr
        self.num_minibatches = num_minibatches
        self.batch_size = num_envs * rollout_steps
        self.minibatch_size = self.batch_size // num_minibatches
        if recurrent and num_envs % num_minibatches:
            raise ValueError("num_envs must divide into the minibatches")   # agent.py:72
        if tuned_gemms:
            enable_tuned_gemms(self.device)   # per-shape GEMM solutions (gemm_tuning.py); OUZ_TUNABLEOP=0: off
        # rpo_alpha None: each actor's own default (0.5 recurrent, RPO-LSTM/model.py:61; 0 for the MLP, PPO/model.py);
        # a value selects the RPO / PPO-LSTM variants (learners/variants.py).  With 0 the update draws no noise.
        alpha_kw = {} if rpo_alpha is None else {"rpo_alpha": float(rpo_alpha)}
        self.actor = (LSTMActor(observation_space, action_space, **alpha_kw) if recurrent
                      else MLPActor(observation_space, action_space, **alpha_kw)).to(self.device)
        self.rpo_alpha = self.actor.rpo_alpha
        self.critic = Critic(observation_space).to(self.device)
        broadcast_params(self.actor)
        broadcast_params(self.critic)
        # running normalisation (fused.RunningNorm): one normaliser per network over the stream it trains on (the
        # actor's: the POMDP stream, or the observations for the single-stream learners; the critic's: the
        # observations), read by every call of that network, and one over the returns.  Every rank starts from the
        # same statistics and merges the same triples, so they need no broadcast.
        self.normalize_input, self.normalize_value = bool(normalize_input), bool(normalize_value)
        n_obs = int(np.prod(observation_space.shape))
        self.actor_norm = self.critic_norm = self.value_norm = None
        if self.normalize_input:
            self.actor_norm = RunningNorm(n_obs, self.device, clip=OBS_CLIP)
            self.critic_norm = RunningNorm(n_obs, self.device, clip=OBS_CLIP)
            self.actor.obs_norm, self.critic.obs_norm = self.actor_norm, self.critic_norm
        if self.normalize_value:
            self.value_norm = RunningNorm(1, self.device)
        # the bf16 GEMM mode: bf16 shadows of both networks' GEMM weights, made after the broadcast
        self._shadows = None
        if gemm_dtype == "bf16":
            self._shadows = (Bf16Shadows(self.actor), Bf16Shadows(self.critic))
            self.actor.gemm_shadows, self.critic.gemm_shadows = self._shadows
        # fused Adam on the GPU: one multi-tensor kernel per optimizer step instead of the foreach
        # form's handful per parameter group (the update is launch-bound)
        fused = self.device.type == "cuda" and os.environ.get("OUZ_ADAM_FUSED", "1") != "0"
        # gradient clipping + Adam as two HIP launches per optimizer step (fused.ClipAdam; the torch optimizer keeps
        # the state and the checkpoint format); OUZ_CLIP_ADAM=0 keeps clip_grad_norm_ + the torch step
        clip_adam = fused and os.environ.get("OUZ_CLIP_ADAM", "1") != "0"
        opt_kw = {"foreach": False} if clip_adam else {"fused": fused}
        self.actor_optimizer = torch.optim.Adam(self.actor.parameters(), lr=lr, eps=1e-5, **opt_kw)
        self.critic_optimizer = torch.optim.Adam(self.critic.parameters(), lr=lr, eps=1e-5, **opt_kw)
        sh = self._shadows or (None, None)
        self._clip_adam = ((ClipAdam(self.actor_optimizer, sh[0]), ClipAdam(self.critic_optimizer, sh[1]))
                           if clip_adam else None)

    def set_lr_fraction(self, frac):
        """Both optimizers' learning rate = ``frac`` * the constructor's ``lr`` (LR annealing: ``train.py --anneal_lr``
        calls it before each update).  The optimizer step reads the group's ``lr`` on every call."""
        for opt in (self.actor_optimizer, self.critic_optimizer):
            for group in opt.param_groups:
                group["lr"] = frac * self.lr0

    def refresh_shadows(self):
        """The bf16 shadows from the current f32 weights, after anything but the optimizer step wrote the weights
        (``load``, a broadcast, a caller's own copy); nothing to do in the f32 mode."""
        for sh in self._shadows or ():
            sh.refresh()

    # ------------------------------------------------------------------ rollout
    @torch.no_grad()
    def get_action(self, state, lstm_state=None, done=None, eps=None):
        if self.recurrent:
            return self.actor(state, lstm_state, done, eps=eps)
        return (*self.actor(state, eps=eps), None)

    def initial_state(self):
        return self.actor.initial_state(self.num_envs, self.device) if self.recurrent else None

    def act(self, state, lstm_state=None, done=None, alias=False):
        """``get_action`` for one rollout step, replayed from a hipGraph on the GPU (``GraphedPolicy``)
        unless ``OUZ_GRAPH_POLICY=0``.  Returns fresh tensors; ``alias=True`` returns the graph's static
        output tensors instead, overwritten by the next call (the rollout loop copies them into its
        buffers at once and passes the LSTM carry straight back)."""
        if (self.device.type != "cuda" or os.environ.get("OUZ_GRAPH_POLICY", "1") == "0"
                or not _graph_replay_safe()):
            return self.get_action(state, lstm_state, done)
        if getattr(self, "_graphed", None) is None:
            self._graphed = GraphedPolicy(self)
        return self._graphed(state, lstm_state, done, alias=alias)

    @torch.no_grad()
    def _raw_values(self, v):
        """The critic's outputs in the units of the returns: with ``normalize_value`` the critic works in normalised
        units, denormalised here under the statistics in force."""
        if self.value_norm is None:
            return v
        return self.value_norm.denormalize(v.reshape(-1, 1)).reshape(v.shape)

    @torch.no_grad()
    def get_gae(self, next_obs, next_done, rewards, dones, values, *, timeouts=None, next_timeout=None):
        """``values``: in the units of the rewards (``_raw_values`` of the critic's outputs).  With
        ``value_bootstrap`` the time-out flags aligned with ``dones`` / ``next_done`` are required; without it they
        are ignored."""
        if self.value_bootstrap:
            self._require_timeouts(timeouts, next_timeout)
        next_value = self._raw_values(self.critic(next_obs).reshape(-1))
        if not self.value_bootstrap:
            return gae(rewards, values, dones, next_value, next_done, self.gamma, self.gae_lamda)
        # raw rewards and raw values here too (``_raw_values``): the bootstrapped tail gamma * V(terminal obs) is in
        # the units of the rewards, so ``normalize_value`` and ``clip_vloss`` see returns of the kind they saw before
        return gae(rewards, values, dones, next_value, next_done, self.gamma, self.gae_lamda,
                   timeouts=timeouts, next_timeout=next_timeout)

    @staticmethod
    def _require_timeouts(timeouts, next_timeout):
        if timeouts is None or next_timeout is None:
            raise ValueError("value_bootstrap=True needs the rollout's time-out flags: pass timeouts=(T, N) and "
                             "next_timeout=(N,), the env's time_outs aligned with dones and next_done")

    @contextlib.contextmanager
    def _inputs_prenormalized(self):
        """The networks without their input normalisers: the update's minibatches are rows of copies that were
        normalised once beforehand."""
        nets = (self.actor, self.critic)
        saved = [net.obs_norm for net in nets]
        for net in nets:
            net.obs_norm = None
        try:
            yield
        finally:
            for net, norm in zip(nets, saved):
                net.obs_norm = norm

    # ------------------------------------------------------------------- update
    def _perm(self, n):
        """A uniform random permutation from device RNG (no host round trip)."""
        return torch.argsort(torch.rand(n, device=self.device))

    def train(self, obs, pomdps, actions, next_obs, next_done, initial_lstm_state, logprobs, rewards, dones, *,
              timeouts=None, next_timeout=None):
        """One PPO update on a (T, N) rollout.  ``pomdps`` are the observations the actor trains on
        (RPO-LSTM trains on the POMDP-corrupted ones, agent.py:83); pass ``obs`` for plain PPO.  ``timeouts`` /
        ``next_timeout``: the env's time-out flags aligned with ``dones`` / ``next_done``, required with
        ``value_bootstrap`` and ignored without it."""
        T, N = rewards.shape
        if self.value_bootstrap:
            self._require_timeouts(timeouts, next_timeout)
        with torch.no_grad():
            values = self._raw_values(self.critic(obs.reshape(T * N, -1))).reshape(T, N)
        returns, advantages = self.get_gae(next_obs, next_done, rewards, dones, values, timeouts=timeouts,
                                           next_timeout=next_timeout)
        raw_obs = b_obs = obs.reshape(T * N, -1)
        raw_pomdps = b_pomdps = pomdps.reshape(T * N, -1)
        b_returns, b_values = returns.reshape(-1), values.reshape(-1)
        if self.normalize_input:
            # normalised copies of the T·N rows, once per update per stream, under the statistics the rollout was
            # collected under (they are merged after the last optimizer step, below)
            b_obs, b_pomdps = self.critic_norm.normalize(raw_obs), self.actor_norm.normalize(raw_pomdps)
        if self.value_norm is not None:
            # GAE ran on raw rewards and raw values; the targets (and the clipped loss's old values) are in the
            # units of the statistics that include this rollout's returns.  Advantages stay raw.
            self.value_norm.update(b_returns.reshape(-1, 1))
            b_returns = self.value_norm.normalize(b_returns.reshape(-1, 1)).reshape(-1)
            if self.clip_vloss:
                b_values = self.value_norm.normalize(b_values.reshape(-1, 1)).reshape(-1)
        with self._inputs_prenormalized():
            stats = self._update(T, N, b_obs, b_pomdps, actions.reshape(T * N, -1), logprobs.reshape(-1),
                                 dones.reshape(-1), advantages.reshape(-1), b_returns, b_values, initial_lstm_state)
        if self.normalize_input:
            self.actor_norm.update(raw_pomdps)
            self.critic_norm.update(raw_obs)
        if self.value_bootstrap:
            # the share of the T·N transitions whose successor was a time-out (rows 1.. and next_timeout; row 0
            # belongs to the rollout before; any non-zero byte counts): one reduction, read by whoever reads the stats
            flags = torch.cat([timeouts[1:].reshape(-1), next_timeout.reshape(-1)])
            stats["timeout_frac"] = torch.count_nonzero(flags) / float(T * N)
        return stats

    def _update(self, T, N, b_obs, b_pomdps, b_actions, b_logprobs, b_dones, b_advantages, b_returns, b_values,
                initial_lstm_state):
        """The epochs of minibatch steps on the flattened (T·N) rollout (``train``)."""
        flatinds = torch.arange(T * N, device=self.device).reshape(T, N)
        # the minibatch's four per-row scalars as ONE gather of their stacked rows (each result row contiguous)
        # instead of four (OUZ_STACKED_GATHER=0: one per tensor); exact either way
        scalars = [b_logprobs, b_dones, b_advantages, b_returns]
        if self.clip_vloss:   # the rollout's values (agent.py:107) as a fifth row of the same gather
            scalars.append(b_values)
        stacked = (torch.stack([x.float() for x in scalars]) if self.device.type == "cuda"
                   and os.environ.get("OUZ_STACKED_GATHER", "1") != "0" else None)
        clipfracs = torch.zeros((), device=self.device)
        n_mb = 0
        # the HIP loss kernels, with or without the entropy bonus and the clipped value loss; OUZ_FUSED_LOSS=0 keeps
        # the torch form (the yardstick, and the CPU form)
        fused_loss = self.device.type == "cuda" and os.environ.get("OUZ_FUSED_LOSS", "1") != "0"
        stats = {}
        epochs_run = 0
        for _ in range(self.update_epochs):
            epochs_run += 1
            if self.recurrent:
                envinds = self._perm(N)
                per = N // self.num_minibatches
                batches = [(flatinds[:, envinds[s:s + per]].reshape(-1), envinds[s:s + per])
                           for s in range(0, N, per)]
            else:
                b_inds = self._perm(T * N)
                batches = [(b_inds[s:s + self.minibatch_size], None) for s in range(0, T * N, self.minibatch_size)]
            for mb_inds, mbenvinds in batches:
                mb_state = ((initial_lstm_state[0][:, mbenvinds], initial_lstm_state[1][:, mbenvinds])
                            if self.recurrent else None)
                if stacked is not None:
                    mb_logp, mb_done, mb_advs, mb_ret, *mb_oldv = torch.index_select(stacked, 1, mb_inds).unbind(0)
                else:
                    mb_logp, mb_done, mb_advs, mb_ret, *mb_oldv = (x[mb_inds] for x in scalars)
                mb_pomdps, mb_obs = b_pomdps.index_select(0, mb_inds), b_obs.index_select(0, mb_inds)
                mb_actions = b_actions.index_select(0, mb_inds)
                if fused_loss:
                    # the HIP losses (fused.PolicyLossEnt / ValueLoss / ValueLossClipped): same quantities, ~5 launches
                    # instead of ~60
                    mean_z = (self.actor.update_mean(mb_pomdps, mb_state, mb_done) if self.recurrent
                              else self.actor.update_mean(mb_pomdps))
                    # (with ent_coef 0 the entropy entry's loss and gradients are PolicyLoss's bit for bit, in the same
                    # three launches; it also reports the entropy)
                    actor_loss, pg_loss, ent_mean, approx_kl, clipfrac = PolicyLossEnt.apply(
                        mean_z, self.actor.actor_logstd, mb_actions, mb_logp,
                        mb_advs, self.clip_coef, self.norm_adv, self.ent_coef)
                    newvalue = self.critic(mb_obs).view(-1)
                    if self.clip_vloss:
                        v_loss, v_clipfrac = ValueLossClipped.apply(newvalue, mb_oldv[0], mb_ret, self.clip_coef)
                    else:
                        v_loss = ValueLoss.apply(newvalue, mb_ret)
                    clipfracs += clipfrac
                    n_mb += 1
                else:
                    if self.recurrent:
                        _, newlogprob, entropy, _ = self.actor(mb_pomdps, mb_state, mb_done,
                                                               mb_actions)
                    else:
                        _, newlogprob, entropy = self.actor(mb_pomdps, mb_actions)
                    newvalue = self.critic(mb_obs).view(-1)
                    logratio = newlogprob - mb_logp
                    ratio = logratio.exp()
                    with torch.no_grad():
                        approx_kl = ((ratio - 1) - logratio).mean()
                        clipfracs += ((ratio - 1.0).abs() > self.clip_coef).float().mean()
                        n_mb += 1
                    mb_adv = mb_advs
                    if self.norm_adv:
                        mb_adv = (mb_adv - mb_adv.mean()) / (mb_adv.std() + 1e-8)
                    pg_loss = torch.max(-mb_adv * ratio,
                                        -mb_adv * torch.clamp(ratio, 1 - self.clip_coef, 1 + self.clip_coef)).mean()
                    if self.clip_vloss:   # agent.py:105-114
                        v_loss_unclipped = (newvalue - mb_ret) ** 2
                        v_clipped = mb_oldv[0] + torch.clamp(newvalue - mb_oldv[0], -self.clip_coef, self.clip_coef)
                        v_loss_clipped = (v_clipped - mb_ret) ** 2
                        v_loss = 0.5 * torch.max(v_loss_unclipped, v_loss_clipped).mean()
                        v_clipfrac = (v_loss_clipped > v_loss_unclipped).float().mean().detach()
                    else:
                        v_loss = 0.5 * ((newvalue - mb_ret) ** 2).mean()
                    ent_mean = entropy.mean()
                    actor_loss = pg_loss - self.ent_coef * ent_mean
                critic_loss = v_loss * self.vf_coef

                self.actor_optimizer.zero_grad()
                actor_loss.backward()
                allreduce_grads(self.actor)            # data parallel over ranks (no-op on one GPU)
                self._clip_step(0, self.actor, self.actor_optimizer)

                self.critic_optimizer.zero_grad()
                critic_loss.backward()
                allreduce_grads(self.critic)
                self._clip_step(1, self.critic, self.critic_optimizer)
                stats = {"pg_loss": pg_loss.detach(), "v_loss": v_loss.detach(), "approx_kl": approx_kl,
                         "entropy": ent_mean.detach()}
                if self.clip_vloss:
                    stats["v_clipfrac"] = v_clipfrac
            if self.target_kl is not None and float(stats["approx_kl"]) > self.target_kl:
                break
        stats["clipfrac"] = clipfracs / max(n_mb, 1)
        if self.target_kl is not None:
            stats["epochs_run"] = epochs_run
        return stats

    def _clip_step(self, which, net, optimizer):
        """clip_grad_norm_(net, max_grad_norm) + optimizer.step() (agent.py:124-134)."""
        if self._clip_adam is not None:
            self._clip_adam[which].step(self.max_grad_norm)
        else:
            nn.utils.clip_grad_norm_(net.parameters(), self.max_grad_norm)
            optimizer.step()
            if self._shadows is not None:     # one multi-tensor cast after torch's step
                self._shadows[which].refresh()

    # -------------------------------------------------------------- checkpoints
    def save(self, filename):
        """Same four files as agent.py:127-131; with ``normalize_input`` / ``normalize_value`` a fifth,
        ``<filename>_normalizers``: the f64 statistics of each normaliser in use."""
        torch.save(self.critic.state_dict(), filename + "_critic")
        torch.save(self.critic_optimizer.state_dict(), filename + "_critic_optimizer")
        torch.save(self.actor.state_dict(), filename + "_actor")
        torch.save(self.actor_optimizer.state_dict(), filename + "_actor_optimizer")
        norms = self._normalizers()
        if norms:
            torch.save({k: n.state_dict() for k, n in norms.items()}, filename + "_normalizers")

    def _normalizers(self):
        return {k: n for k, n in (("actor_input", self.actor_norm), ("critic_input", self.critic_norm),
                                  ("value", self.value_norm)) if n is not None}

    def load(self, filename):
        """agent.py:133-139; tensors only (weights_only).  With a normalisation flag on, the fifth file is required
        (a policy trained on normalised inputs is another function of the raw ones)."""
        m = self.device
        norms = self._normalizers()
        if norms:
            path = filename + "_normalizers"
            if not os.path.exists(path):
                raise FileNotFoundError(f"{path}: this learner normalises ({', '.join(norms)}) and needs the "
                                        "statistics the checkpoint was trained with")
            saved = torch.load(path, map_location=m, weights_only=True)
            missing = [k for k in norms if k not in saved]
            if missing:
                raise KeyError(f"{path} holds no statistics for {missing}")
            for k, n in norms.items():
                n.load_state(saved[k])
        self.critic.load_state_dict(torch.load(filename + "_critic", map_location=m, weights_only=True))
        self.critic_optimizer.load_state_dict(torch.load(filename + "_critic_optimizer", map_location=m,
                                                         weights_only=True))
        self.actor.load_state_dict(torch.load(filename + "_actor", map_location=m, weights_only=True))
        self.actor_optimizer.load_state_dict(torch.load(filename + "_actor_optimizer", map_location=m,
                                                        weights_only=True))
        self.refresh_shadows()


class GraphedPolicy:
    """The rollout step's policy call (trunk MLP, input projection, LSTM GEMM + fused cell kernel,
    mean head, Normal sample, log-prob, entropy: ~25 launches) captured once in a hipGraph and
    replayed per step.  Eagerly each of those launches costs several µs of host time, ~440 µs per
    4096-env step in all, 100x the env step; a replay is one host call.

    Inputs are copied into static buffers before each replay; the parameters are read in place
    (Adam updates them in place, so every replay sees the current policy).  The sample's standard
    normal draws are made by ``normal_`` into a static buffer before each replay (models._policy_head:
    the sample is mean + std * eps).  The LSTM's final carry is written into the static carry input
    buffers themselves (``LSTMActor.carry_inplace``), so a carry handed back from the previous replay
    (``alias=True``) needs no copy; any other carry is copied in.
    """

    def __init__(self, learner, warmup=3):
        self.learner = learner
        self.warmup = warmup
        self.graph = None

    def _capture(self, state, lstm_state, done):
        ln = self.learner
        self.s_in = state.detach().clone()
        self.s_done = done.detach().clone()
        self.s_lstm = (lstm_state[0].detach().clone(), lstm_state[1].detach().clone()) if ln.recurrent else None
        self.s_eps = torch.zeros((state.shape[0], ln.actor.actor_logstd.shape[1]), device=ln.device)
        side = torch.cuda.Stream(device=ln.device)
        side.wait_stream(torch.cuda.current_stream(ln.device))
        # the LSTM's final carry is written back into the static input buffers (models.LSTMActor.carry_inplace),
        # so the replay's output carry IS its next input: no copy in or out when the caller hands it back
        if ln.recurrent and os.environ.get("OUZ_GRAPH_CARRY_INPLACE", "1") != "0":
            ln.actor.carry_inplace = self.s_lstm
        try:
            with torch.cuda.stream(side):   # warm-up: lazy workspaces / kernels resolved outside the capture
                for _ in range(self.warmup):
                    ln.get_action(self.s_in, self.s_lstm, self.s_done, eps=self.s_eps)
            torch.cuda.current_stream(ln.device).wait_stream(side)
            self.graph = torch.cuda.CUDAGraph()
            # relaxed: the caching allocator may map a fresh segment for the graph's private pool during
            # the capture
            with torch.cuda.graph(self.graph, capture_error_mode="relaxed"):
                self.out = ln.get_action(self.s_in, self.s_lstm, self.s_done, eps=self.s_eps)
        finally:
            if ln.recurrent:
                ln.actor.carry_inplace = None

    def _matches(self, state, lstm_state, done):
        """The call has the captured shapes, dtypes and device (a broadcastable but different batch would
        otherwise be silently broadcast by copy_ into the static buffers)."""
        def same(a, b):
            return a.shape == b.shape and a.dtype == b.dtype and a.device == b.device
        if not (same(state, self.s_in) and same(done, self.s_done)):
            return False
        if self.s_lstm is None:
            return lstm_state is None
        return lstm_state is not None and same(lstm_state[0], self.s_lstm[0]) and same(lstm_state[1], self.s_lstm[1])

    def __call__(self, state, lstm_state, done, alias=False):
        """One replay.  ``alias=False`` (the default) returns copies, as ``get_action`` would; ``alias=True``
        returns the graph's output buffers themselves, which the next replay overwrites (the rollout loop
        copies them into its storage right away, train.py)."""
        if self.graph is None or not self._matches(state, lstm_state, done):
            self._capture(state, lstm_state, done)
        self.s_in.copy_(state)
        self.s_done.copy_(done)
        self.s_eps.normal_()
        if self.s_lstm is not None:
            for dst, src in zip(self.s_lstm, lstm_state):
                if src is not dst:          # the previous replay's carry handed back (alias=True): already there
                    dst.copy_(src)
        self.graph.replay()
        if alias:
            return self.out
        return tuple(None if x is None else (tuple(y.clone() for y in x) if isinstance(x, tuple) else x.clone())
                     for x in self.out)
