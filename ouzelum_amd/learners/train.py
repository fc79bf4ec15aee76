"""Recurrent PPO / RPO-LSTM training driver on the HIP env (RPO-LSTM/main.py:28-124, PPO/main.py).

    python -m ouzelum_amd.learners.train --env Landing --num_envs 4096 --POMDP flicker --pomdp_prob 0.1

Same loop as the reference: T-step rollout with the LSTM carry reset on done, the
actor acting on the clean observations and training on the learner-side POMDP ones
(App. B item 10; ``--rollout_obs pomdp`` gives the RPO-LSTM_Critic variant), one
PPO update per rollout, best/final checkpoints under the reference's file names.
The reference's TensorBoard scalars (PPO/main.py:101-109: ``charts/episodic_return``, ``charts/episodic_length``,
``average/average_reward``) go to a TensorBoard event file in ``<logdir>/<run>/`` (the reference's
``SummaryWriter("../runs/<run>")``; written by ``tbevents.py``, tensorboard itself is not installed), one point per
rollout: the mean return / length of the episodes that finished in it, where the reference logs the episodes that
end in the rollout's first three steps one by one.  Every logged column also goes to ``<logdir>/<run>.csv``.  Episode
statistics are the env's in-kernel [sum, count] (``ouz_episode_stats``), all-reduced
over RCCL when launched with torchrun (one process per GPU, env ids sharded).

``--learner NAME`` runs one of the reference's seven learners by its directory name (``PPO``, ``RPO``, ``PPO-LSTM``,
``RPO-LSTM_Critic``, ``PPO_Critic``, ``RPO_Critic``, ``RPO-LSTM``; the table is ``variants.py``): it decides the actor
(MLP / LSTM), ``rpo_alpha`` in the update, which observation the policy acts on and the critic values, and the names
of the run directory, the final and the best checkpoint, so curves and checkpoints lie over the reference's.  It
cannot be combined with ``--algo`` / ``--rollout_obs``, which keep their own (older) loop unchanged.  On this path
the per-step episode bookkeeping is one ``ouz_episode_step`` launch (``wrappers.EpisodeRecorder``), and
``--episode_log per_episode`` writes the reference's points: one ``charts/episodic_return`` /
``charts/episodic_length`` pair per episode that ends in rollout steps 0-2, env ids ascending, at that step's
``global_step`` (PPO/main.py:98-103).  The rollout loop reads nothing back for them: the kernel appends the records
on the device, and the host reads the count and ``records[:count]`` once per rollout, after the synchronize the
loop already has.  ``--play --learner NAME`` runs NAME's networks from ``--checkpoint`` on the observations NAME's
rollout feeds its policy and logs ``reward/play``.
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
from .variants import LEARNERS, VARIANTS, names, single_stream
from .wrappers import (RECORD_DTYPE, EpisodeRecorder, ExtractObsWrapper, POMDPWrapper, RecordEpisodeStatisticsTorch,
                       merge_records)


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
    p.add_argument("--episode_log", default="rollout_mean", choices=["rollout_mean", "per_episode"],
                   help="charts/* points: one mean per rollout, or the reference's one per episode (with --learner)")
    args = p.parse_args(argv)
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


def train_learner(args, on_rollout=None):
    """``train`` for ``--learner NAME``: the same loop with NAME's routing and names (variants.py), the episode
    bookkeeping as one launch per step, and optionally the reference's per-episode points.  ``on_rollout(dict)``, if
    given, is called once per rollout (after the update and the synchronize) with the rollout's tensors: ``obs`` and
    ``pomdps`` storage (``pomdps`` None for the single-stream learners), the bootstrap ``next_obs``, ``acted_on``
    (T, N, d: what the policy was given at each step), ``dones`` (T, N: ``next_done`` after each step),
    ``r`` / ``l`` (T, N: info["r"] / info["l"] after each step), ``global_step_before`` and ``stats``."""
    v = VARIANTS[args.learner]
    single = single_stream(v)
    per_episode = args.episode_log == "per_episode"
    rank, world, local = init_from_env()
    device = torch.device("cuda", local)
    torch.cuda.set_device(device)
    np.random.seed(args.seed + rank)
    torch.manual_seed(args.seed + rank)
    N, T = args.num_envs, args.rollout_steps
    off, total = shard(N, rank, world)

    base = make(seed=args.seed, task=args.env, num_envs=N, sim_device=str(device), rl_device=str(device),
                graphics_device_id=-1, headless=True, env_id_offset=off, num_envs_total=total, track_episodes=True)
    envs = EpisodeRecorder(ExtractObsWrapper(base), device, env_id0=off, capacity=3 * N)
    pomdp_w = POMDPWrapper(args.POMDP, args.pomdp_prob, seed=args.seed + 1, row_offset=off)
    agent = PPOLearner(base.observation_space, base.action_space, N, device, recurrent=v.recurrent,
                       rollout_steps=T, rpo_alpha=v.rpo_alpha)
    name, best = names(args.learner, args.POMDP, args.pomdp_prob)

    obs_shape = base.observation_space.shape
    obs = torch.zeros((T, N) + obs_shape, device=device)
    pomdps = None if single else torch.zeros((T, N) + obs_shape, device=device)
    actions = torch.zeros((T, N) + base.action_space.shape, device=device)
    logprobs = torch.zeros((T, N), device=device)
    rewards = torch.zeros((T, N), device=device)
    dones = torch.zeros((T, N), device=device)
    if on_rollout is not None:
        seen = {"acted_on": torch.zeros((T, N) + obs_shape, device=device),
                "dones": torch.zeros((T, N), dtype=torch.int64, device=device),
                "r": torch.zeros((T, N), device=device), "l": torch.zeros((T, N), dtype=torch.int32, device=device)}

    writer = tb = None
    if rank == 0:
        os.makedirs(args.logdir, exist_ok=True)
        tb = EventWriter(os.path.join(args.logdir, name))
        fh = open(os.path.join(args.logdir, name + ".csv"), "w", newline="")
        writer = csv.writer(fh)
        writer.writerow(["global_step", "average_reward", "episodes", "episodic_return", "episodic_length",
                         "pg_loss", "v_loss", "approx_kl", "clipfrac", "env_steps_per_s"])

    global_step = 0
    max_reward = -float("inf")
    next_obs = envs.reset()
    pomdp = next_obs.clone()              # the first observation of a run is the clean one (main.py:80-82)
    if single:
        next_obs = pomdp                  # a tensor of its own: the env overwrites its observation buffer in place
    next_done = torch.zeros(N, device=device)
    lstm_state = agent.initial_state()
    history = []
    t_start = time.perf_counter()
    while global_step < args.total_steps:
        t0 = time.perf_counter()
        g0 = global_step
        init_state = (lstm_state[0].clone(), lstm_state[1].clone()) if lstm_state is not None else None
        if per_episode:
            envs.begin_rollout()
        for step in range(T):
            global_step += N * world
            if single:
                store((obs[step], dones[step]), (next_obs, next_done))
                act_in = next_obs
            else:
                store((pomdps[step], obs[step], dones[step]), (pomdp, next_obs, next_done))
                act_in = pomdp if v.acts_on == "pomdp" else next_obs
            if on_rollout is not None:
                seen["acted_on"][step].copy_(act_in)
            action, logprob, _, lstm_state = agent.act(act_in, lstm_state, next_done, alias=True)
            store((actions[step], logprobs[step]), (action, logprob))
            if per_episode and step <= 2:         # PPO/main.py:98: if 0 <= step <= 2
                envs.record(step)
            next_obs, rewards[step], next_done, info = envs.step(action)
            if single:
                next_obs = pomdp_w.observation(next_obs)     # PPO/main.py:96
            else:
                pomdp = pomdp_w.observation(next_obs)        # RPO-LSTM/main.py:103
            if on_rollout is not None:
                store((seen["dones"][step], seen["r"][step], seen["l"][step]), (next_done, info["r"], info["l"]))
        stats = agent.train(obs, obs if single else pomdps, actions, next_obs, next_done, init_state, logprobs,
                            rewards, dones)
        ep = base.episode_stats()
        mean_rew = rewards.mean()
        merged = None
        if world > 1:
            dist.all_reduce(ep)
            dist.all_reduce(mean_rew)
            mean_rew /= world
            if per_episode:
                merged = gather_records(envs, world)
        torch.cuda.synchronize(device)
        base.check_health()
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
            on_rollout({"obs": obs, "pomdps": pomdps, "next_obs": next_obs, **seen, "global_step_before": g0,
                        "stats": stats, "records": records})
        if rank == 0:
            writer.writerow([row[k] for k in ("global_step", "average_reward", "episodes", "episodic_return",
                                              "episodic_length", "pg_loss", "v_loss", "approx_kl", "clipfrac",
                                              "env_steps_per_s")])
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


def train(args, on_rollout=None):
    if getattr(args, "learner", None) is not None:
        return train_learner(args, on_rollout)
    if on_rollout is not None:
        raise ValueError("on_rollout is a hook of the --learner loop")
    rank, world, local = init_from_env()
    device = torch.device("cuda", local)
    torch.cuda.set_device(device)
    np.random.seed(args.seed + rank)
    torch.manual_seed(args.seed + rank)
    N, T = args.num_envs, args.rollout_steps
    off, total = shard(N, rank, world)

    base = make(seed=args.seed, task=args.env, num_envs=N, sim_device=str(device), rl_device=str(device),
                graphics_device_id=-1, headless=True, env_id_offset=off, num_envs_total=total, track_episodes=True)
    envs = RecordEpisodeStatisticsTorch(ExtractObsWrapper(base), device)
    pomdp_w = POMDPWrapper(args.POMDP, args.pomdp_prob, seed=args.seed + 1, row_offset=off)
    agent = PPOLearner(base.observation_space, base.action_space, N, device, recurrent=args.algo == "rpo_lstm",
                       rollout_steps=T)
    name = f"{'RPO_LSTM' if args.algo == 'rpo_lstm' else 'PPO'}_{args.POMDP}_{args.pomdp_prob}"

    obs_shape = base.observation_space.shape
    obs = torch.zeros((T, N) + obs_shape, device=device)
    pomdps = torch.zeros((T, N) + obs_shape, device=device)
    actions = torch.zeros((T, N) + base.action_space.shape, device=device)
    logprobs = torch.zeros((T, N), device=device)
    rewards = torch.zeros((T, N), device=device)
    dones = torch.zeros((T, N), device=device)

    writer = tb = None
    if rank == 0:
        os.makedirs(args.logdir, exist_ok=True)
        tb = EventWriter(os.path.join(args.logdir, name))
        fh = open(os.path.join(args.logdir, name + ".csv"), "w", newline="")
        writer = csv.writer(fh)
        writer.writerow(["global_step", "average_reward", "episodes", "episodic_return", "episodic_length",
                         "pg_loss", "v_loss", "approx_kl", "clipfrac", "env_steps_per_s"])

    global_step = 0
    max_reward = -float("inf")
    next_obs = envs.reset()
    pomdp = next_obs.clone()
    next_done = torch.zeros(N, device=device)
    lstm_state = agent.initial_state()
    history = []
    t_start = time.perf_counter()
    while global_step < args.total_steps:
        t0 = time.perf_counter()
        init_state = (lstm_state[0].clone(), lstm_state[1].clone()) if lstm_state is not None else None
        for step in range(T):
            global_step += N * world
            store((pomdps[step], obs[step], dones[step]), (pomdp, next_obs, next_done))
            act_in = pomdp if args.rollout_obs == "pomdp" else next_obs
            action, logprob, _, lstm_state = agent.act(act_in, lstm_state, next_done, alias=True)
            store((actions[step], logprobs[step]), (action, logprob))
            next_obs, rewards[step], next_done, info = envs.step(action)
            pomdp = pomdp_w.observation(next_obs)
        stats = agent.train(obs, pomdps, actions, next_obs, next_done, init_state, logprobs, rewards, dones)
        ep = base.episode_stats()
        mean_rew = rewards.mean()
        if world > 1:
            dist.all_reduce(ep)
            dist.all_reduce(mean_rew)
            mean_rew /= world
        torch.cuda.synchronize(device)
        base.check_health()   # raises if a fused rollout's split-wave wait gave up (never on the per-step path)
        sps = N * world * T / (time.perf_counter() - t0)
        row = {"global_step": global_step, "average_reward": float(mean_rew), "episodes": int(ep[1]),
               "episodic_return": float(ep[0] / ep[1]) if float(ep[1]) > 0 else float("nan"),
               "episodic_length": float(ep[2] / ep[1]) if float(ep[1]) > 0 else float("nan"),
               **{k: float(v) for k, v in stats.items()}, "env_steps_per_s": sps}
        history.append(row)
        if rank == 0:
            writer.writerow([row[k] for k in ("global_step", "average_reward", "episodes", "episodic_return",
                                              "episodic_length", "pg_loss", "v_loss", "approx_kl", "clipfrac",
                                              "env_steps_per_s")])
            if row["episodes"] > 0:
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
                agent.save(os.path.join(args.checkpoint_dir, f"best_reward_{args.POMDP}_{args.pomdp_prob}"))
    if rank == 0:
        if not args.no_checkpoints:
            agent.save(os.path.join(args.checkpoint_dir, name))
        fh.close()
        tb.close()
    elapsed = time.perf_counter() - t_start
    return {"history": history, "agent": agent, "env": base, "elapsed": elapsed, "events": tb.path if tb else None,
            "env_steps_per_s": global_step / elapsed}


@torch.no_grad()
def play(args):
    """RPO-LSTM/play.py:25-80: load a checkpoint and run the policy, printing the mean reward."""
    device = torch.device("cuda", 0)
    N = args.num_envs
    base = make(seed=args.seed, task=args.env, num_envs=N, sim_device=str(device), rl_device=str(device),
                track_episodes=True)
    env = ExtractObsWrapper(base)
    agent = PPOLearner(base.observation_space, base.action_space, N, device, recurrent=args.algo == "rpo_lstm",
                       rollout_steps=args.rollout_steps, tuned_gemms=False)   # inference only
    if args.checkpoint:
        agent.load(args.checkpoint)
    next_obs = env.reset()
    next_done = torch.zeros(N, device=device)
    lstm = agent.initial_state()
    rewards = []
    for _ in range(max(1, args.total_steps // N)):
        action, _, _, lstm = agent.act(next_obs, lstm, next_done)
        next_obs, rew, next_done, _ = env.step(action)
        rewards.append(rew.mean())
        if not args.quiet:
            print(f"Average rewards {float(rewards[-1]):.4f}")
    return {"mean_reward": float(torch.stack(rewards).mean()), "episode_stats": base.episode_stats().tolist()}


@torch.no_grad()
def play_learner(args):
    """``--play --learner NAME``: NAME's networks (variants.py) from ``--checkpoint``, fed what NAME's rollout feeds
    its policy: the POMDP observation for the five learners that act on it, the clean one for PPO-LSTM and RPO-LSTM;
    the first observation is the clean reset, as in training.  Logs the reference's ``reward/play`` scalar (the
    step's mean reward at ``global_step``, RPO-LSTM_Critic/play.py:78-94) to an event file under ``--logdir``.
    (The reference's RPO/play.py is a stale copy that skips the corruption; this follows the table.)"""
    v = VARIANTS[args.learner]
    device = torch.device("cuda", 0)
    N = args.num_envs
    base = make(seed=args.seed, task=args.env, num_envs=N, sim_device=str(device), rl_device=str(device),
                track_episodes=True)
    env = ExtractObsWrapper(base)
    agent = PPOLearner(base.observation_space, base.action_space, N, device, recurrent=v.recurrent,
                       rollout_steps=args.rollout_steps, tuned_gemms=False, rpo_alpha=v.rpo_alpha)   # inference only
    if args.checkpoint:
        agent.load(args.checkpoint)
    pomdp_w = POMDPWrapper(args.POMDP, args.pomdp_prob, seed=args.seed + 1)
    name, _ = names(args.learner, args.POMDP, args.pomdp_prob)
    tb = EventWriter(os.path.join(args.logdir, name + "_play"))
    act_in = env.reset().clone()
    next_done = torch.zeros(N, device=device)
    lstm = agent.initial_state()
    rewards, global_step = [], 0
    for _ in range(max(1, args.total_steps // N)):
        global_step += N
        action, _, _, lstm = agent.act(act_in, lstm, next_done)
        next_obs, rew, next_done, _ = env.step(action)
        act_in = pomdp_w.observation(next_obs) if v.acts_on == "pomdp" else next_obs
        rewards.append(rew.mean())
        tb.add_scalar("reward/play", float(rewards[-1]), global_step)
        if not args.quiet:
            print(f"Step: {global_step}, Average rewards {float(rewards[-1]):.4f}")
    tb.close()
    return {"mean_reward": float(torch.stack(rewards).mean()), "episode_stats": base.episode_stats().tolist(),
            "events": tb.path}


def main(argv=None):
    args = parse_args(argv)
    if args.play:
        return play_learner(args) if args.learner is not None else play(args)
    out = train(args)
    if dist.is_initialized():
        dist.destroy_process_group()
    return out


if __name__ == "__main__":
    main()
