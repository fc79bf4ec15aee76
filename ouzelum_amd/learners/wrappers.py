"""gym-free equivalents of the learners' env glue (``gym`` is not installed here).

* ``ExtractObsWrapper``         PPO/utils.py:37-39, RPO-LSTM/utils.py:36-38
* ``RecordEpisodeStatisticsTorch`` RPO-LSTM/utils.py:4-34 (same info["r"] / info["l"])
* ``EpisodeRecorder``           the same statistics as one ``ouz_episode_step`` launch, with the records of the
  finished episodes that PPO/main.py:98-103 logs one by one, read once per rollout
* ``POMDPWrapper``              utils/POMDP.py:5-43, evaluated by the HIP kernel
  ``ouz_pomdp_obs`` (one launch, device counter-RNG) instead of a CPU coin / CPU noise
  tensor copied to ``cuda:0`` on every call.
"""
import numpy as np
import torch

from .. import _lib as L


class _Wrapper:
    def __init__(self, env):
        self.env = env

    def __getattr__(self, name):          # forward everything else (num_envs, spaces, ...)
        return getattr(self.env, name)

    def reset(self, **kw):
        return self.env.reset(**kw)

    def step(self, action):
        return self.env.step(action)


class ExtractObsWrapper(_Wrapper):
    """obs dict -> the "obs" tensor."""

    def reset(self, **kw):
        return self.env.reset(**kw)["obs"]

    def step(self, action):
        obs, rew, done, info = self.env.step(action)
        return obs["obs"], rew, done, info


class RecordEpisodeStatisticsTorch(_Wrapper):
    """Running episodic return / length per env on the device; info["r"], info["l"] hold the
    values at the current step (before the done envs are zeroed)."""

    def __init__(self, env, device):
        super().__init__(env)
        self.num_envs = getattr(env, "num_envs", 1)
        self.device = device

    def reset(self, **kw):
        obs = self.env.reset(**kw)
        n, d = self.num_envs, self.device
        self.episode_returns = torch.zeros(n, dtype=torch.float32, device=d)
        self.episode_lengths = torch.zeros(n, dtype=torch.int32, device=d)
        self.returned_episode_returns = torch.zeros(n, dtype=torch.float32, device=d)
        self.returned_episode_lengths = torch.zeros(n, dtype=torch.int32, device=d)
        return obs

    def step(self, action):
        obs, rew, done, info = self.env.step(action)
        self.episode_returns += rew
        self.episode_lengths += 1
        self.returned_episode_returns.copy_(self.episode_returns)
        self.returned_episode_lengths.copy_(self.episode_lengths)
        self.episode_returns *= 1 - done
        self.episode_lengths *= 1 - done
        info["r"] = self.returned_episode_returns
        info["l"] = self.returned_episode_lengths
        return obs, rew, done, info


RECORD_DTYPE = np.dtype([("tag", "<i4"), ("env_id", "<i4"), ("ret", "<f4"), ("len", "<i4")])   # ouz_episode_record


def sort_records(rec):
    """Records ordered by (tag, env id): the order of the reference's step loop over ascending env indices."""
    return rec[np.lexsort((rec["env_id"], rec["tag"]))]


def merge_records(shards):
    """The records of every rank (env ids already global: ``env_id0`` is the rank's ``env_id_offset``) as one array
    ordered by (tag, global env id), so the event file does not depend on the rank count."""
    shards = [np.asarray(s, dtype=RECORD_DTYPE) for s in shards]
    return sort_records(np.concatenate(shards) if shards else np.empty(0, RECORD_DTYPE))


class EpisodeRecorder(_Wrapper):
    """``RecordEpisodeStatisticsTorch`` (same info["r"] / info["l"], bitwise) as ONE ``ouz_episode_step`` launch per
    step on HIP tensors, with the records of the finished episodes the reference logs one ``.item()`` at a time
    (PPO/main.py:98-103) appended on the device and read once per rollout:

        rec.begin_rollout()                 # count = 0
        rec.record(step); rec.step(action)  # the armed step appends {tag, env_id0 + i, r, l} of its done envs
        ... torch.cuda.synchronize() ...
        rec.drain()                         # numpy RECORD_DTYPE, sorted by (tag, env_id)

    On CPU tensors ``step`` is the same math as torch ops plus ``nonzero``."""

    def __init__(self, env, device, env_id0=0, capacity=None):
        super().__init__(env)
        self.num_envs = getattr(env, "num_envs", 1)
        self.device = torch.device(device)
        self.env_id0 = int(env_id0)
        self.capacity = int(capacity) if capacity is not None else 3 * self.num_envs   # rollout steps 0-2
        if self.capacity <= 0:
            raise ValueError("capacity must be > 0")
        self._tag = None
        self._host = []      # CPU tensors: the records themselves
        self._total = 0

    def _allocate(self):
        n, d = self.num_envs, self.device
        self.episode_returns = torch.zeros(n, dtype=torch.float32, device=d)
        self.episode_lengths = torch.zeros(n, dtype=torch.int32, device=d)
        self.returned_episode_returns = torch.zeros(n, dtype=torch.float32, device=d)
        self.returned_episode_lengths = torch.zeros(n, dtype=torch.int32, device=d)
        self.records = torch.zeros((self.capacity, 4), dtype=torch.int32, device=d)   # torch allocations: 16-byte aligned
        self.count = torch.zeros(1, dtype=torch.int32, device=d)

    def reset(self, **kw):
        obs = self.env.reset(**kw)
        self._allocate()
        self._host, self._total, self._tag = [], 0, None
        return obs

    def begin_rollout(self):
        self.count.zero_()
        self._host, self._total = [], 0

    def record(self, tag):
        """Arm the next ``step``: its done envs are appended under ``tag``."""
        self._tag = int(tag)

    def update(self, rew, done):
        """The statistics of one step from its ``rew`` (f32) and ``done`` (int64); ``step`` without the env."""
        tag, self._tag = self._tag, None
        if rew.device.type == "cuda":
            L.require_hip_tensor(rew, "rew")
            L.require_hip_tensor(done, "done")
            if rew.dtype != torch.float32 or done.dtype != torch.int64 or rew.numel() != self.num_envs \
                    or done.numel() != self.num_envs:
                raise ValueError("rew must be (N,) float32 and done (N,) int64")
            L.check(L.lib.ouz_episode_step(
                L.ptr(rew), L.ptr(done), L.ptr(self.episode_returns), L.ptr(self.episode_lengths),
                L.ptr(self.returned_episode_returns), L.ptr(self.returned_episode_lengths), self.num_envs,
                tag if tag is not None else 0, self.env_id0, L.ptr(self.records) if tag is not None else None,
                self.capacity, L.ptr(self.count) if tag is not None else None, L.stream_ptr(rew.device)),
                "ouz_episode_step")
            return
        self.episode_returns += rew
        self.episode_lengths += 1
        self.returned_episode_returns.copy_(self.episode_returns)
        self.returned_episode_lengths.copy_(self.episode_lengths)
        self.episode_returns *= 1 - done
        self.episode_lengths *= 1 - done
        if tag is not None:
            idx = done.nonzero(as_tuple=False).flatten()
            rec = np.empty(idx.numel(), RECORD_DTYPE)
            rec["tag"] = tag
            rec["env_id"] = self.env_id0 + idx.numpy()
            rec["ret"] = self.returned_episode_returns[idx].numpy()
            rec["len"] = self.returned_episode_lengths[idx].numpy()
            self._total += len(rec)
            self._host.append(rec[:max(0, self.capacity - (self._total - len(rec)))])

    def step(self, action):
        obs, rew, done, info = self.env.step(action)
        self.update(rew, done)
        info["r"] = self.returned_episode_returns
        info["l"] = self.returned_episode_lengths
        return obs, rew, done, info

    def drain(self):
        """The rollout's records, sorted by (tag, env_id).  Call after the stream is synchronised: it copies the
        count, then only ``records[:count]``.  Raises if more were appended than the buffer holds."""
        if self.device.type == "cuda":
            total = int(self.count.cpu()[0])
            if total > self.capacity:
                raise L.OuzelumError(f"episode records overflowed: {total} appended, capacity {self.capacity}")
            raw = self.records[:total].cpu().numpy()
            return sort_records(np.ascontiguousarray(raw).view(RECORD_DTYPE).reshape(-1))
        if self._total > self.capacity:
            raise L.OuzelumError(f"episode records overflowed: {self._total} appended, capacity {self.capacity}")
        return merge_records(self._host)


POMDP_MODES = {"none": L.POMDP_NONE, "flicker": L.POMDP_FLICKER, "random_noise": L.POMDP_NOISE,
               "flickering_and_random_noise": L.POMDP_FLICKER_NOISE}


class POMDPWrapper:
    """Learner-side observation corruption (utils/POMDP.py).  ``observation(obs)`` returns a new
    (N, d) tensor; draws are keyed (seed, row_offset + row, call index), so a sharded run
    reproduces the unsharded one."""

    def __init__(self, pomdp="flicker", pomdp_prob=0.1, seed=0, row_offset=0):
        if pomdp not in POMDP_MODES:
            raise ValueError(f"pomdp was not in {sorted(POMDP_MODES)}!")   # POMDP.py:20
        self.pomdp = pomdp
        self.mode = POMDP_MODES[pomdp]
        self.prob = float(pomdp_prob)
        self.seed = int(seed)
        self.row_offset = int(row_offset)
        self.calls = 0

    def observation(self, obs, out=None):
        L.require_hip_tensor(obs, "obs")
        if obs.dtype != torch.float32 or obs.dim() != 2:
            raise ValueError("obs must be a (N, d) float32 tensor")
        out = torch.empty_like(obs) if out is None else out
        L.check(L.lib.ouz_pomdp_obs(L.ptr(obs), L.ptr(out), obs.shape[0], obs.shape[1], self.mode, self.prob,
                                    self.seed, self.row_offset, self.calls & 0xFFFFFFFF, L.stream_ptr(obs.device)),
                "ouz_pomdp_obs")
        self.calls += 1
        return out
