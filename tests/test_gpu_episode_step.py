"""``ouz_episode_step`` on the MI355X against ``RecordEpisodeStatisticsTorch`` (PPO/utils.py:20-35) and the
reference's per-env logging loop (PPO/main.py:98-103), restated here: statistics bitwise, the records of the done
envs exact, the capacity respected.  Sizes: one lane, a ragged wave, exact wave (64) and block (256) edges, several
blocks; the ragged last wave is where a wave-aggregated append can go wrong."""
import numpy as np
import pytest
import torch

from ouzelum_amd import _lib as L
from ouzelum_amd.learners.wrappers import RECORD_DTYPE, EpisodeRecorder, RecordEpisodeStatisticsTorch

pytestmark = pytest.mark.gpu

ENV_ID0 = 4096
SIZES = [1, 63, 64, 65, 255, 256, 257, 1000]
PATTERNS = ["none", "all", "first", "last", "alternating", "random"]


class ScriptedEnv:
    """step() hands out pre-made (rew, done) pairs, as VecTask.step does: f32 rewards, int64 dones."""

    def __init__(self, rews, dones):
        self.num_envs = rews[0].numel()
        self.rews, self.dones, self.k = rews, dones, 0

    def reset(self):
        self.k = 0
        return None

    def step(self, action):
        k, self.k = self.k, self.k + 1
        return None, self.rews[k], self.dones[k], {}


def done_pattern(name, n, rng):
    d = np.zeros(n, np.int64)
    if name == "all":
        d[:] = 1
    elif name == "first":
        d[0] = 1
    elif name == "last":
        d[n - 1] = 1
    elif name == "alternating":
        d[::2] = 1
    elif name == "random":
        d[:] = rng.random(n) < 0.3
    return d


def scripted(n, pattern, steps, seed):
    rng = np.random.default_rng(seed)
    rews = [torch.as_tensor((rng.standard_normal(n) * 3).astype(np.float32), device="cuda") for _ in range(steps)]
    dones = [torch.as_tensor(done_pattern(pattern, n, rng), device="cuda") for _ in range(steps)]
    return rews, dones


def bits(t):
    return t.view(torch.int32).cpu().numpy()


def reference_loop(tag, env_id0, done, r, l):
    """PPO/main.py:98-103: for idx, d in enumerate(next_done): if d: ... info["r"][idx].item(), info["l"][idx].item()"""
    out = []
    for idx, d in enumerate(done.tolist()):
        if d:
            out.append((tag, env_id0 + idx, r[idx], l[idx]))
    return out


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", SIZES)
def test_kernel_matches_wrapper_and_reference_loop(n, pattern):
    steps = 3
    rews, dones = scripted(n, pattern, steps, seed=n * 7 + PATTERNS.index(pattern))
    old = RecordEpisodeStatisticsTorch(ScriptedEnv(rews, dones), torch.device("cuda"))
    new = EpisodeRecorder(ScriptedEnv(rews, dones), "cuda", env_id0=ENV_ID0)
    old.reset()
    new.reset()
    new.begin_rollout()
    want, total = [], 0
    for s in range(steps):
        _, _, d_old, info_old = old.step(None)
        new.record(s)
        _, _, _, info_new = new.step(None)
        np.testing.assert_array_equal(bits(info_new["r"]), bits(info_old["r"]))
        np.testing.assert_array_equal(info_new["l"].cpu().numpy(), info_old["l"].cpu().numpy())
        np.testing.assert_array_equal(bits(new.episode_returns), bits(old.episode_returns))     # -0.0 counts
        np.testing.assert_array_equal(new.episode_lengths.cpu().numpy(), old.episode_lengths.cpu().numpy())
        assert info_new["l"].dtype == torch.int32 and info_new["r"].dtype == torch.float32
        want += reference_loop(s, ENV_ID0, d_old.cpu().numpy(), info_old["r"].cpu().numpy(),
                               info_old["l"].cpu().numpy())
        total += int(dones[s].sum())
    torch.cuda.synchronize()
    assert int(new.count.cpu()[0]) == total == len(want)
    got = new.drain()
    assert got.dtype == RECORD_DTYPE and len(got) == total
    want = np.array(want, dtype=RECORD_DTYPE)
    for f in ("tag", "env_id", "len"):
        np.testing.assert_array_equal(got[f], want[f])
    np.testing.assert_array_equal(got["ret"].view(np.int32), want["ret"].view(np.int32))


def test_capacity_is_respected():
    n, cap, tail = 257, 100, 64
    rews, dones = scripted(n, "all", 1, seed=3)
    rec = EpisodeRecorder(ScriptedEnv(rews, dones), "cuda", env_id0=ENV_ID0, capacity=cap)
    rec.reset()
    whole = torch.full((cap + tail, 4), -7, dtype=torch.int32, device="cuda")    # records, then the sentinel tail
    rec.records = whole[:cap]
    rec.begin_rollout()
    rec.record(5)
    _, _, _, info = rec.step(None)
    torch.cuda.synchronize()
    assert int(rec.count.cpu()[0]) == n                       # the true total, beyond the capacity
    host = whole.cpu().numpy()
    assert (host[cap:] == -7).all()                           # nothing stored past the capacity
    got = np.ascontiguousarray(host[:cap]).view(RECORD_DTYPE).reshape(-1)
    assert (got["tag"] == 5).all()
    ids = got["env_id"] - ENV_ID0
    assert len(set(ids.tolist())) == cap and ids.min() >= 0 and ids.max() < n
    r, l = info["r"].cpu().numpy(), info["l"].cpu().numpy()
    np.testing.assert_array_equal(got["ret"].view(np.int32), r[ids].view(np.int32))
    np.testing.assert_array_equal(got["len"], l[ids])
    with pytest.raises(L.OuzelumError, match="overflow"):
        rec.drain()


def test_null_records_update_statistics_only():
    n = 65
    rews, dones = scripted(n, "random", 2, seed=11)
    old = RecordEpisodeStatisticsTorch(ScriptedEnv(rews, dones), torch.device("cuda"))
    new = EpisodeRecorder(ScriptedEnv(rews, dones), "cuda", env_id0=ENV_ID0)
    old.reset()
    new.reset()
    new.begin_rollout()
    new.count.fill_(17)
    new.records.fill_(-7)
    for _ in range(2):                                         # never armed: records == NULL
        _, _, _, io = old.step(None)
        _, _, _, i_n = new.step(None)
        np.testing.assert_array_equal(bits(i_n["r"]), bits(io["r"]))
        np.testing.assert_array_equal(i_n["l"].cpu().numpy(), io["l"].cpu().numpy())
    np.testing.assert_array_equal(bits(new.episode_returns), bits(old.episode_returns))
    assert int(new.count.cpu()[0]) == 17 and bool((new.records == -7).all())
