"""``PPOLearner(normalize_input, normalize_value)`` without a GPU: construction, the checkpoint's fifth file, the
command-line flags, and the data-parallel merge over two gloo ranks."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import norm_refs as NR


def spaces():
    from ouzelum_amd.spaces import Box
    return Box(-np.inf * np.ones(13), np.inf * np.ones(13)), Box(-np.ones(4), np.ones(4))


def learner(**kw):
    from ouzelum_amd.learners import PPOLearner
    return PPOLearner(*spaces(), 8, "cpu", recurrent=False, rollout_steps=4, tuned_gemms=False, **kw)


def test_flags_off_is_the_parent_learner():
    ag = learner()
    assert ag.normalize_input is False and ag.normalize_value is False
    assert ag.actor_norm is None and ag.critic_norm is None and ag.value_norm is None
    assert ag.actor.obs_norm is None and ag.critic.obs_norm is None


def test_flags_attach_one_normaliser_per_network():
    ag = learner(normalize_input=True, normalize_value=True)
    assert ag.actor.obs_norm is ag.actor_norm and ag.critic.obs_norm is ag.critic_norm
    assert ag.actor_norm is not ag.critic_norm
    assert (ag.actor_norm.d, ag.actor_norm.clip) == (13, 5.0) == (ag.critic_norm.d, ag.critic_norm.clip)
    assert (ag.value_norm.d, ag.value_norm.clip) == (1, float("inf"))
    only_v = learner(normalize_value=True)
    assert only_v.actor.obs_norm is None and only_v.value_norm is not None
    # the networks read raw observations through the normalisers; inside the update's scope they do not
    x = torch.tensor(NR.moments_case(65, 13, "offset")[0])
    ag.critic_norm.update(x)
    with torch.no_grad():
        want = ag.critic.critic(ag.critic_norm.normalize(x))
        assert torch.equal(ag.critic(x), want)
        with ag._inputs_prenormalized():
            assert ag.critic.obs_norm is None and torch.equal(ag.critic(x), ag.critic.critic(x))
        assert ag.critic.obs_norm is ag.critic_norm
        # normalize_value: the critic's output is in normalised units
        ag.value_norm.update(torch.tensor(NR.moments_case(65, 1, "cancel")[0]))
        v = ag.critic(x).reshape(-1)
        assert torch.equal(ag._raw_values(v), ag.value_norm.denormalize(v.reshape(-1, 1)).reshape(-1))
        assert float(ag._raw_values(v).mean()) > 100.0


def test_checkpoint_files(tmp_path):
    """Exactly the parent's four files with both flags off; a fifth when a flag is on, which load requires then."""
    four = {"ck_actor", "ck_actor_optimizer", "ck_critic", "ck_critic_optimizer"}
    plain = learner()
    plain.save(str(tmp_path / "ck"))
    assert set(os.listdir(tmp_path)) == four
    plain.load(str(tmp_path / "ck"))
    for kw in ({"normalize_input": True}, {"normalize_value": True}, {"normalize_input": True, "normalize_value": True}):
        with pytest.raises(FileNotFoundError):
            learner(**kw).load(str(tmp_path / "ck"))       # the four files alone do not do
    x = torch.tensor(NR.moments_case(1000, 13, "offset")[0])
    ag = learner(normalize_input=True, normalize_value=True)
    ag.actor_norm.update(x[:400])
    ag.critic_norm.update(x)
    ag.value_norm.update(x[:, :1].contiguous())
    d = tmp_path / "norm"
    d.mkdir()
    ag.save(str(d / "ck"))
    assert set(os.listdir(d)) == four | {"ck_normalizers"}
    saved = torch.load(d / "ck_normalizers", weights_only=True)
    assert set(saved) == {"actor_input", "critic_input", "value"}
    assert all(t.dtype == torch.float64 for s in saved.values() for t in s.values())
    other = learner(normalize_input=True, normalize_value=True)
    other.load(str(d / "ck"))
    for a, b in ((ag.actor_norm, other.actor_norm), (ag.critic_norm, other.critic_norm),
                 (ag.value_norm, other.value_norm)):
        assert torch.equal(a.state, b.state) and torch.equal(a.m, b.m) and torch.equal(a.r, b.r)
    assert other.actor.obs_norm is other.actor_norm and not torch.equal(other.actor_norm.state, other.critic_norm.state)
    # a learner that normalises less reads what it needs; one that needs statistics the file lacks is refused
    learner(normalize_value=True).load(str(d / "ck"))
    learner().load(str(d / "ck"))
    only_v = tmp_path / "only_v"
    only_v.mkdir()
    learner(normalize_value=True).save(str(only_v / "ck"))
    with pytest.raises(KeyError):
        learner(normalize_input=True).load(str(only_v / "ck"))


def test_flags_reach_the_learner_from_the_parser():
    from ouzelum_amd.learners import train as TR
    from ouzelum_amd.learners.variants import VARIANTS
    v = VARIANTS["RPO-LSTM"]
    off = TR.parse_args(["--learner", "RPO-LSTM"])
    assert off.normalize_input is False and off.normalize_value is False
    assert "normalize_input" not in TR.learner_kwargs(off, v) and TR.normalization_kwargs(off) == {}
    on = TR.parse_args(["--learner", "RPO-LSTM", "--normalize_input", "--normalize_value"])
    kw = TR.learner_kwargs(on, v)
    assert kw["normalize_input"] is True and kw["normalize_value"] is True
    ag = learner(**{k: kw[k] for k in ("normalize_input", "normalize_value", "lr", "clip_coef")})
    assert ag.normalize_input and ag.normalize_value and ag.actor_norm is not None and ag.value_norm is not None
    one = TR.parse_args(["--algo", "ppo", "--normalize_value", "--play"])
    assert TR.normalization_kwargs(one) == {"normalize_value": True}


# ---------------------------------------------------------------------------------------------------------------
# two gloo ranks
# ---------------------------------------------------------------------------------------------------------------
D, ROWS_PER_RANK = 13, 500


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _norm_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    from ouzelum_amd.distributed import init_from_env
    from ouzelum_amd.learners.fused import RunningNorm
    init_from_env(backend="gloo")
    x = NR.moments_case(2 * world * ROWS_PER_RANK, D, "offset")[0]
    norm = RunningNorm(D, "cpu", clip=5.0)
    for u in range(2):      # two updates; rank r holds rows [r, r + 1) * ROWS_PER_RANK of each update's block
        lo = (u * world + rank) * ROWS_PER_RANK
        norm.update(torch.tensor(x[lo:lo + ROWS_PER_RANK]))
    torch.save({"state": norm.state.clone(), "m": norm.m.clone(), "r": norm.r.clone()},
               os.path.join(out_dir, f"n{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_hold_identical_statistics(tmp_path):
    """Every rank all-gathers the batch triples and merges them in rank order: bitwise identical statistics on both
    ranks, within 1e-11 relative of the single-process statistics of the concatenated rows."""
    from ouzelum_amd.learners.fused import RunningNorm
    world = 2
    mp.spawn(_norm_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    got = [torch.load(tmp_path / f"n{r}.pt", weights_only=True) for r in range(world)]
    for k in ("state", "m", "r"):
        assert torch.equal(got[0][k], got[1][k]), k
    x = NR.moments_case(2 * world * ROWS_PER_RANK, D, "offset")[0]
    single = RunningNorm(D, "cpu", clip=5.0)
    for u in range(2):
        single.update(torch.tensor(x[u * world * ROWS_PER_RANK:(u + 1) * world * ROWS_PER_RANK]))
    assert float(got[0]["state"][-1]) == float(single.count) == 1.0 + 2 * world * ROWS_PER_RANK
    assert NR.rel_err(got[0]["state"][:D].numpy(), single.mean.numpy()) <= 1e-11
    assert NR.rel_err(got[0]["state"][D:2 * D].numpy(), single.var.numpy()) <= 1e-11
    # and of the exact moments of all the rows with the prior row
    _, mean, m2 = NR.moments_case(2 * world * ROWS_PER_RANK, D, "offset")
    pm, pv = NR.prior_row_moments(mean, m2, float(x.shape[0]))
    assert NR.rel_err(got[0]["state"][:D].numpy(), pm) <= 1e-11
    assert NR.rel_err(got[0]["state"][D:2 * D].numpy(), pv) <= 1e-11
