"""The plain-config form of the output-wave rollouts (OUZ_PLAIN_ROLLOUT, csrc/quad_env.h plain_config) and the
R(q) they carry from a step's integrator to the next step: bitwise the general kernels (OUZ_PLAIN_ROLLOUT=0) and
the one-step kernels, with resets inside a launch, and chosen per launch from that launch's configuration."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

TASKS = ("LeeLanded", "QuadFault", "Ouzelum")   # the tasks whose output-wave rollout has a plain form
Z_DIE = {"LeeLanded": 0.3, "QuadFault": 0.5, "Ouzelum": 0.5}


@pytest.fixture(scope="module")
def ouz():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    import ouzelum_amd
    return ouzelum_amd


def make_pair(ouz, monkeypatch, task, n, off=0, seed=31, **kw):
    """The same env twice: with the plain-config kernels (the default, set explicitly) and with the general ones."""
    kw = dict(seed=seed, task=task, num_envs=n, sim_device="cuda:0", track_episodes=True, env_id_offset=off,
              num_envs_total=off + n + 11, **kw)
    monkeypatch.setenv("OUZ_PLAIN_ROLLOUT", "1")
    a = ouz.make(**kw)
    monkeypatch.setenv("OUZ_PLAIN_ROLLOUT", "0")
    b = ouz.make(**kw)
    monkeypatch.delenv("OUZ_PLAIN_ROLLOUT")
    return a, b


def action_ring(n, seed=7):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.rand((32, n, 4), device="cuda", generator=g) * 2 - 1).contiguous()


def launch(env, ring, k):
    """k fused steps with rollout storage and the fused statistics through rollout_plan (ouz_rollout_stats)."""
    n = env.num_envs
    st = (torch.full((k, n, 13), -7.0, device="cuda"), torch.full((k, n), -7.0, device="cuda"),
          torch.full((k, n), -7, dtype=torch.int64, device="cuda"), torch.ones((k, n), dtype=torch.bool, device="cuda"))
    got = torch.full((3,), -1.0, dtype=torch.float64, device="cuda")
    env.rollout_plan(ring, k, storage=st, drain=True)(got.data_ptr())
    return st, got


def assert_same_state(a, b, tag):
    from ouzelum_amd import _lib as L
    torch.cuda.synchronize()
    assert torch.equal(a.frows(0, L.F_COUNT), b.frows(0, L.F_COUNT)), tag      # p, q, v, w, episode fields, ...
    assert torch.equal(a.irows(0, L.I_COUNT), b.irows(0, L.I_COUNT)), tag      # progress, counters, ...
    for buf in ("obs_buf", "rew_buf", "reset_buf", "timeout_buf"):
        assert torch.equal(getattr(a, buf), getattr(b, buf)), (tag, buf)


def assert_same_launch(a, b, ring, k, tag):
    (sa, ga), (sb, gb) = launch(a, ring, k), launch(b, ring, k)
    torch.cuda.synchronize()
    for name, x, y in zip(("obs", "rew", "reset", "time_outs"), sa, sb):
        assert torch.equal(x, y), (tag, k, name)
    assert torch.equal(ga, gb), (tag, k, "statistics")
    assert_same_state(a, b, (tag, k))
    return sa, ga


def split_timeouts():
    from ouzelum_amd import _lib as L
    cnt = ctypes.c_uint32(0)
    L.check(L.lib.ouz_split_timeouts(ctypes.byref(cnt), 1))
    return cnt.value


@pytest.mark.parametrize("off", [0, 37])
@pytest.mark.parametrize("n", [64, 100, 1344])
@pytest.mark.parametrize("task", TASKS)
def test_plain_is_bitwise_general(ouz, task, n, off, monkeypatch):
    """One full tile, a partial last tile and 21 tiles, at shard offsets 0 and 37 of a larger id space: launches of
    1, 2, 32 and 32 steps with storage and fused statistics; every storage tensor, the statistics, the whole state
    and the env buffers after every launch are those of the general kernels, and no ring wait gave up."""
    split_timeouts()
    a, b = make_pair(ouz, monkeypatch, task, n, off)
    ring = action_ring(n)
    for k in (1, 2, 32, 32):
        assert_same_launch(a, b, ring, k, task)
    assert split_timeouts() == 0


@pytest.mark.parametrize("die", [False, True])
@pytest.mark.parametrize("task", TASKS)
def test_plain_resets_inside_a_launch(ouz, task, die, monkeypatch):
    """max_episode_length = 5: every lane resets several times in a 32-step launch (the carried R(q) is re-formed
    from the reset quaternion, the reset paths of the plain form run).  die: after the first launch every third
    env is put just above the die height, falling, from staggered heights, so lanes of a wave end their episodes
    at different steps (a divergent reset)."""
    from ouzelum_amd import _lib as L
    n = 100
    split_timeouts()
    a, b = make_pair(ouz, monkeypatch, task, n, 0, max_episode_length=5)
    ring = action_ring(n)
    assert_same_launch(a, b, ring, 1, task)
    if die:
        e = torch.arange(n, device="cuda")
        hit = e % 3 == 0
        for env in (a, b):
            pz, vz = env.frows(L.F_P + 2)[0], env.frows(L.F_V + 2)[0]
            env.set_frows(L.F_P + 2, torch.where(hit, Z_DIE[task] + 0.004 * (e % 16).float(), pz))
            env.set_frows(L.F_V + 2, torch.where(hit, torch.full_like(vz, -1.5), vz))
    st, _ = assert_same_launch(a, b, ring, 2, task)
    first = st[2]
    st, got = assert_same_launch(a, b, ring, 32, task)
    if die:   # the staggered envs ended at more than one step before the episode length ends everyone
        done = torch.cat([first, st[2][:2]])[:, hit] != 0
        assert done.any(0).all(), "an env put at the die height did not end its episode"
        assert len(set(done.int().argmax(0).tolist())) >= 2, "the overwritten envs all ended at the same step"
    assert float(got[1]) >= 4 * n, "fewer than four finished episodes per env in 32 steps"
    assert_same_launch(a, b, ring, 32, task)
    assert split_timeouts() == 0


MASS_DR = {"actor_params": {"Drone": {"rigid_body_properties": {"mass": {
    "range": [0.7, 1.3], "operation": "scaling", "distribution": "uniform"}}}}}
OBS_NOISE = {"observations": {"range": [0.0, 0.02], "operation": "additive", "distribution": "gaussian"}}
GRAVITY_DR = {"sim_params": {"gravity": {"range": [0.8, 1.2], "operation": "scaling", "distribution": "uniform"}}}
FEATURES = {
    "physical_dr": (lambda e: e.apply_randomizations(MASS_DR), lambda e: e.apply_randomizations({"actor_params": {}})),
    "obs_noise": (lambda e: e.apply_randomizations(OBS_NOISE), lambda e: e.apply_randomizations({})),
    "gravity_dr": (lambda e: e.apply_randomizations(GRAVITY_DR), lambda e: e.apply_randomizations({"sim_params": {}})),
    "trace": (lambda e: e.enable_trace(3, 64), lambda e: e.enable_trace(capacity=0)),
}


@pytest.mark.parametrize("feature", sorted(FEATURES))
def test_plain_predicate_is_per_launch(ouz, feature, monkeypatch):
    """An option the plain form leaves out, switched on after creation and after a plain launch: the next launch
    must run the general kernel (a plain kernel that ignored the option would differ from the OUZ_PLAIN_ROLLOUT=0
    env, and the option must have changed the results at all); switched off again, the results still agree."""
    n = 100
    a, b = make_pair(ouz, monkeypatch, "LeeLanded", n, 0, max_episode_length=5)
    c = make_pair(ouz, monkeypatch, "LeeLanded", n, 0, max_episode_length=5)[0]   # never gets the option
    on, off = FEATURES[feature]
    assert_same_launch(a, b, None, 32, feature)
    launch(c, None, 32)
    for env in (a, b):
        on(env)
    st, _ = assert_same_launch(a, b, None, 32, (feature, "on"))
    sc, _ = launch(c, None, 32)
    torch.cuda.synchronize()
    if feature == "trace":
        for x, y in zip(a._trace[:2], b._trace[:2]):
            assert torch.equal(x, y), "trace"
        assert float(a._trace[0].abs().sum()) > 0 and int(a._trace[1].sum()) > 0, "the trace was not written"
    else:
        assert not torch.equal(st[0], sc[0]), "the option did not change the observations: the test shows nothing"
    for env in (a, b):
        off(env)
    assert_same_launch(a, b, None, 32, (feature, "off"))


def test_plain_predicate_substeps(ouz, monkeypatch):
    """substeps = 3 (a creation-time setting: there is no setter) is outside the plain form, which has the two
    sub-steps unrolled: both toggles must run the generic integrator."""
    a, b = make_pair(ouz, monkeypatch, "LeeLanded", 100, 0, max_episode_length=5, substeps=3)
    c = make_pair(ouz, monkeypatch, "LeeLanded", 100, 0, max_episode_length=5)[0]
    for k in (2, 32):
        st, _ = assert_same_launch(a, b, None, k, "substeps")
        sc, _ = launch(c, None, k)
    torch.cuda.synchronize()
    assert not torch.equal(st[0], sc[0]), "three sub-steps gave the observations of two"


@pytest.mark.parametrize("plain", ["1", "0"])
@pytest.mark.parametrize("task", TASKS)
def test_carried_rotation_matches_one_step_path(ouz, task, plain, monkeypatch):
    """Seven steps in one fused launch (R(q) carried from step to step) against seven VecTask.step calls (R(q)
    formed from the stored quaternion in every step), from the initial reset of every env: bitwise."""
    n, k = 100, 7
    kw = dict(seed=41, task=task, num_envs=n, sim_device="cuda:0", track_episodes=True)
    monkeypatch.setenv("OUZ_PLAIN_ROLLOUT", plain)
    a, b = ouz.make(**kw), ouz.make(**kw)
    monkeypatch.delenv("OUZ_PLAIN_ROLLOUT")
    ring = action_ring(n)
    for rep in range(2):   # the second round starts from a flown state instead of the reset pose
        a.rollout(ring, k, fused=True)
        for j in range(k):
            b.step(ring[j])
        assert_same_state(a, b, (task, plain, rep))
