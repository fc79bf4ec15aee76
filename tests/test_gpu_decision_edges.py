"""Every discrete decision of the env step, on both sides of its line, through every form the step is compiled in.

tests/decision_cases.py lays one 64-rung ladder per decision of the task across that decision's line (the table in its
docstring; the host build runs the same cases in tests/test_decision_edges_cpu.py).  Here each kernel form steps that
state once and is compared with the f64 oracle: rungs farther than 1e-4 from every line at test_single_step_parity's
tolerances, the others against the oracle stepped with its compared quantities biased by +2e-4 or by -2e-4.

Forms: below 65 536 envs the class-layout step kernel, the quad-lane estimator (OUZ_QUAD_LANE=1, step
and fused rollout), the fused rollout with the split-wave estimator and the output wave on and off (OUZ_SPLIT_PV x
OUZ_OUT_WAVE); above, the 256-lane step kernels of every task family (the mixed curriculum as one launch per task),
the two-waves-per-env fused estimator rollout, the pipelined (OUZ_PIPE_TILES=2) and non-temporal-load (OUZ_NT_LOADS=1)
step kernels and the streamed rollout (OUZ_ROLLOUT_STREAM=1).  A fused rollout's storage row is compared as well as
the state it leaves.  n = 64 L + 37 (L ladders; the 37-lane tail repeats the first rungs of a ladder, so the partial
last wave carries live decisions); above 65 536 envs every other ladder lies in the last tiles of its task.
"""
import functools

import numpy as np
import pytest
import torch

from tests import decision_cases as D
from tests.test_gpu_timed_kernels import storage_for

pytestmark = pytest.mark.gpu

ESTIMATOR = ("EKFLeeLanded", "QuadTracking", "QuadMixed")
LARGE_N = 70016 + 37


@pytest.fixture(scope="module")
def ouz():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    import ouzelum_amd
    return ouzelum_amd


def run_case(ouz, monkeypatch, task, form, toggles, n=None, **kw):
    """One env creation (toggles set before it: ouz_create reads them), one launch, one oracle step of the ladder envs."""
    for k, v in toggles.items():
        monkeypatch.setenv(k, v)
    large = n is not None
    n = n or D.small_n(task)
    make = functools.partial(ouz.make, sim_device="cuda:0", rl_device="cuda:0")
    env, o = D.warm_pair(make, task, n, **kw)
    plan = D.plan_ladders(o, spread=large)
    actions = D.actions_for(n)
    rows = D.lay_ladders(o, plan, actions)
    D.load_env(env, o)
    tag = f"{task} {n} envs {form} {toggles}"
    a = torch.as_tensor(actions, device="cuda")
    if form == "step":
        env.step(a)
        D.check_step(tag, D.env_snapshot(env), o, rows, actions, plan)
    else:
        st = storage_for(1, n)
        env.rollout(a[None].contiguous(), 1, fused=True, storage=st, check=True)
        D.check_step(tag, D.env_snapshot(env), o, rows, actions, plan)
        D.check_step(tag + " storage", D.env_snapshot(env, st), o, rows, actions, plan,
                     fields=("obs", "rew", "reset", "timeouts"))
    env.check_health()


def _toggles(**kw):
    return {k: str(v) for k, v in kw.items()}


SMALL = [(t, "step", {}) for t in D.TASK_TABLE]
for _t in D.TASK_TABLE:
    if _t in ESTIMATOR:
        SMALL += [(_t, "step", _toggles(OUZ_QUAD_LANE=1)), (_t, "rollout", _toggles(OUZ_QUAD_LANE=1)),
                  (_t, "rollout", {}), (_t, "rollout", _toggles(OUZ_SPLIT_PV=0, OUZ_OUT_WAVE=1)),
                  (_t, "rollout", _toggles(OUZ_SPLIT_PV=1, OUZ_OUT_WAVE=0)),
                  (_t, "rollout", _toggles(OUZ_SPLIT_PV=0, OUZ_OUT_WAVE=0))]
    else:
        SMALL += [(_t, "rollout", {}), (_t, "rollout", _toggles(OUZ_OUT_WAVE=0))]


def _id(v):
    return ",".join(f"{k[4:]}={x}" for k, x in v.items()) or "default" if isinstance(v, dict) else str(v)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("task,form,toggles", SMALL, ids=_id)
def test_decision_edges_latency_regime(ouz, monkeypatch, task, form, toggles):
    run_case(ouz, monkeypatch, task, form, toggles)


LARGE = ([(t, "step", {}) for t in ("LeeLanded", "QuadFault", "Ouzelum", "QuadTracking", "QuadMixed")]
         + [(t, "rollout", {}) for t in ("QuadTracking", "QuadMixed")]
         + [(t, "step", _toggles(OUZ_PIPE_TILES=2)) for t in ("Ouzelum", "QuadFault")]
         + [(t, "step", _toggles(OUZ_NT_LOADS=1)) for t in ("LeeLanded", "QuadTracking")]
         + [(t, "rollout", _toggles(OUZ_ROLLOUT_STREAM=1)) for t in ("LeeLanded", "QuadFault")])


@pytest.mark.timeout(300)
@pytest.mark.parametrize("task,form,toggles", LARGE, ids=_id)
def test_decision_edges_large_n(ouz, monkeypatch, task, form, toggles):
    """Above 65 536 envs.  The oracle steps the ladder envs only (OracleEnv.take); the GPU steps all of them."""
    kw = {"env_id_offset": 64 * 5, "num_envs_total": 64 * 5 + LARGE_N + 4096} if task == "QuadMixed" else {}
    run_case(ouz, monkeypatch, task, form, toggles, n=LARGE_N, **kw)
