"""Every discrete decision of the env step, on both sides of its line, on the host build
(``make(sim_device="cpu")``: the same env_core as the HIP kernels, compiled for the CPU) against the f64 oracle.

tests/decision_cases.py lays one 64-rung ladder per decision of the task across that decision's line (the table in its
docstring), asserts on the oracle alone that both sides are populated, and compares one step: rungs farther than 1e-4
from every line at test_single_step_parity's tolerances, the others against the oracle stepped with its compared
quantities biased by +2e-4 or by -2e-4.  tests/test_gpu_decision_edges.py runs the same cases through every kernel form.
"""
import functools

import numpy as np
import pytest
import torch

import ouzelum_amd
from oracle import quad_oracle as Q
from tests import decision_cases as D

make_cpu = functools.partial(ouzelum_amd.make, sim_device="cpu", rl_device="cpu")


@pytest.mark.parametrize("task", D.TASK_TABLE)
def test_decision_edges_host_build(task):
    n = D.small_n(task)
    env, o = D.warm_pair(make_cpu, task, n)
    plan = D.plan_ladders(o)
    assert [name for name, _ in plan] == [c for t in sorted(D.CASES_OF) if np.any(o.task_ids == t)
                                          for c in D.CASES_OF[t]]
    actions = D.actions_for(n)
    rows = D.lay_ladders(o, plan, actions)
    assert len(np.unique(rows)) == len(rows) == D.RUNGS * len(plan) + D.TAIL
    D.load_env(env, o)
    env.step(torch.as_tensor(actions))
    near = D.check_step(f"{task} host step", D.env_snapshot(env), o, rows, actions, plan)
    assert near <= 2 * len(plan) + 4, f"{near} rungs within {D.DELTA} of a line: the ladders are not where they were put"


def test_one_step_rollout_with_storage_on_the_host_build():
    """The host build's rollout(storage=...) path on the same cases: its storage row is the step's output."""
    task = "QuadTracking"
    n = D.small_n(task)
    env, o = D.warm_pair(make_cpu, task, n)
    plan = D.plan_ladders(o)
    actions = D.actions_for(n)
    rows = D.lay_ladders(o, plan, actions)
    D.load_env(env, o)
    st = (torch.full((1, n, 13), -7.0), torch.full((1, n), -7.0), torch.full((1, n), -7, dtype=torch.int64),
          torch.ones((1, n), dtype=torch.bool))
    env.rollout(torch.as_tensor(actions)[None], 1, fused=True, storage=st)
    D.check_step(f"{task} host rollout", D.env_snapshot(env), o, rows, actions, plan)
    D.check_step(f"{task} host rollout storage", D.env_snapshot(env, st), o, rows, actions, plan,
                 fields=("obs", "rew", "reset", "timeouts"))


def test_every_table_row_has_a_case():
    """Each decision of the table is laid for every task that takes it (decision_cases.CASES_OF)."""
    have = {t: set(c) for t, c in D.CASES_OF.items()}
    done = {"die_far", "die_z", "time_out"}
    assert all(done <= c for c in have.values())
    for t in (Q.TASK_LEE_LANDED, Q.TASK_EKF_LEE_LANDED, Q.TASK_TRACKING, Q.TASK_LANDING):   # the tasks with a deck
        assert {"deck_z", "deck_r"} <= have[t]
    assert "hover" in have[Q.TASK_LEE_LANDED]
    for t in (Q.TASK_EKF_LEE_LANDED, Q.TASK_TRACKING):
        assert {"land", "reaim_lo", "reaim_hi", "final"} <= have[t]
    for t in (Q.TASK_TRACKING, Q.TASK_LANDING):
        assert {"husky_switch", "husky_band", "husky_wrap", "traj_done"} <= have[t]
    for t in (Q.TASK_OUZELUM, Q.TASK_FAULT):
        assert "goal_redraw" in have[t]
    assert "fault_onset" in have[Q.TASK_FAULT]
    assert set(Q.MIXED_TASKS) <= set(have)
