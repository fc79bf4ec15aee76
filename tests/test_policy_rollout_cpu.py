"""ouz_policy_rollout without a device: the ctypes mirrors of its two structs against the header (sizes and every
field's offset, from a C program compiled against include/ouzelum.h), the argument checks that run before any launch,
the host build's refusal and the ``--fused_rollout`` flag's refusals."""
import ctypes
import os
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    from ouzelum_amd import _lib
    return _lib


def test_struct_mirrors_match_the_header(L, tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("g++")
    assert cc, "a C compiler (the host build needs one too)"
    structs = {"ouz_policy_mlp": L.OuzPolicyMlp, "ouz_policy_rollout_io": L.OuzPolicyRolloutIo}
    lines = []
    for cname, cls in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for f, _ in cls._fields_:
            lines.append(f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));')
    src = tmp_path / "offsets.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ouzelum.h"\nint main(void) {\n'
                   + "\n".join(lines) + "\nreturn 0; }\n")
    exe = tmp_path / "offsets"
    subprocess.run([cc, "-x", "c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True,
                                                       check=True).stdout.splitlines())
    for cname, cls in structs.items():
        assert int(got[cname]) == ctypes.sizeof(cls), cname
        for f, _ in cls._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(cls, f).offset, (cname, f)
    assert ctypes.sizeof(L.OuzPolicyMlp) == 80 and ctypes.sizeof(L.OuzPolicyRolloutIo) == 136   # the static_asserts


def test_header_lists_the_entry_and_the_rng_stream(L):
    assert "ouz_policy_rollout" in L.SIGNATURES
    src = open(os.path.join(ROOT, "ouzelum_amd", "csrc", "philox.h")).read()
    assert f"RNG_POLICY = {L.RNG_POLICY}," in src
    from tests import policy_rollout_refs as PR
    assert PR.RNG_POLICY == L.RNG_POLICY


def good(n=8, K=3):
    from tests import policy_rollout_refs as PR
    W = tuple(torch.from_numpy(w) for w in PR.weights())
    return dict(n=n, n_steps=K, weights=W, act_in0=torch.zeros(n, 13),
                storage=(torch.zeros(K, n, 13), torch.zeros(K, n), torch.zeros(K, n, dtype=torch.int64),
                         torch.zeros(K, n, dtype=torch.bool)),
                actions=torch.zeros(K, n, 4), logprobs=torch.zeros(K, n))


def test_argument_checks_need_no_device(L):
    from ouzelum_amd.vec_task import check_policy_rollout_args as chk
    chk(**good())
    chk(**good(), pomdp=torch.zeros(3, 8, 13), pomdp_mode=L.POMDP_NOISE, eps_out=torch.zeros(3, 8, 4),
        norm=(torch.zeros(13), torch.ones(13), 5.0))
    # rows 1.. of a (K + 1)-row store (4-byte aligned 13-wide rows) are accepted
    a = good(n=5)
    a["storage"] = (torch.zeros(4, 5, 13)[1:], *a["storage"][1:])
    chk(**a)
    with pytest.raises(ValueError, match="n_steps"):
        chk(**{**good(), "n_steps": 0})
    with pytest.raises(ValueError, match="float32"):
        chk(**{**good(), "act_in0": torch.zeros(8, 13, dtype=torch.float64)})
    with pytest.raises(ValueError, match="int64"):
        a = good()
        chk(**{**a, "storage": (a["storage"][0], a["storage"][1], a["storage"][2].int(), a["storage"][3])})
    with pytest.raises(ValueError, match="shape"):
        chk(**{**good(), "actions": torch.zeros(3, 8, 3)})
    with pytest.raises(ValueError, match="shape"):
        a = good()
        chk(**{**a, "weights": (a["weights"][0].t().contiguous(), *a["weights"][1:])})
    with pytest.raises(ValueError, match="contiguous"):
        chk(**{**good(), "actions": torch.zeros(3, 4, 8).transpose(1, 2)})
    with pytest.raises(ValueError, match="16-byte aligned"):
        chk(**{**good(), "actions": torch.zeros(3 * 8 * 4 + 1)[1:].view(3, 8, 4)})
    with pytest.raises(ValueError, match="needs eps_in"):
        chk(**good(), sample_mode=L.SAMPLE_GIVEN)
    with pytest.raises(ValueError, match="needs the pomdp tensor"):
        chk(**good(), pomdp_mode=L.POMDP_FLICKER)
    with pytest.raises(ValueError, match="clip"):
        chk(**good(), norm=(torch.zeros(13), torch.ones(13), 0.0))
    with pytest.raises(TypeError, match="torch tensor"):
        chk(**{**good(), "logprobs": None})
    with pytest.raises(L.OuzelumError, match="no CPU fallback"):
        chk(**good(), device=torch.device("cuda", 0))


def test_c_entry_refuses_without_an_env(L):
    assert L.lib.ouz_policy_rollout(None, L.OuzPolicyMlp(), L.OuzPolicyRolloutIo(), 4, None, 0, None) == -3
    assert b"not bound" in L.lib.ouz_last_error()


def test_host_build_raises_not_implemented():
    import ouzelum_amd
    env = ouzelum_amd.make(seed=0, task="Ouzelum", num_envs=8, sim_device="cpu")
    a = good()
    with pytest.raises(NotImplementedError, match="HIP path"):
        env.policy_rollout_plan(a["weights"], 3, a["act_in0"], a["storage"], a["actions"], a["logprobs"])
    with pytest.raises(NotImplementedError):
        env.policy_rollout(a["weights"], 3, a["act_in0"], a["storage"], a["actions"], a["logprobs"])
    assert env.sim_step_count == 0


@pytest.mark.parametrize("learner", ["PPO-LSTM", "RPO-LSTM", "RPO-LSTM_Critic"])
def test_flag_refuses_the_lstm_learners(learner, capsys):
    from ouzelum_amd.learners.train import parse_args
    with pytest.raises(SystemExit):
        parse_args(["--learner", learner, "--env", "Landing", "--fused_rollout"])
    assert "not the LSTM learners" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        parse_args(["--env", "Landing", "--fused_rollout"])   # --algo's default is rpo_lstm


@pytest.mark.parametrize("task", ["LeeLanded", "EKFLeeLanded", "QuadTracking", "QuadMixed"])
def test_flag_refuses_the_tasks_without_a_policy_action(task, capsys):
    from ouzelum_amd.learners.train import parse_args
    with pytest.raises(SystemExit):
        parse_args(["--learner", "PPO", "--env", task, "--fused_rollout"])
    assert "needs a task whose step takes the policy's action" in capsys.readouterr().err


def test_flag_accepted_for_the_mlp_learners():
    from ouzelum_amd.learners.train import fused_rollout_refusal, parse_args
    from ouzelum_amd.learners.variants import VARIANTS
    for learner in ("PPO", "RPO", "PPO_Critic", "RPO_Critic"):
        for task in ("Ouzelum", "QuadFault", "Landing"):
            assert parse_args(["--learner", learner, "--env", task, "--fused_rollout"]).fused_rollout
            assert fused_rollout_refusal(VARIANTS[learner], task) is None
    assert parse_args(["--algo", "ppo", "--env", "QuadFault", "--fused_rollout", "--play"]).fused_rollout
    assert not parse_args(["--learner", "PPO"]).fused_rollout   # off by default
