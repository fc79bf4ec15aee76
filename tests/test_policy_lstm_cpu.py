"""ouz_policy_rollout_lstm without a device: the f64 restatement of the recurrent actor against
``LSTMActor`` in torch f64, the ctypes mirrors of the two new structs against the header, the argument checks that run
before any launch, the host build's refusal and what ``--fused_lstm_rollout`` accepts and refuses."""
import ctypes
import os
import shutil
import subprocess
import types

import numpy as np
import pytest
import torch

from tests import policy_lstm_refs as PL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LSTM_LEARNERS = ("PPO-LSTM", "RPO-LSTM", "RPO-LSTM_Critic")
MLP_LEARNERS = ("PPO", "RPO", "PPO_Critic", "RPO_Critic")


@pytest.fixture(scope="module")
def L():
    from ouzelum_amd import _lib
    return _lib


@pytest.mark.parametrize("normed", [False, True])
def test_f64_restatement_is_the_torch_actor(normed):
    """``actor64`` against ``LSTMActor.forward`` in f64 on the CPU, stepped one call per step with the carry handed
    on (as ``Rollout.collect`` does) and in one call over all steps: dones at step 0, mid-sequence and at the last
    step, a nonzero initial carry."""
    from ouzelum_amd.learners.models import LSTMActor
    from tests import policy_rollout_refs as PR
    K, B = 5, 7
    g = np.random.default_rng(1)
    x = g.standard_normal((K, B, 13))
    eps = g.standard_normal((K, B, 4))
    h0, c0 = g.standard_normal((B, PL.H)) * 0.5, g.standard_normal((B, PL.H)) * 0.5
    done = np.zeros((K, B))
    done[0, 1] = done[2, 3] = done[2, 1] = done[K - 1, 5] = 1.0
    W = PL.weights()
    norm = PR.norm_consts() if normed else None
    ref = PL.actor64(W, x, done, h0, c0, eps, norm)
    space = types.SimpleNamespace(shape=(13,))
    actor = PL.load_actor(LSTMActor(space, types.SimpleNamespace(shape=(4,))).double(), W)
    tx = torch.from_numpy(x)
    if normed:   # the forward normalisation in torch ops (RunningNorm's arithmetic)
        m, r, clip = (torch.as_tensor(np.asarray(v, np.float64)) for v in norm)
        tx = torch.clamp((tx - m) * r, -float(clip), float(clip))
    state = (torch.from_numpy(h0)[None], torch.from_numpy(c0)[None])
    with torch.no_grad():
        a_all, lp_all, _, st_all = actor(tx.reshape(K * B, 13), state, torch.from_numpy(done).reshape(K * B),
                                         eps=torch.from_numpy(eps).reshape(K * B, 4))
        acts, lps = [], []
        for k in range(K):
            a, lp, _, state = actor(tx[k], state, torch.from_numpy(done[k]), eps=torch.from_numpy(eps[k]))
            acts.append(a)
            lps.append(lp)
    tol = 1e-12
    assert np.abs(a_all.numpy().reshape(K, B, 4) - ref["action"]).max() < tol
    assert np.abs(lp_all.numpy().reshape(K, B) - ref["logprob"]).max() < tol
    assert np.abs(torch.stack(acts).numpy() - ref["action"]).max() < tol
    assert np.abs(torch.stack(lps).numpy() - ref["logprob"]).max() < tol
    for got in (st_all, state):
        assert np.abs(got[0][0].numpy() - ref["h_T"]).max() < tol and np.abs(got[1][0].numpy() - ref["c_T"]).max() < tol
    # the done of the last step's input was applied before that step, not to the carry handed out
    assert np.abs(ref["h_T"][5]).max() > 0


def test_struct_mirrors_match_the_header(L, tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("g++")
    assert cc, "a C compiler (the host build needs one too)"
    structs = {"ouz_policy_lstm": L.OuzPolicyLstm, "ouz_policy_lstm_carry": L.OuzPolicyLstmCarry}
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
    assert ctypes.sizeof(L.OuzPolicyLstm) == 112 and ctypes.sizeof(L.OuzPolicyLstmCarry) == 40   # the static_asserts
    assert [f for f, _ in L.OuzPolicyLstm._fields_][:11] == list(PL.NAMES)


def test_the_entry_is_declared_and_the_abi_version_stays(L):
    assert "ouz_policy_rollout_lstm" in L.SIGNATURES
    assert L.ABI_VERSION == 9 == L.lib.ouz_abi_version()
    hdr = open(os.path.join(ROOT, "include", "ouzelum.h")).read()
    assert "int ouz_policy_rollout_lstm(" in hdr


def test_c_entry_refuses_without_an_env(L):
    rc = L.lib.ouz_policy_rollout_lstm(None, L.OuzPolicyLstm(), L.OuzPolicyLstmCarry(), L.OuzPolicyRolloutIo(), 4,
                                       None, 0, None)
    assert rc == -3
    assert b"not bound" in L.lib.ouz_last_error()


def good(n=8):
    W = tuple(torch.from_numpy(w) for w in PL.weights())
    z = lambda *s: torch.zeros(*s)   # noqa: E731
    return dict(n=n, weights=W, carry=(z(n, PL.H), z(n, PL.H), z(n), z(n, PL.H), z(n, PL.H)))


def test_argument_checks_need_no_device(L):
    from ouzelum_amd.vec_task import check_lstm_policy_rollout_args as chk
    chk(**good())
    a = good()
    with pytest.raises(ValueError, match="weights must be"):
        chk(**{**a, "weights": a["weights"][:7]})
    with pytest.raises(ValueError, match="shape"):
        chk(**{**a, "weights": (a["weights"][0][:256].contiguous(), *a["weights"][1:])})
    with pytest.raises(ValueError, match="float32"):
        chk(**{**a, "weights": (*a["weights"][:4], a["weights"][4].double(), *a["weights"][5:])})
    h, c, d, ho, co = a["carry"]
    with pytest.raises(ValueError, match="carry must be"):
        chk(**{**a, "carry": (h, c, d, ho)})
    with pytest.raises(ValueError, match="distinct"):
        chk(**{**a, "carry": (h, c, d, h, co)})
    with pytest.raises(ValueError, match="distinct"):
        chk(**{**a, "carry": (h, c, d, ho, c)})
    with pytest.raises(ValueError, match="shape"):
        chk(**{**a, "carry": (h, c, torch.zeros(8, 1), ho, co)})
    with pytest.raises(ValueError, match="16-byte aligned"):
        chk(**{**a, "carry": (torch.zeros(8 * PL.H + 1)[1:].view(8, PL.H), c, d, ho, co)})
    with pytest.raises(TypeError, match="torch tensor"):
        chk(**{**a, "carry": (h, c, None, ho, co)})
    with pytest.raises(L.OuzelumError, match="no CPU fallback"):
        chk(**a, device=torch.device("cuda", 0))


def test_host_build_raises_not_implemented():
    import ouzelum_amd
    env = ouzelum_amd.make(seed=0, task="Ouzelum", num_envs=8, sim_device="cpu")
    a, K = good(), 3
    io = (K, torch.zeros(8, 13), (torch.zeros(K, 8, 13), torch.zeros(K, 8), torch.zeros(K, 8, dtype=torch.int64),
                                  torch.zeros(K, 8, dtype=torch.bool)), torch.zeros(K, 8, 4), torch.zeros(K, 8))
    with pytest.raises(NotImplementedError, match="HIP path"):
        env.lstm_policy_rollout_plan(a["weights"], a["carry"], *io)
    with pytest.raises(NotImplementedError, match="HIP path"):
        env.lstm_policy_rollout(a["weights"], a["carry"], *io)
    assert env.sim_step_count == 0


@pytest.mark.parametrize("learner", MLP_LEARNERS)
def test_flag_refuses_the_mlp_learners(learner, capsys):
    from ouzelum_amd.learners.train import parse_args
    with pytest.raises(SystemExit):
        parse_args(["--learner", learner, "--env", "Landing", "--fused_lstm_rollout"])
    assert "not the MLP learners" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        parse_args(["--algo", "ppo", "--env", "Landing", "--fused_lstm_rollout"])


@pytest.mark.parametrize("task", ["LeeLanded", "EKFLeeLanded", "QuadTracking", "QuadMixed"])
def test_flag_refuses_the_tasks_without_a_policy_action(task, capsys):
    from ouzelum_amd.learners.train import parse_args
    with pytest.raises(SystemExit):
        parse_args(["--learner", "RPO-LSTM", "--env", task, "--fused_lstm_rollout"])
    assert "needs a task whose step takes the policy's action" in capsys.readouterr().err


def test_flag_accepted_for_the_lstm_learners_and_off_by_default():
    from ouzelum_amd.learners.train import fused_lstm_rollout_refusal, fused_rollout_refusal, parse_args
    from ouzelum_amd.learners.variants import VARIANTS
    for learner in LSTM_LEARNERS:
        for task in ("Ouzelum", "QuadFault", "Landing"):
            args = parse_args(["--learner", learner, "--env", task, "--fused_lstm_rollout"])
            assert args.fused_lstm_rollout and not args.fused_rollout
            assert fused_lstm_rollout_refusal(VARIANTS[learner], task) is None
            assert "not the LSTM learners" in fused_rollout_refusal(VARIANTS[learner], task)   # unchanged
    assert parse_args(["--env", "QuadFault", "--fused_lstm_rollout"]).fused_lstm_rollout   # --algo rpo_lstm, the default
    assert parse_args(["--algo", "rpo_lstm", "--env", "Landing", "--fused_lstm_rollout", "--play"]).fused_lstm_rollout
    assert not parse_args(["--learner", "RPO-LSTM"]).fused_lstm_rollout
    assert not parse_args([]).fused_lstm_rollout and not parse_args([]).fused_rollout
