"""Writes tests/golden/learner_variants.json: the reference's seven learners and its experiment grid as data
(names and numbers only), read as TEXT from a checkout of the reference:

    python tests/golden/make_learner_variants.py /path/to/reference

* ``isaacgymenvs/experiments.sh``: the order of the learner directories (its ``cd`` lines) and, per directory,
  the ``--POMDP`` / ``--pomdp_prob`` pairs of its ``python main.py`` lines;
* ``<dir>/main.py``: the ``SummaryWriter`` and ``agent.save`` format strings (run, best and final checkpoint
  names), the ``getAction(...)`` argument (what the policy acts on), whether ``next_obs = POMDP.observation(...)``
  replaces the observation itself (the single-stream routing: the critic sees the corrupted observation) and
  whether ``agent.train`` is handed ``pomdps``;
* ``<dir>/model.py``: ``rpo_alpha`` and whether the "new to RPO" branch is live or commented out, and whether
  the actor has an LSTM.

Nothing is imported or run from the reference.  The tests compare ``ouzelum_amd/learners/variants.py`` and
``sweep.grid()`` with the file; nothing on a GPU machine reads the reference.
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def fmt(s):
    """'../runs/PPO_{args.POMDP}_{args.pomdp_prob}' -> 'PPO_{P}_{p}'"""
    s = s.rsplit("/", 1)[-1]
    return s.replace("{args.POMDP}", "{P}").replace("{args.pomdp_prob}", "{p}")


def learner(root, d):
    main = open(os.path.join(root, d, "main.py")).read()
    model = open(os.path.join(root, d, "model.py")).read()
    run = fmt(re.search(r"SummaryWriter\(f[\"']([^\"']+)[\"']\)", main).group(1))
    saves = [fmt(x) for x in re.findall(r"^\s*agent\.save\(f[\"']([^\"']+)[\"']\)", main, re.M)]
    assert len(saves) == 2, saves
    best, final = saves            # the save inside the loop (best reward) comes first, the final one after it
    act_arg = re.search(r"agent\.getAction\(\s*(\w+)", main).group(1)
    single = re.search(r"^\s*next_obs\s*=\s*POMDP\.observation\(next_obs\)", main, re.M) is not None
    trains_pomdps = re.search(r"agent\.train\(obs,\s*pomdps", main) is not None
    assert single != trains_pomdps
    alpha = float(re.search(r"self\.rpo_alpha\s*=\s*([0-9.]+)", model).group(1))
    live = re.search(r"^\s*else:\s*# new to RPO", model, re.M) is not None
    dead = re.search(r"^\s*#\s*else:\s*# new to RPO", model, re.M) is not None
    assert live != dead
    return {"recurrent": "nn.LSTM" in model, "rpo_alpha": alpha if live else 0.0,
            "acts_on": "pomdp" if single or act_arg == "pomdp" else "clean",
            "actor_trains_on": "pomdp",
            "critic_on": "pomdp" if single else "clean",
            "run": run, "final": final, "best": best}


def main(ref):
    root = os.path.join(ref, "isaacgymenvs")
    order, grid, cur = [], [], None
    for line in open(os.path.join(root, "experiments.sh")):
        m = re.match(r"\s*cd\s+([\w-]+)\s*$", line)
        if m:
            cur = m.group(1)
            order.append(cur)
            continue
        m = re.match(r"\s*python main\.py --POMDP=(\w+) --pomdp_prob=([0-9.]+)", line)
        if m:
            grid.append([cur, m.group(1), float(m.group(2))])
    out = {"order": order, "learners": {d: learner(root, d) for d in order}, "grid": grid}
    path = os.path.join(HERE, "learner_variants.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(path, len(order), "learners,", len(grid), "runs")


if __name__ == "__main__":
    main(sys.argv[1])
