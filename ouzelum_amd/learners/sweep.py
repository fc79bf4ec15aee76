"""The reference's experiment (``isaacgymenvs/experiments.sh``): seven learners x 16 POMDP settings, 112 runs.

    python -m ouzelum_amd.learners.sweep --learners all --grid reference [--total_steps N] [--dry_run]
    python -m ouzelum_amd.learners.sweep --learners PPO,RPO-LSTM --dry_run

Runs ``python -m ouzelum_amd.learners.train --learner L --POMDP P --pomdp_prob p`` once per (L, P, p), in the
script's order (learner by learner; flicker, random_noise, flickering_and_random_noise), one after another, each a
fresh child process, and stops at the first run that exits non-zero.  ``--dry_run`` prints the command lines and
starts nothing.  Arguments this module does not know (``--env``, ``--num_envs``, ``--logdir``, ``--episode_log``,
``--gemm_dtype``, the update's flags such as ``--ent_coef 0.01 --clip_vloss --anneal_lr --run_tag tuned``,
``--value_bootstrap``, ``--max_episode_length N`` ...) are handed to every run, and only when given.
"""
import argparse
import shlex
import subprocess
import sys

from .variants import GRID, LEARNERS


def grid(learners=LEARNERS):
    """[(learner, POMDP, prob)] in experiments.sh order."""
    return [(ln, mode, p) for ln in learners for mode, probs in GRID for p in probs]


def command(learner, pomdp, prob, total_steps=None, extra=()):
    cmd = [sys.executable, "-m", "ouzelum_amd.learners.train", "--learner", learner, "--POMDP", pomdp,
           "--pomdp_prob", str(prob)]
    if total_steps is not None:
        cmd += ["--total_steps", str(total_steps)]
    return cmd + list(extra)


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    p.add_argument("--learners", default="all", help="'all' or a comma-separated list of: " + ", ".join(LEARNERS))
    p.add_argument("--grid", default="reference", choices=["reference"])
    p.add_argument("--total_steps", type=int, default=None, help="per run (default: train.py's)")
    p.add_argument("--dry_run", action="store_true")
    args, extra = p.parse_known_args(argv)
    if args.learners == "all":
        args.learners = list(LEARNERS)
    else:
        args.learners = [x for x in args.learners.split(",") if x]
        unknown = [x for x in args.learners if x not in LEARNERS]
        if unknown or not args.learners:
            p.error(f"unknown learner(s) {unknown}; choose from {', '.join(LEARNERS)}")
    args.extra = extra
    return args


def main(argv=None, run=subprocess.run):
    args = parse_args(argv)
    for learner, pomdp, prob in grid(args.learners):
        cmd = command(learner, pomdp, prob, args.total_steps, args.extra)
        if args.dry_run:
            print(" ".join(shlex.quote(c) for c in cmd))
            continue
        print("== " + " ".join(shlex.quote(c) for c in cmd), flush=True)
        rc = run(cmd).returncode
        if rc != 0:
            print(f"{learner} {pomdp} {prob} exited {rc}: stopping", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
