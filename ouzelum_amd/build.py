"""Build ``libouzelum_hip.so`` in-tree for gfx950 (explicit hipcc, no JIT cache).

``python -m ouzelum_amd.build`` or ``__graft_entry__.build()``.  The library is
written next to this file so it travels to the GPU box with the repo snapshot.
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRCS = [os.path.join(HERE, "csrc", "quad_kernels.hip"), os.path.join(HERE, "csrc", "learner_kernels.hip")]
DEPS = [*SRCS, *(os.path.join(HERE, "csrc", h) for h in ("quad_math.h", "quad_env.h", "philox.h", "quad_pv_ql.h",
                                                          "quad_pv_split.h", "quad_policy.h", "quad_policy_lstm.h")),
        os.path.join(ROOT, "include", "ouzelum.h")]
# the host build of the same step (make(sim_device="cpu"); include/ouzelum_host.h)
HOST_SRC = os.path.join(HERE, "csrc", "quad_host.cpp")
HOST_DEPS = [HOST_SRC, *(os.path.join(HERE, "csrc", h) for h in ("quad_math.h", "quad_env.h", "philox.h",
                                                                 "host_compat.h")),
             os.path.join(ROOT, "include", "ouzelum.h"), os.path.join(ROOT, "include", "ouzelum_host.h")]
HOST_OUT = os.path.join(HERE, "libouzelum_cpu.so")
CXX = os.environ.get("CXX", "g++")
# x86-64-v3 (AVX2 + FMA): the build container's and the GPU boxes' EPYC hosts; no FMA contraction (the f32 step
# rounds each operation, like the oracle's numpy), OpenMP over the envs of a step (libgomp, torch's own runtime)
HOST_FLAGS = ["-O3", "-std=c++17", "-march=x86-64-v3", "-ffp-contract=off", "-fopenmp", "-fPIC", "-shared",
              "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-variable", "-DOUZ_HOST"]
OUT = os.environ.get("OUZ_BUILD_OUT") or os.path.join(HERE, "libouzelum_hip.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ARCH = os.environ.get("OUZ_OFFLOAD_ARCH", "gfx950")
FLAGS = ["-O3", "-std=c++17", "-shared", "-fPIC", f"--offload-arch={ARCH}", "-Wno-unused-result",
         # f32 divide / sqrt to ~1-2 ulp instead of correctly rounded: -14 % VALU in the step kernel,
         # well inside the parity tolerances.  f64 (PV filter) and the RNG (__f*_rn) are unaffected.
         "-fno-hip-fp32-correctly-rounded-divide-sqrt",
         # FMA contraction within an expression (a * b + c), never across statements, except where a
         # `#pragma clang fp contract(off)` asks for torch's one-rounding-per-op order (RNG uniforms, GAE):
         # __fmul_rn/__fadd_rn are plain operators in HIP.  With cross-statement fusion (fast) the rounding
         # of the step depended on the code around it (basic-block boundaries, a value's other uses), so the
         # kernel forms (one-lane / split-wave / quad-lane / output-wave, step / rollout) needed empty-asm seals
         # to stay bitwise equal; with "on" they are equal by construction.
         "-ffp-contract=on",
         # no SLP packing of f32 pairs into v_pk_*: on this per-lane scalar code it only adds register-pair
         # moves (v_mov -60 %, -5..7 % instructions per step phase) and ~40 VGPRs in the estimator kernels: it picks
         # pairs expression by expression, with no layout.  Where packing pays it is written by hand with one layout
         # (quad_math.h P3 / PQ / PR: the plain LeeLanded rollout's state wave, 468 -> 411 instructions per step,
         # +7 % env-steps/s; docs/HISTORY.md round 20), and this flag keeps the rest scalar.
         "-fno-slp-vectorize",
         # f32 denormals flush to zero: rcp / rsq / sqrt become single instructions instead of 5-6 with
         # range scaling (-7..10 % instructions in the controller / integrator phases).  State, RNG uniforms
         # and learner tensors are normal floats; f64 (the PV filter) keeps denormals.
         "-fgpu-flush-denormals-to-zero",
         # machine scheduler for instruction-level parallelism: at the 4096-env bench size a CU runs ONE wave,
         # whose step is a dependent instruction chain (~6.7 cycles per instruction against the 4-cycle issue
         # floor), so latency hiding inside the wave beats occupancy.  Measured against the default
         # (scripts/archive/lib_ab.sh, one box): fused LeeLanded 2.08 -> 2.02 us per step, per-step kernel
         # 3.51 -> 3.38 us, the other configs within +-1 %, large-N HBM fractions unchanged.  The iterative-ilp
         # and max-memory-clause strategies measured 1-3 % slower on the fused B / C / D steps
         # (profiles/r02/sched_strategy_ab.txt).
         "-mllvm", "-amdgpu-sched-strategy=max-ilp"]


def up_to_date(out=OUT, deps=DEPS) -> bool:
    if not os.path.exists(out):
        return False
    t = os.path.getmtime(out)
    return all(os.path.getmtime(d) <= t for d in deps)


def source_id(extra=()) -> str:
    """16 hex digits of sha256 over the library's sources (DEPS, in order) and its build flags.  Compiled into the
    library (``ouz_source_id()``): hipcc names every compilation unit with a random id that ends up in the
    binary, so two builds of the same sources differ in bytes; PMC evidence is matched to a library by this id."""
    import hashlib
    h = hashlib.sha256()
    for d in DEPS:
        with open(d, "rb") as fh:
            h.update(os.path.relpath(d, ROOT).encode() + b"\0" + fh.read() + b"\0")
    h.update(" ".join([*FLAGS, *extra]).encode())
    return h.hexdigest()[:16]


def build_host(force: bool = False, verbose: bool = True) -> str:
    """libouzelum_cpu.so: quad_host.cpp (quad_env.h + quad_math.h for the host) with g++ and OpenMP."""
    if not force and up_to_date(HOST_OUT, HOST_DEPS):
        return HOST_OUT
    cmd = [CXX, *HOST_FLAGS, "-o", HOST_OUT + ".tmp", HOST_SRC]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    os.replace(HOST_OUT + ".tmp", HOST_OUT)
    return HOST_OUT


def build(force: bool = False, verbose: bool = True) -> str:
    """The HIP library (OUT), after the host library unless this is a variant build (OUZ_BUILD_OUT).  A failed host
    build (no g++ / OpenMP) does not stop the HIP build: it is reported, and make(sim_device="cpu") raises until
    the host library exists."""
    if not os.environ.get("OUZ_BUILD_OUT"):
        try:
            build_host(force=force, verbose=verbose)
        except (OSError, subprocess.CalledProcessError) as e:
            print(f"ouzelum_amd.build: host library (libouzelum_cpu.so) not built: {e}", file=sys.stderr, flush=True)
    if not force and up_to_date():
        return OUT
    extra = os.environ.get("OUZ_EXTRA_FLAGS", "").split()
    sid = source_id(extra)
    cmd = [HIPCC, *FLAGS, *extra, f'-DOUZ_SOURCE_ID="{sid}"', "-o", OUT + ".tmp", *SRCS]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    os.replace(OUT + ".tmp", OUT)
    return OUT


EXAMPLE_SRC = os.path.join(ROOT, "examples", "c_host_step.cpp")
EXAMPLE_OUT = os.path.join(ROOT, "examples", "c_host_step")


def build_examples(verbose: bool = True) -> str:
    """The C/C++ host example linked against the in-tree library (rpath to ouzelum_amd/)."""
    cmd = [HIPCC, "-O2", "-std=c++17", f"--offload-arch={ARCH}", "-Wno-unused-result",
           "-I", os.path.join(ROOT, "include"), EXAMPLE_SRC, "-L", HERE, "-louzelum_hip",
           "-Wl,-rpath,$ORIGIN/../ouzelum_amd", "-o", EXAMPLE_OUT]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    return EXAMPLE_OUT


if __name__ == "__main__":
    build(force="--force" in sys.argv)
    build_examples()
