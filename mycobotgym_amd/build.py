"""In-tree build of the HIP library (gfx950 only)."""
from __future__ import annotations

import glob
import os
import shutil
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
SRC = os.path.join(_HERE, "csrc", "mcg_hip.hip")
SRC_RENDER = os.path.join(_HERE, "csrc", "mcg_render.hip")      # the ray caster: a code object of its own (see the file)
SRC_REPLAY = os.path.join(_HERE, "csrc", "mcg_replay.hip")      # the hindsight replay buffer: likewise
SRC_ROLLOUT = os.path.join(_HERE, "csrc", "mcg_rollout.hip")    # the on-policy rollout buffers: likewise
SRC_REPLAY_IMG = os.path.join(_HERE, "csrc", "mcg_replay_img.hip")      # the off-policy replay buffer of pictures: likewise
SRC_FRAME_STACK = os.path.join(_HERE, "csrc", "mcg_frame_stack.hip")    # act-time frame stacking: likewise
SRC_POLICY = os.path.join(_HERE, "csrc", "mcg_policy.hip")      # the actor-critic policy forward: likewise
SRC_POLICY_GRAD = os.path.join(_HERE, "csrc", "mcg_policy_grad.hip")    # the policy update (gradient, Adam): likewise
SRC_SAC = os.path.join(_HERE, "csrc", "mcg_sac.hip")            # SAC's actor, twin critics and TD target: likewise
SRC_SAC_GRAD = os.path.join(_HERE, "csrc", "mcg_sac_grad.hip")  # SAC's update (critic, actor and alpha gradients, Adam): likewise
SRC_TD3 = os.path.join(_HERE, "csrc", "mcg_td3.hip")            # TD3's / DDPG's actor, critics and smoothed TD target: likewise
SRC_TD3_GRAD = os.path.join(_HERE, "csrc", "mcg_td3_grad.hip")  # TD3's / DDPG's update (critic and actor gradients): likewise
SRC_CNN = os.path.join(_HERE, "csrc", "mcg_cnn.hip")            # the CNN actor-critic forward of the picture ids: likewise
SRC_SELFTEST = os.path.join(_HERE, "csrc", "mcg_selftest.hip")  # device self-tests of step-kernel functions (test-only entries): likewise
DEPS = sorted(glob.glob(os.path.join(_HERE, "csrc", "*"))) + [os.path.join(ROOT, "include", "mcg.h")]      # every source and header
OUT = os.path.join(_HERE, "libmycobot_hip.so")


def source_hash() -> str:
    """sha256 over the kernel sources (csrc/*, include/mcg.h): stamps counter measurements, so that bench.py can tell when
    profiles/pmc_latest.json was collected on other kernels than the ones it is running."""
    import hashlib
    h = hashlib.sha256()
    for d in DEPS:
        h.update(os.path.basename(d).encode()); h.update(open(d, "rb").read())
    return h.hexdigest()


def hipcc() -> str:
    for c in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found")


def build_hip(force: bool = False, verbose: bool = False) -> str:
    if not force and os.path.exists(OUT) and all(os.path.getmtime(OUT) >= os.path.getmtime(d) for d in DEPS):
        return OUT
    cmd = [hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++20", "-fPIC", "-shared",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(_HERE, "csrc"), SRC, SRC_RENDER, SRC_REPLAY, SRC_ROLLOUT, SRC_REPLAY_IMG,
           SRC_FRAME_STACK, SRC_POLICY, SRC_POLICY_GRAD, SRC_SAC, SRC_SAC_GRAD, SRC_TD3, SRC_TD3_GRAD, SRC_CNN, SRC_SELFTEST,
           "-o", OUT]
    if verbose:
        cmd.insert(1, "-Rpass-analysis=kernel-resource-usage")
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed:\n" + r.stderr[-4000:])
    if verbose:
        print(r.stderr)
    return OUT
