"""The conditions of tests/test_gpu_pnp_controllers_on_contacts.py, checked on the CPU oracle alone (no GPU):

* the start states hold what they are meant to hold: the random policies reach mesh contacts (and, under fetch-mocap, lists cut by the cap),
  and every pose family holds a contact beyond the resting cube's four on the controller's own model table;
* the oracle's own sensitivity on these states: a twin oracle started +-1e-14 away (robot joints only, tests.common.twin_errors) stays within
  1e-12 after one sub-step and within 1e-10 after a mocap env-step of 20 sub-steps.  The GPU file's absolute bounds (1e-10 .. 1e-9) are
  therefore the kernels' to use up, not the reference's.

The rollouts are chaotic and the oracle is built for the host's CPU, so the census is asserted with floors at about half of the counts
measured when the tests were written (mocap 46 / 0, fetch-mocap 132 / 22, IK 35 / 0, fetch-IK 69 / 0: with a mesh contact / cut by the cap)."""
import numpy as np
import pytest

from tests import pnp_contact_states as cs
from tests.common import make_oracle, twin_errors

FLOORS = {"mocap": (20, 0), "fetch-mocap": (48, 8), "IK": (16, 0), "fetch-IK": (32, 0)}      # (with a mesh contact, cut by the cap)
ROBOT = slice(0, 12)


@pytest.mark.parametrize("name", list(cs.CONTROLLERS))
def test_random_policy_census(name):
    r = cs.random_policy_states(name)
    c = r["census"]
    print(f"\n[{name}] random policy, 45 env-steps x {c['n']} envs: {c['mesh']} with a mesh contact, {c['cut']} cut by the cap, largest list {c['ncon_max']}, "
          f"|qvel| max {c['qvel_max']:.2e}; picked {int(r['mesh'].sum())} with (of them {int(r['cut'].sum())} cut) + {int((~r['mesh']).sum())} without")
    assert c["finite"]
    assert c["mesh"] >= FLOORS[name][0] and c["cut"] >= FLOORS[name][1]
    assert len(r["mesh"]) <= cs.N_POSES and int((~r["mesh"]).sum()) >= 8
    assert r["state"]["qpos"].shape == (len(r["mesh"]), 19) and not r["state"]["elapsed"].any()


@pytest.mark.parametrize("mocap", [False, True])
@pytest.mark.parametrize("family", cs.FAMILIES)
def test_pose_families_hold_their_contacts(family, mocap):
    """On the controller's own table, at least half of a family's poses hold a contact beyond the resting cube's four (the cube families put
    the cube on a link instead: any contact with a mesh geom there)."""
    name = "mocap" if mocap else "IK"
    poses = cs.pose_family(family, mocap)
    ora = make_oracle(cs.N_POSES, **cs.engine_kw(name))
    ora.reset(seed=3)
    cs.put_poses(ora, family, poses)
    has, cut, ncon = cs.contact_census(ora)
    beyond = has if family in cs.CUBE_FAMILIES else (ncon > 4)
    print(f"\n[{name}] family {family}: {int(beyond.sum())} of {cs.N_POSES} poses with their contact, list sizes {ncon.min()}..{ncon.max()}, {int(cut.sum())} cut by the cap")
    assert np.isfinite(poses).all()
    assert beyond.sum() >= cs.N_POSES // 2


def _twin_run(name, start, steps, frame_skip, seed=1):
    """Worst twin difference over `steps` launches from `start` (("family", f) or ("random",)), actions as in the GPU file."""
    kw = cs.engine_kw(name, frame_skip=frame_skip)
    if start[0] == "family":
        n = cs.N_POSES
        ora, twin = make_oracle(n, **kw), make_oracle(n, **kw)
        ora.reset(seed=3); twin.reset(seed=3)
        cs.put_poses(ora, start[1], cs.pose_family(start[1], cs.CONTROLLERS[name][0] == "mocap"))
    else:
        st = cs.random_policy_states(name)["state"]
        n = len(st["elapsed"])
        ora, twin = make_oracle(n, **kw), make_oracle(n, **kw)
        ora.reset(seed=3); twin.reset(seed=3)
        cs.put_state(ora, st)
    rng = np.random.default_rng(seed); prng = np.random.default_rng(7)
    worst = 0.0; ncon_max = 0; vmax = 0.0
    for t in range(steps):
        if t % 20 == 0 or frame_skip > 1: a = cs.draw_actions(rng, ora)
        state = ora.get_state()
        o = ora.step(a)
        worst = max(worst, float(twin_errors(twin, state, a, o, prng, cols=ROBOT).max()))
        ncon_max = max(ncon_max, int(cs.list_sizes(ora).max()))
        s = ora.get_state()
        assert np.isfinite(s["qpos"]).all() and np.isfinite(s["qvel"]).all()
        vmax = max(vmax, float(np.abs(s["qvel"]).max()))
    return worst, ncon_max, vmax


@pytest.mark.parametrize("name", ["IK", "mocap", "fetch-mocap"])
def test_one_substep_sensitivity_on_pose_families(name):
    for family in cs.FAMILIES:
        worst, ncon_max, vmax = _twin_run(name, ("family", family), 40, 1)
        print(f"\n[{name}] {family}: 40 sub-steps x {cs.N_POSES} envs, twin (+-1e-14 on the robot's joints) differs by at most {worst:.2e}; "
              f"largest list {ncon_max}, |qvel| max {vmax:.2e}")
        assert worst <= 1e-12


@pytest.mark.parametrize("name", list(cs.CONTROLLERS))
def test_one_substep_sensitivity_from_random_policy_states(name):
    worst, ncon_max, vmax = _twin_run(name, ("random",), 20, 1)
    print(f"\n[{name}] random-policy states: 20 sub-steps, twin differs by at most {worst:.2e}; largest list {ncon_max}, |qvel| max {vmax:.2e}")
    assert worst <= 1e-12


@pytest.mark.parametrize("name", ["mocap", "fetch-mocap"])
def test_mocap_env_step_sensitivity(name):
    for start in (("family", "mesh"), ("random",)):
        worst, ncon_max, vmax = _twin_run(name, start, 2, 20)
        print(f"\n[{name}] {start[-1]}: two env-steps of 20 sub-steps, twin differs by at most {worst:.2e}; largest list {ncon_max}, |qvel| max {vmax:.2e}")
        assert worst <= 1e-10
