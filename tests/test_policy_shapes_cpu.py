"""The three learner families' packers and host layouts at the shape edges of tests/policy_shape_cases.py, without a GPU: the five
trunks (three layers, widths 80..240, actor and critic on different sides of 64) at (D, A) in {(1, 1), (12, 9), (12, 13), (45, 16),
(58, 1)}, which the older CPU files' shapes ((10, 7), (25, 4), (25, 8), one or two layers) leave out."""
import ctypes as C

import pytest
import torch

from tests import indep_policy as ip
from tests import indep_sac as isac
from tests import indep_td3 as it
from tests import policy_shape_cases as psc
from tests.test_policy_cpu import _arr, _pol
from tests.test_sac_cpu import _floats as sac_floats
from tests.test_sac_cpu import _sac
from tests.test_td3_cpu import _floats as td3_floats
from tests.test_td3_cpu import _td3

SHAPES = [(D, A, t) for (D, A) in psc.CPU_DIMS for t in psc.TRUNK_NAMES]


def once_and_plus_zero(blob, own):
    """Every weight sits in the blob exactly once, and everything else is +0.0 bit for bit."""
    assert int((blob != 0).sum()) == sum(int((v != 0).sum()) for v in own)
    assert not (blob.view(torch.int32)[blob == 0] != 0).any()


def same_bytes(back, sd):
    assert set(back) == set(sd)
    for k, v in sd.items():
        assert back[k].shape == v.shape and back[k].numpy().tobytes() == v.detach().numpy().tobytes(), k


# ------------------------------------------------------------------------------------------------------------ the packers
@pytest.mark.parametrize("D,A,trunk", SHAPES)
def test_policy_pack_unpack_round_trip_bit_for_bit(built, D, A, trunk):
    from mycobotgym_amd import _abi, policy
    pi, vf, act = ip.TRUNKS[trunk]
    sd = ip.Twin(D, A, pi, vf, act).randomize(11).state_dict()
    blob = policy.pack(sd, D, A, pi, vf)
    assert blob.dtype == torch.float32 and blob.numel() == _abi.load().mcg_policy_blob_floats(D, A, len(pi), _arr(pi), len(vf), _arr(vf)) > 0
    back = policy.unpack(blob, D, A, pi, vf)
    assert set(back) == set(policy.state_names(len(pi), len(vf)))
    same_bytes(back, sd)
    once_and_plus_zero(blob, sd.values())
    assert torch.equal(policy.pack(back, D, A, pi, vf).view(torch.int32), blob.view(torch.int32))


@pytest.mark.parametrize("D,A,trunk", SHAPES)
def test_sac_pack_unpack_round_trip_bit_for_bit(built, D, A, trunk):
    from mycobotgym_amd import _abi, sac_policy as sp
    pi, qf, act = isac.TRUNKS[trunk]
    sd = isac.Twin(D, A, pi, qf, act).randomize(11, D).state_dict()
    total, fa, fc = sac_floats(_abi.load(), D, A, pi, qf)
    blobs = {"actor": sp.pack_actor(sd, D, A, pi), "critic": sp.pack_critic(sd, D, A, qf, "critic"),
             "critic_target": sp.pack_critic(sd, D, A, qf, "critic_target")}
    assert all(b.dtype == torch.float32 for b in blobs.values())
    assert [b.numel() for b in blobs.values()] == [fa, fc, fc] and total == fa + fc > 0 and fa % 16 == 0 and fc % 32 == 0
    back = sp.unpack_actor(blobs["actor"], D, A, pi)
    back.update(sp.unpack_critic(blobs["critic"], D, A, qf, "critic"))
    back.update(sp.unpack_critic(blobs["critic_target"], D, A, qf, "critic_target"))
    assert set(back) == set(sp.state_names(len(pi), len(qf)))
    same_bytes(back, sd)
    for name, blob in blobs.items():
        once_and_plus_zero(blob, [v for k, v in sd.items() if k.startswith(name + ".")])
        again = sp.pack_actor(back, D, A, pi) if name == "actor" else sp.pack_critic(back, D, A, qf, name)
        assert torch.equal(again.view(torch.int32), blob.view(torch.int32)), name


@pytest.mark.parametrize("nc", [1, 2])
@pytest.mark.parametrize("D,A,trunk", SHAPES)
def test_td3_pack_unpack_round_trip_bit_for_bit(built, D, A, trunk, nc):
    from mycobotgym_amd import _abi, td3_policy as tp
    pi, qf, act = it.TRUNKS[trunk]
    sd = it.Twin(D, A, pi, qf, act, nc).randomize(11).state_dict()
    total, fa, fc = td3_floats(_abi.load(), D, A, pi, qf, nc)
    blobs = {"actor": tp.pack_actor(sd, D, A, pi, "actor"), "actor_target": tp.pack_actor(sd, D, A, pi, "actor_target"),
             "critic": tp.pack_critic(sd, D, A, qf, "critic", nc), "critic_target": tp.pack_critic(sd, D, A, qf, "critic_target", nc)}
    assert all(b.dtype == torch.float32 for b in blobs.values())
    assert [b.numel() for b in blobs.values()] == [fa, fa, fc, fc] and total == fa + fc > 0 and fa % 16 == 0 and fc % 16 == 0
    back = {}
    for name in ("actor", "actor_target"):
        back.update(tp.unpack_actor(blobs[name], D, A, pi, name))
    for name in ("critic", "critic_target"):
        back.update(tp.unpack_critic(blobs[name], D, A, qf, name, nc))
    assert set(back) == set(tp.state_names(len(pi), len(qf), nc))
    same_bytes(back, sd)
    for name, blob in blobs.items():
        once_and_plus_zero(blob, [v for k, v in sd.items() if k.startswith(name + ".")])
        again = tp.pack_actor(back, D, A, pi, name) if name.startswith("actor") else tp.pack_critic(back, D, A, qf, name, nc)
        assert torch.equal(again.view(torch.int32), blob.view(torch.int32)), name


# ------------------------------------------------------------------------------------------------- the blob sizes by hand
def test_three_layer_blob_floats_by_hand(built):
    """A first layer of `out` units holds out x 4 kb0 weights (the D + 6 feature columns padded to kb0 = ceil((D + 6) / 4) k-blocks
    of 4) and out biases; a critic's first layer 16 more columns per unit, the action's; a later layer out x in + out; a head is one
    tile of 16 rows: 16 x in + 16; ActorCritic's log_std is 16 floats."""
    from mycobotgym_amd import _abi
    L = _abi.load()
    # ActorCritic, D = 12 (18 features, kb0 = 5: 20 columns), pi = (80, 16, 112), vf = (96, 240, 16)
    pi_net = (80 * 20 + 80) + (16 * 80 + 16) + (112 * 16 + 112) + (16 * 112 + 16)
    vf_net = (96 * 20 + 96) + (240 * 96 + 240) + (16 * 240 + 16) + (16 * 16 + 16)
    assert L.mcg_policy_blob_floats(12, 13, 3, _arr((80, 16, 112)), 3, _arr((96, 240, 16))) == pi_net + vf_net + 16
    # SAC, D = 45 (51 features, kb0 = 13: 52 columns), A = 13, pi = qf = (64, 64, 64): two heads for the actor, two critics
    actor = (64 * 52 + 64) + 2 * (64 * 64 + 64) + 2 * (16 * 64 + 16)
    critic = 2 * ((64 * (52 + 16) + 64) + 2 * (64 * 64 + 64) + (16 * 64 + 16))
    assert sac_floats(L, 45, 13, (64, 64, 64), (64, 64, 64)) == (actor + critic, actor, critic)
    # TD3, D = 1 (7 features, kb0 = 2: 8 columns), A = 1, pi = (32, 48, 16), qf = (16, 48, 32): one head, one or two critics
    actor = (32 * 8 + 32) + (48 * 32 + 48) + (16 * 48 + 16) + (16 * 16 + 16)
    one = (16 * (8 + 16) + 16) + (48 * 16 + 48) + (32 * 48 + 32) + (16 * 32 + 16)
    assert td3_floats(L, 1, 1, (32, 48, 16), (16, 48, 32), 2) == (actor + 2 * one, actor, 2 * one)
    assert td3_floats(L, 1, 1, (32, 48, 16), (16, 48, 32), 1) == (actor + one, actor, one)


# ------------------------------------------------------------------------------------------------------- the work layout
def _fr(D):
    return (D + 6 + 15) // 16 * 16                                   # the feature rows of a tile's chunk, padded to 16


@pytest.mark.parametrize("D,A,trunk,B", psc.CASES)
def test_grad_work_floats_cover_the_restated_layout(built, D, A, trunk, B):
    """Per tile and net, `work` holds 16 floats for each row of the chunk: the feature rows, every layer's activations and dZ rows
    (its width each), 16 rows of the head's dZ, and what the entry adds (the policy net's log_std rows, the critics' 16 action rows,
    the actor entry's second head and its copy of the critics' activations); then one partial blob per part; in front, 4 floats (8
    for the policy update) and 8 per tile of sums.  The C side's count is at least the rows and the partial blobs, and at most those plus the sums."""
    from mycobotgym_amd import _abi
    L = _abi.load()
    T, fr, sums = psc.tiles(B), _fr(D), 4 + 8 * psc.tiles(B)
    pi, vf, _ = ip.TRUNKS[trunk]
    blob = L.mcg_policy_blob_floats(D, A, len(pi), _arr(pi), len(vf), _arr(vf))
    pol = _pol(_abi, L, obs_dim=D, act_dim=A, n_pi=len(pi), pi_width=_arr(pi), n_vf=len(vf), vf_width=_arr(vf))
    rows = (fr + 2 * sum(pi) + 16 + 16) + (fr + 2 * sum(vf) + 16)
    want = T * 16 * rows + psc.parts(B, max(pi + vf)) * blob
    need = L.mcg_policy_grad_work_floats(C.byref(pol), C.c_int64(B))
    assert need > 0 and want <= need <= want + sums + 4, ("policy", need, want)      # (4 more floats in front: the advantage's statistics)

    pi, qf, _ = isac.TRUNKS[trunk]
    _, fa, fc = sac_floats(L, D, A, pi, qf)
    sac = _sac(_abi, L, obs_dim=D, act_dim=A, n_pi=len(pi), pi_width=_arr(pi), n_qf=len(qf), qf_width=_arr(qf))
    critic = 2 * T * 16 * (fr + 16 + 2 * sum(qf) + 16) + psc.parts(B, max(qf)) * fc
    actor = T * 16 * (fr + 2 * sum(pi) + 16 + 16) + 2 * T * 16 * sum(qf) + psc.parts(B, max(pi)) * fa
    want = max(critic, actor)
    need = L.mcg_sac_grad_work_floats(C.byref(sac), C.c_int64(B))
    assert need > 0 and want <= need <= want + sums, ("sac", need, want)

    for nc in (1, 2):
        _, fa, fc = td3_floats(L, D, A, pi, qf, nc)
        td3 = _td3(_abi, L, obs_dim=D, act_dim=A, n_pi=len(pi), pi_width=_arr(pi), n_qf=len(qf), qf_width=_arr(qf), n_critics=nc)
        critic = nc * T * 16 * (fr + 16 + 2 * sum(qf) + 16) + psc.parts(B, max(qf)) * fc
        actor = T * 16 * (fr + 2 * sum(pi) + 16) + T * 16 * sum(qf) + psc.parts(B, max(pi)) * fa
        want = max(critic, actor)
        need = L.mcg_td3_grad_work_floats(C.byref(td3), C.c_int64(B))
        assert need > 0 and want <= need <= want + sums, ("td3", nc, need, want)


def test_the_split_restated():
    """38 tiles: 13 parts of 3 up to width 64, 4 parts of 10 above; up to 16 (or 4) tiles one part each."""
    assert (psc.tiles(600), psc.parts(600, 32), psc.parts(600, 80)) == (38, 13, 4)
    assert (psc.parts(75, 64), psc.parts(75, 80), psc.parts(33, 240), psc.parts(1, 256)) == (5, 3, 3, 1)
