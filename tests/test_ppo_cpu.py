"""The policy update's restatement (tests/indep_ppo.py) against finite differences and against torch's own optimiser and clip, the
batch maker's census, and the Python-side refusals of PPOUpdate / evaluate_actions that need no device.  No GPU."""
import types

import numpy as np
import pytest
import torch

from tests import indep_policy as ip
from tests import indep_ppo as pp


def small_twin():
    return ip.Twin(4, 2, (16,), (16,), "tanh").double().randomize(3)


@pytest.mark.parametrize("hyper", [dict(loss="ppo", normalize_advantage=True), dict(loss="ppo", normalize_advantage=False),
                                   dict(loss="a2c", normalize_advantage=True)], ids=["ppo-norm", "ppo", "a2c"])
def test_autograd_equals_finite_differences(hyper):
    """float64, central differences of step 1e-6 on a [16] net, (D, A) = (4, 2), B = 7: 1e-6 relative per tensor."""
    twin = small_twin()
    batch, _ = pp.make_batch(twin, 4, 2, 7, seed=5)
    hyper = dict(hyper, ent_coef=0.01, vf_coef=0.5, clip_range=0.2)
    grads, _ = pp.grad_and_stats(twin, batch, **hyper)
    h = 1e-6
    for name, p in twin.named_parameters():
        fd = np.zeros(p.numel())
        flat = p.data.view(-1)
        for j in range(p.numel()):
            keep = float(flat[j])
            with torch.no_grad():
                flat[j] = keep + h
                up = float(pp.loss_terms(twin, batch, **hyper)["loss"])
                flat[j] = keep - h
                down = float(pp.loss_terms(twin, batch, **hyper)["loss"])
                flat[j] = keep
            fd[j] = (up - down) / (2 * h)
        g = grads[name].reshape(-1)
        assert np.abs(g).max() > 0, name
        assert np.abs(g - fd).max() <= 1e-6 * np.abs(g).max(), (name, np.abs(g - fd).max(), np.abs(g).max())


def test_adam_restatement_equals_torch():
    rng = np.random.default_rng(0)
    p0 = rng.normal(size=(5, 3))
    p = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([p], lr=3e-4, betas=(0.9, 0.999), eps=1e-5)
    q, m, v = p0.copy(), np.zeros_like(p0), np.zeros_like(p0)
    for step in range(1, 6):
        g = rng.normal(size=p0.shape) * 10.0 ** rng.integers(-3, 2)
        p.grad = torch.from_numpy(g.copy())
        opt.step()
        q, m, v = pp.adam_step(q, g, m, v, step, 3e-4, 0.9, 0.999, 1e-5)
        assert np.abs(p.detach().numpy() - q).max() <= 1e-12, step


@pytest.mark.parametrize("max_norm", [0.5, 1e-3, 100.0])
def test_clip_restatement_equals_clip_grad_norm(max_norm):
    rng = np.random.default_rng(1)
    grads = {"a": rng.normal(size=(4, 3)), "b": rng.normal(size=7)}
    params = [torch.nn.Parameter(torch.zeros(g.shape, dtype=torch.float64)) for g in grads.values()]
    for p, g in zip(params, grads.values()):
        p.grad = torch.from_numpy(g.copy())
    norm = float(torch.nn.utils.clip_grad_norm_(params, max_norm))
    assert abs(norm - pp.global_norm(grads)) <= 1e-12 * norm
    coef = pp.clip_coef(pp.global_norm(grads), max_norm)
    for p, g in zip(params, grads.values()):
        assert np.abs(p.grad.numpy() - coef * g).max() <= 1e-14
    assert pp.clip_coef(3.0, 0.0) == 1.0 and pp.clip_coef(3.0, -1.0) == 1.0


@pytest.mark.parametrize("trunk", list(ip.TRUNKS))
@pytest.mark.parametrize("D,A", ip.DIMS)
def test_the_batch_makers_census(D, A, trunk):
    pi, vf, act = ip.TRUNKS[trunk]
    twin = ip.Twin(D, A, pi, vf, act).double().randomize(3)
    batch, census = pp.make_batch(twin, D, A, 75, seed=5, relu=act == "relu")
    print(trunk, D, A, census)
    assert census["dropped"] < 0.10
    assert 0.0 < census["clip_fraction"] < 1.0                   # both clip branches
    assert 0.0 < census["positive_advantages"] < 1.0             # both signs
    assert census["clip_margin"] >= 1e-3
    assert all(np.array_equal(v, v.astype(np.float32).astype(np.float64)) for v in (batch["actions"], batch["old_log_prob"], batch["advantages"]))
    assert batch["actions"].shape == (75, A) and batch["obs"]["observation"].shape == (75, D)


# ------------------------------------------------------------------------------------------------------------ refusals
def fake_policy(D=10, A=7):
    return types.SimpleNamespace(obs_dim=D, act_dim=A, blob_floats=16, device=torch.device("cpu"), pi=(16,), vf=(16,))


def samples(B=5, D=10, A=7, **over):
    from mycobotgym_amd import RolloutSamples
    f = dict(observations={"observation": torch.zeros(B, D), "achieved_goal": torch.zeros(B, 3), "desired_goal": torch.zeros(B, 3)},
             actions=torch.zeros(B, A), old_values=torch.zeros(B), old_log_prob=torch.zeros(B), advantages=torch.zeros(B), returns=torch.zeros(B),
             index=torch.zeros(B, dtype=torch.int32))
    f.update(over)
    return RolloutSamples(**f)


def test_constructor_refusals():
    from mycobotgym_amd import PPOUpdate
    pol = fake_policy()
    with pytest.raises(ValueError, match="loss must be one of"):
        PPOUpdate(pol, loss="trpo")
    with pytest.raises(ValueError, match="clip_range must be > 0"):
        PPOUpdate(pol, clip_range=0.0)
    with pytest.raises(ValueError, match="clip_range_vf is not built"):
        PPOUpdate(pol, clip_range_vf=0.2)
    with pytest.raises(ValueError, match="target_kl is not built"):
        PPOUpdate(pol, target_kl=0.01)
    with pytest.raises(TypeError, match="unexpected keyword"):
        PPOUpdate(pol, momentum=0.9)
    with pytest.raises(ValueError, match="betas"):
        PPOUpdate(pol, betas=(0.9, 1.0))
    opt = PPOUpdate(pol, loss="a2c", clip_range=0.0)             # A2C does not read clip_range
    assert opt.steps == 0 and opt.loss == "a2c"


def test_minibatch_refusals():
    from mycobotgym_amd import PPOUpdate
    from mycobotgym_amd.policy_update import check_minibatch
    assert check_minibatch(samples(), 10, 7, True) == 5
    with pytest.raises(ValueError, match="picture buffers"):
        check_minibatch(samples(observations=torch.zeros(5, 3, 8, 8, dtype=torch.uint8)), 10, 7, True)
    with pytest.raises(ValueError, match="expected float32"):
        check_minibatch(samples(observations={"observation": torch.zeros(5, 10, dtype=torch.float64), "achieved_goal": torch.zeros(5, 3),
                                              "desired_goal": torch.zeros(5, 3)}), 10, 7, True)
    with pytest.raises(ValueError, match="expected shape"):
        check_minibatch(samples(D=11), 10, 7, True)
    with pytest.raises(ValueError, match="actions"):
        check_minibatch(samples(A=6), 10, 7, True)
    with pytest.raises(ValueError, match="B must be >= 1"):
        check_minibatch(samples(B=0), 10, 7, True)
    with pytest.raises(ValueError, match="advantages"):
        check_minibatch(samples(advantages=torch.zeros(4)), 10, 7, True)
    with pytest.raises(ValueError, match="old_log_prob"):
        check_minibatch(samples(old_log_prob=torch.zeros(5, dtype=torch.float64)), 10, 7, True)
    assert check_minibatch(samples(old_log_prob=None), 10, 7, False) == 5       # A2C does not read it
    with pytest.raises(ValueError, match="no field"):
        check_minibatch((1, 2, 3), 10, 7, True)
    opt = PPOUpdate(fake_policy())
    opt.clip_range = -0.1                                        # settable between steps: checked again at the step
    with pytest.raises(ValueError, match="clip_range must be > 0"):
        opt.compute_grad(samples())
