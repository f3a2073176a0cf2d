"""The refusals of the Python host layer of the policy families, word for word: each named case below must raise, and its
(exception type, text) is compared with tests/golden/host_refusals.json, recorded before the host layer was folded onto `_nets.py`
(the `cnn-*` cases: before `CnnActorCritic` was).

No GPU and no built library: the cases stop at a check that needs neither.  Tiny inputs: B = 5, D = 10, A = 7, widths 16; pictures 36 x 36.  Refusals
whose text names a device (``.. lives on ..``) are the GPU tests'.  Run as a script, this file writes the fixture:

    python tests/test_host_refusals_cpu.py
"""
import json
import os
import sys
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "host_refusals.json")
B, D, A, W = 5, 10, 7, 16
CPU = torch.device("cpu")
nn = torch.nn


# ---------------------------------------------------------------------------------------------------------------- inputs
def obs(rows=B, cols=D, **over):
    o = {"observation": torch.zeros(rows, cols), "achieved_goal": torch.zeros(rows, 3), "desired_goal": torch.zeros(rows, 3)}
    o.update(over)
    return o


def without(d, k):
    return {n: v for n, v in d.items() if n != k}


def ppo_sd(**over):
    sd = {"mlp_extractor.policy_net.0.weight": torch.zeros(W, D + 6), "mlp_extractor.policy_net.0.bias": torch.zeros(W),
          "action_net.weight": torch.zeros(A, W), "action_net.bias": torch.zeros(A),
          "mlp_extractor.value_net.0.weight": torch.zeros(W, D + 6), "mlp_extractor.value_net.0.bias": torch.zeros(W),
          "value_net.weight": torch.zeros(1, W), "value_net.bias": torch.zeros(1), "log_std": torch.zeros(A)}
    sd.update(over)
    return sd


def samples(**over):
    from mycobotgym_amd import RolloutSamples
    f = dict(observations=obs(), actions=torch.zeros(B, A), old_values=torch.zeros(B), old_log_prob=torch.zeros(B), advantages=torch.zeros(B),
             returns=torch.zeros(B), index=torch.zeros(B, dtype=torch.int32))
    f.update(over)
    return RolloutSamples(**f)


def replay(**over):
    f = dict(observations=obs(), actions=torch.zeros(B, A), next_observations=obs(), dones=torch.zeros(B, 1), rewards=torch.zeros(B))
    f.update(over)
    return types.SimpleNamespace(**f)


def fake_policy():
    from mycobotgym_amd.policy import pack
    return types.SimpleNamespace(obs_dim=D, act_dim=A, blob_floats=pack(ppo_sd(), D, A, (W,), (W,)).numel(), device=CPU, pi=(W,), vf=(W,))


def ppo_update(**kw):
    from mycobotgym_amd import PPOUpdate
    return PPOUpdate(fake_policy(), **kw)


def moments(n, **over):
    sd = {"m": torch.zeros(n), "v": torch.zeros(n), "step": 3}
    sd.update(over)
    return sd


def bare(cls, **attrs):
    """An object of ``cls`` with ``attrs`` and no constructor call: for the methods that refuse before they touch a device."""
    x = cls.__new__(cls)
    x.__dict__.update(attrs)
    return x


def no_device(cls, **dims):
    """``cls`` whose constructor resolves its dimensions (``dims`` where a case gives none) without loading the library: it gets as far
    as its own refusals."""
    class NoDevice(cls):
        def _resolve(self, envs, device, given):
            self.device = CPU
            return [given[k] for k, _ in self._FROM_ENVS]
    NoDevice.__name__ = cls.__name__
    return lambda **kw: NoDevice(**{**(dims or dict(num_envs=4, obs_dim=D, act_dim=A)), **kw})


def module(activation_fn=None, **seqs):
    """An ``nn.Module`` whose state dict has the Linear layers ``seqs``: dotted name with _ for . -> the (out, in) of its layers."""
    m = nn.Module()
    for path, layers in seqs.items():
        at, names = m, path.split("__")
        for n in names[:-1]:
            if not hasattr(at, n):
                setattr(at, n, nn.Module())
            at = getattr(at, n)
        mods = []
        for out, k in layers:
            mods += [nn.Linear(k, out), nn.ReLU()]
        setattr(at, names[-1], nn.Sequential(*mods[:-1]))
    if activation_fn is not None:
        m.activation_fn = activation_fn
    return m


def flagged(**flags):
    m = nn.Module()
    for k, v in flags.items():
        setattr(m, k, v)
    return m


def cnn_sd(channels=1, features=W, act=A, aliases=(), **over):
    """A CnnPolicy's state dict at S = 36 (o3 = 1), zeros; ``aliases``: the extractor under these further prefixes too."""
    sd = {"features_extractor.cnn.0.weight": torch.zeros(32, channels, 8, 8), "features_extractor.cnn.0.bias": torch.zeros(32),
          "features_extractor.cnn.2.weight": torch.zeros(64, 32, 4, 4), "features_extractor.cnn.2.bias": torch.zeros(64),
          "features_extractor.cnn.4.weight": torch.zeros(64, 64, 3, 3), "features_extractor.cnn.4.bias": torch.zeros(64),
          "features_extractor.linear.0.weight": torch.zeros(features, 64), "features_extractor.linear.0.bias": torch.zeros(features),
          "action_net.weight": torch.zeros(act, features), "action_net.bias": torch.zeros(act),
          "value_net.weight": torch.zeros(1, features), "value_net.bias": torch.zeros(1), "log_std": torch.zeros(act)}
    sd.update({a + k[len("features_extractor."):]: v.clone() for a in aliases for k, v in list(sd.items()) if k.startswith("features_extractor.")})
    sd.update(over)
    return sd


def holding(sd, **flags):
    """An ``nn.Module`` whose ``state_dict()`` is ``sd``, with ``flags`` as attributes."""
    m = flagged(**flags)
    m.state_dict = lambda: dict(sd)
    return m


def sac_module(activation_fn=None):
    q = [(W, D + 6 + A), (1, W)]
    return module(activation_fn, actor__latent_pi=[(W, D + 6), (W, W)], critic__qf0=q, critic__qf1=q)


def td3_module(activation_fn=None):
    return module(activation_fn, actor__mu=[(W, D + 6), (A, W)], critic__qf0=[(W, D + 6 + A), (1, W)])


# ----------------------------------------------------------------------------------------------------------------- cases
def cases():
    from mycobotgym_amd import ActorCritic, CnnActorCritic, DDPGUpdate, SACPolicy, SACUpdate, TD3Policy, TD3Update
    from mycobotgym_amd import cnn_policy as cp, policy, policy_update as pu, sac_policy as sp, sac_update as su, td3_policy as tp, td3_update as tu
    from mycobotgym_amd._offpolicy import check_common_hyper
    t = {}
    f64 = torch.float64

    # pack / pack_net / _param
    t["pack/weight-shape"] = lambda: policy.pack(ppo_sd(**{"action_net.weight": torch.zeros(A - 1, W)}), D, A, (W,), (W,))
    t["pack/bias-shape"] = lambda: policy.pack(ppo_sd(**{"mlp_extractor.value_net.0.bias": torch.zeros(W, 1)}), D, A, (W,), (W,))
    t["pack/log_std-shape"] = lambda: policy.pack(ppo_sd(log_std=torch.zeros(A, A)), D, A, (W,), (W,))
    t["pack/log_std-scalar"] = lambda: policy.pack(ppo_sd(log_std=0.0), D, A, (W,), (W,))
    t["pack_net/weight-shape"] = lambda: sp.pack_net({"a.weight": torch.zeros(3, 4), "a.bias": torch.zeros(W)}, [("a", W, 4, True)])
    t["pack_net/bias-shape"] = lambda: sp.pack_net({"a.weight": torch.zeros(W, 4), "a.bias": torch.zeros(3)}, [("a", W, 4, True)])
    t["pack_actor/sac"] = lambda: sp.pack_actor({"actor.latent_pi.0.weight": torch.zeros(W, D), "actor.latent_pi.0.bias": torch.zeros(W)}, D, A, (W,))
    t["pack_critic/sac"] = lambda: sp.pack_critic({"critic.qf0.0.weight": torch.zeros(W, D + 6), "critic.qf0.0.bias": torch.zeros(W)}, D, A, (W,))
    t["pack_critic/td3-target"] = lambda: tp.pack_critic({"critic_target.qf0.0.weight": torch.zeros(W, D + 6 + A), "critic_target.qf0.0.bias": torch.zeros(1)},
                                                         D, A, (W,), "critic_target", 1)
    t["pack_actor/td3"] = lambda: tp.pack_actor({"actor.mu.0.weight": torch.zeros(W, D + 6), "actor.mu.0.bias": torch.zeros(W),
                                                 "actor.mu.2.weight": torch.zeros(A, W + 1), "actor.mu.2.bias": torch.zeros(A)}, D, A, (W,))

    # minibatch_rows
    mr = lambda o, a: policy.minibatch_rows(o, a, D, A, "evaluate_actions")
    t["minibatch_rows/pictures"] = lambda: mr(torch.zeros(B, 3, 8, 8, dtype=torch.uint8), torch.zeros(B, A))
    t["minibatch_rows/missing-one"] = lambda: mr(without(obs(), "achieved_goal"), torch.zeros(B, A))
    t["minibatch_rows/missing-all"] = lambda: mr({}, torch.zeros(B, A))
    t["minibatch_rows/actions-none"] = lambda: mr(obs(), None)
    t["minibatch_rows/actions-columns"] = lambda: mr(obs(), torch.zeros(B, A - 1))
    t["minibatch_rows/actions-1d"] = lambda: mr(obs(), torch.zeros(B))
    t["minibatch_rows/empty"] = lambda: mr(obs(0), torch.zeros(0, A))
    t["minibatch_rows/observation-float64"] = lambda: mr(obs(observation=torch.zeros(B, D, dtype=f64)), torch.zeros(B, A))
    t["minibatch_rows/achieved-list"] = lambda: mr(obs(achieved_goal=[[0.0] * 3] * B), torch.zeros(B, A))
    t["minibatch_rows/actions-float64"] = lambda: mr(obs(), torch.zeros(B, A, dtype=f64))
    t["minibatch_rows/observation-columns"] = lambda: mr(obs(cols=D + 1), torch.zeros(B, A))
    t["minibatch_rows/desired-rows"] = lambda: mr(obs(desired_goal=torch.zeros(B - 1, 3)), torch.zeros(B, A))
    t["minibatch_rows/observation-rows"] = lambda: mr(obs(B + 1), torch.zeros(B, A))

    # batch_rows
    br = lambda o, a: sp.batch_rows(o, a, D, A, "q_values")
    t["batch_rows/pictures"] = lambda: br(torch.zeros(B, 3, 8, 8, dtype=torch.uint8), torch.zeros(B, A))
    t["batch_rows/missing-one"] = lambda: br(without(obs(), "desired_goal"), None)
    t["batch_rows/missing-all"] = lambda: br({}, None)
    t["batch_rows/empty"] = lambda: br(obs(0), None)
    t["batch_rows/observation-list"] = lambda: br(obs(observation=[[0.0] * D] * B), None)
    t["batch_rows/observation-0d"] = lambda: br(obs(observation=torch.zeros(())), None)
    t["batch_rows/observation-float64"] = lambda: br(obs(observation=torch.zeros(B, D, dtype=f64)), None)
    t["batch_rows/achieved-none"] = lambda: br(obs(achieved_goal=None), None)
    t["batch_rows/observation-columns"] = lambda: br(obs(cols=D - 1), None)
    t["batch_rows/achieved-rows"] = lambda: br(obs(achieved_goal=torch.zeros(B + 2, 3)), None)
    t["batch_rows/actions-columns"] = lambda: br(obs(), torch.zeros(B, A + 1))
    t["batch_rows/actions-rows"] = lambda: br(obs(), torch.zeros(B - 1, A))
    t["batch_rows/actions-float64"] = lambda: br(obs(), torch.zeros(B, A, dtype=f64))
    t["batch_rows/actions-list"] = lambda: br(obs(), [[0.0] * A] * B)
    t["batch_rows/who"] = lambda: sp.batch_rows({}, None, D, A, "td_target", CPU)

    # _per_row
    pr = lambda x: sp._per_row(x, B, "rewards", "td_target", None)
    t["_per_row/none"] = lambda: pr(None)
    t["_per_row/float64"] = lambda: pr(torch.zeros(B, dtype=f64))
    t["_per_row/bool"] = lambda: sp._per_row(torch.zeros(B, dtype=torch.bool), B, "dones", "SACUpdate", CPU)
    t["_per_row/two-columns"] = lambda: pr(torch.zeros(B, 2))
    t["_per_row/rows"] = lambda: pr(torch.zeros(B - 1))
    t["_per_row/row-vector"] = lambda: pr(torch.zeros(1, B))

    # check_out
    shapes = {"action": (4, A), "log_prob": (4,), "mean": (4, A)}
    co = lambda out: sp.check_out(out, shapes, "action", "forward", CPU)
    t["check_out/no-dict"] = lambda: co(torch.zeros(4, A))
    t["check_out/required"] = lambda: co({"mean": torch.zeros(4, A)})
    t["check_out/unknown"] = lambda: co({"action": torch.zeros(4, A), "value": torch.zeros(4), "entropy": torch.zeros(4)})
    t["check_out/float64"] = lambda: co({"action": torch.zeros(4, A, dtype=f64)})
    t["check_out/shape"] = lambda: co({"action": torch.zeros(4, A), "log_prob": torch.zeros(4, 1)})
    t["check_out/strided"] = lambda: co({"action": torch.zeros(A, 4).T})
    t["check_out/list"] = lambda: co({"action": [0.0]})
    t["check_out/td3"] = lambda: tp.check_out({}, {"target": (B,)}, "target", "td_target")

    # check_minibatch
    cm = lambda mb, need_old=True: pu.check_minibatch(mb, D, A, need_old)
    t["check_minibatch/no-field"] = lambda: cm((1, 2, 3))
    t["check_minibatch/no-returns"] = lambda: cm(types.SimpleNamespace(observations=obs(), actions=torch.zeros(B, A), old_log_prob=None, advantages=None))
    t["check_minibatch/pictures"] = lambda: cm(samples(observations=torch.zeros(B, D)))
    t["check_minibatch/advantages-rows"] = lambda: cm(samples(advantages=torch.zeros(B - 1)))
    t["check_minibatch/advantages-column"] = lambda: cm(samples(advantages=torch.zeros(B, 1)))
    t["check_minibatch/returns-float64"] = lambda: cm(samples(returns=torch.zeros(B, dtype=f64)))
    t["check_minibatch/returns-list"] = lambda: cm(samples(returns=[0.0] * B), False)
    t["check_minibatch/old_log_prob-float64"] = lambda: cm(samples(old_log_prob=torch.zeros(B, dtype=f64)))
    t["check_minibatch/old_log_prob-none"] = lambda: cm(samples(old_log_prob=None))
    t["check_minibatch/who"] = lambda: pu.check_minibatch(samples(advantages=torch.zeros(1)), D, A, False, "A2C")
    def set_between_steps(**attrs):
        opt = ppo_update()
        opt.__dict__.update(attrs)
        return opt
    t["compute_grad/clip_range"] = lambda: set_between_steps(clip_range=-0.1).compute_grad(samples())
    t["compute_grad/advantages"] = lambda: ppo_update().compute_grad(samples(advantages=torch.zeros(B + 1)))
    t["compute_grad/old_log_prob"] = lambda: ppo_update().compute_grad(samples(old_log_prob=torch.zeros(B, 1)))
    t["compute_grad/observations"] = lambda: ppo_update(loss="a2c").compute_grad(samples(observations=without(obs(), "observation")))

    # check_batch
    cb = lambda b: su.check_batch(b, D, A)
    t["check_batch/no-field"] = lambda: cb((1, 2, 3))
    t["check_batch/no-rewards"] = lambda: cb(types.SimpleNamespace(observations=obs(), actions=None, next_observations=obs(), dones=None))
    t["check_batch/observations"] = lambda: cb(replay(observations=obs(cols=D + 2)))
    t["check_batch/actions"] = lambda: cb(replay(actions=torch.zeros(B, A - 1)))
    t["check_batch/actions-none"] = lambda: cb(replay(actions=None, rewards=torch.zeros(B, 3)))
    t["check_batch/next-missing"] = lambda: cb(replay(next_observations=without(obs(), "observation")))
    t["check_batch/next-rows"] = lambda: cb(replay(next_observations=obs(B + 1)))
    t["check_batch/rewards"] = lambda: cb(replay(rewards=torch.zeros(B, dtype=f64)))
    t["check_batch/dones"] = lambda: cb(replay(dones=torch.zeros(B, 2)))
    t["check_batch/who"] = lambda: su.check_batch(replay(next_observations=obs(1)), D, A, CPU, "DDPGUpdate")

    # policy_update.check_hyper
    ph = lambda loss="ppo", clip_range=0.2, betas=(0.9, 0.999), **unbuilt: pu.check_hyper(loss, clip_range, betas, unbuilt)
    t["ppo-hyper/clip_range_vf"] = lambda: ph(clip_range_vf=0.2)
    t["ppo-hyper/target_kl"] = lambda: ph(target_kl=0.01)
    t["ppo-hyper/unexpected"] = lambda: ph(momentum=0.9)
    t["ppo-hyper/loss"] = lambda: ph(loss="trpo")
    t["ppo-hyper/clip_range-zero"] = lambda: ph(clip_range=0.0)
    t["ppo-hyper/clip_range-nan"] = lambda: ph(clip_range=float("nan"))
    t["ppo-hyper/betas-one"] = lambda: ph(betas=(0.9, 1.0))
    t["ppo-hyper/betas-three"] = lambda: ph(betas=(0.9, 0.99, 0.999))
    t["ppo-hyper/constructor"] = lambda: ppo_update(loss="a2c", target_kl=None)

    # sac_update.check_hyper and check_common_hyper through it
    def sh(**kw):
        a = dict(learning_rate=3e-4, gamma=0.99, tau=0.005, ent_coef="auto", target_entropy="auto", target_update_interval=1, betas=(0.9, 0.999), eps=1e-8)
        unbuilt = {k: kw.pop(k) for k in list(kw) if k not in a}
        a.update(kw)
        return su.check_hyper(unbuilt=unbuilt, **a)
    t["sac-hyper/interval-zero"] = lambda: sh(target_update_interval=0)
    t["sac-hyper/interval-bool"] = lambda: sh(target_update_interval=True)
    t["sac-hyper/interval-fraction"] = lambda: sh(target_update_interval=1.5)
    t["sac-hyper/target_entropy-word"] = lambda: sh(target_entropy="low")
    t["sac-hyper/target_entropy-nan"] = lambda: sh(target_entropy=float("nan"))
    t["sac-hyper/auto-word"] = lambda: sh(ent_coef="auto_x")
    t["sac-hyper/auto-negative"] = lambda: sh(ent_coef="auto_-1")
    t["sac-hyper/auto-inf"] = lambda: sh(ent_coef="auto_inf")
    t["sac-hyper/ent_coef-word"] = lambda: sh(ent_coef="fixed")
    t["sac-hyper/ent_coef-negative"] = lambda: sh(ent_coef=-0.1)
    t["sac-hyper/ent_coef-bool"] = lambda: sh(ent_coef=True)
    t["sac-hyper/ent_coef-none"] = lambda: sh(ent_coef=None)
    t["sac-hyper/use_sde"] = lambda: sh(use_sde=True)
    t["sac-hyper/sde_sample_freq"] = lambda: sh(use_sde=False, sde_sample_freq=4)
    t["sac-hyper/max_grad_norm"] = lambda: sh(max_grad_norm=0.5)
    t["sac-hyper/n_critics"] = lambda: sh(n_critics=3)
    t["sac-hyper/action_noise"] = lambda: sh(action_noise=None)
    t["sac-hyper/optimizer_class"] = lambda: sh(optimizer_class="SGD")
    t["sac-hyper/optimizer_kwargs"] = lambda: sh(optimizer_kwargs={})
    t["sac-hyper/unexpected"] = lambda: sh(train_freq=1)
    t["sac-hyper/schedule"] = lambda: sh(learning_rate=abs)
    t["sac-hyper/learning_rate-zero"] = lambda: sh(learning_rate=0.0)
    t["sac-hyper/learning_rate-inf"] = lambda: sh(learning_rate=float("inf"))
    t["sac-hyper/learning_rate-word"] = lambda: sh(learning_rate="3e-4")
    t["sac-hyper/gamma"] = lambda: sh(gamma=1.5)
    t["sac-hyper/tau-zero"] = lambda: sh(tau=0)
    t["sac-hyper/tau-bool"] = lambda: sh(tau=True)
    t["sac-hyper/betas-one"] = lambda: sh(betas=(0.9, 1.0))
    t["sac-hyper/betas-single"] = lambda: sh(betas=(0.9,))
    t["sac-hyper/eps"] = lambda: sh(eps=-1e-8)
    t["sac-hyper/constructor"] = lambda: SACUpdate(types.SimpleNamespace(), gamma=-0.1)
    t["sac-update/needs-a-policy"] = lambda: SACUpdate(types.SimpleNamespace())
    t["common-hyper/who"] = lambda: check_common_hyper(1e-3, 0.99, 0.005, (0.9, 0.999), 1e-8, {"n_steps": 5}, {}, "why", "SomeUpdate")
    t["common-hyper/refused"] = lambda: check_common_hyper(1e-3, 0.99, 0.005, (0.9, 0.999), 1e-8, {"x": 1}, {"x": "x is not built"}, "why", "SomeUpdate")
    t["common-hyper/sde"] = lambda: check_common_hyper(1e-3, 0.99, 0.005, (0.9, 0.999), 1e-8, {"use_sde_at_warmup": True}, {}, "the reason", "SomeUpdate")

    # td3_update.check_hyper
    def th(who="TD3Update", **kw):
        a = dict(learning_rate=1e-3, gamma=0.99, tau=0.005, policy_delay=2, target_policy_noise=0.2, target_noise_clip=0.5, betas=(0.9, 0.999), eps=1e-8)
        unbuilt = {k: kw.pop(k) for k in list(kw) if k not in a}
        a.update(kw)
        return tu.check_hyper(unbuilt=unbuilt, who=who, **a)
    t["td3-hyper/policy_delay-zero"] = lambda: th(policy_delay=0)
    t["td3-hyper/policy_delay-fraction"] = lambda: th(policy_delay=1.5)
    t["td3-hyper/policy_delay-bool"] = lambda: th(policy_delay=True)
    t["td3-hyper/policy_delay-nan"] = lambda: th(policy_delay=float("nan"))
    t["td3-hyper/target_policy_noise"] = lambda: th(target_policy_noise=-0.2)
    t["td3-hyper/target_noise_clip"] = lambda: th(target_noise_clip=float("inf"))
    t["td3-hyper/use_sde"] = lambda: th(use_sde=True)
    t["td3-hyper/n_critics"] = lambda: th(n_critics=2)
    t["td3-hyper/action_noise"] = lambda: th(action_noise="ou")
    t["td3-hyper/unexpected"] = lambda: th(who="DDPGUpdate", ent_coef="auto")
    t["td3-hyper/gamma"] = lambda: th(gamma=float("nan"))
    t["td3-hyper/constructor"] = lambda: DDPGUpdate(types.SimpleNamespace(), train_freq=1)
    t["td3-update/needs-a-policy"] = lambda: TD3Update(types.SimpleNamespace())
    t["ddpg-update/needs-a-policy"] = lambda: DDPGUpdate(types.SimpleNamespace(_t={"actor": 0}))

    # the three _refuse_foreign, and td3_policy._refuse_widths
    t["ppo-foreign/shared"] = lambda: policy._refuse_foreign(["mlp_extractor.shared_net.0.weight"])
    t["ppo-foreign/cnn"] = lambda: policy._refuse_foreign(["features_extractor.cnn.0.weight"])
    t["ppo-foreign/extractor"] = lambda: policy._refuse_foreign({"pi_features_extractor.linear.weight": 0})
    t["sac-foreign/cnn"] = lambda: sp._refuse_foreign(["actor.features_extractor.extractors.image.CNN.0.weight"])
    t["sac-foreign/extractor"] = lambda: sp._refuse_foreign(["critic.features_extractor.linear.weight", "critic.qf1.0.weight"])
    t["sac-foreign/three-critics"] = lambda: sp._refuse_foreign(["critic.qf1.0.weight", "critic.qf2.0.weight"])
    t["sac-foreign/one-critic"] = lambda: sp._refuse_foreign(["critic.qf0.0.weight"])
    t["sac-foreign/sde"] = lambda: sp._refuse_foreign(["critic.qf1.0.weight", "actor.log_std"])
    t["td3-foreign/cnn"] = lambda: tp._refuse_foreign(["actor.features_extractor.cnn.0.weight"])
    t["td3-foreign/extractor"] = lambda: tp._refuse_foreign(["actor.features_extractor.linear.weight"])
    t["td3-foreign/three-critics"] = lambda: tp._refuse_foreign(["critic_target.qf2.0.weight"])
    t["td3-foreign/sde"] = lambda: tp._refuse_foreign(["actor.log_std.weight"])
    t["td3-widths"] = lambda: tp._refuse_widths((400, 300))

    # PPOUpdate.load_state_dict on a fake policy
    n = fake_policy().blob_floats
    t["ppo-load/empty"] = lambda: ppo_update().load_state_dict({})
    t["ppo-load/no-v"] = lambda: ppo_update().load_state_dict({"m": torch.zeros(n), "step": 1})
    t["ppo-load/m-float64"] = lambda: ppo_update().load_state_dict(moments(n, m=torch.zeros(n, dtype=f64)))
    t["ppo-load/v-shape"] = lambda: ppo_update().load_state_dict(moments(n, v=torch.zeros(n + 16)))
    t["ppo-load/m-2d"] = lambda: ppo_update().load_state_dict(moments(n, m=torch.zeros(1, n)))
    t["ppo-load/exp_avg-misfit"] = lambda: ppo_update().load_state_dict({"exp_avg": ppo_sd(**{"value_net.weight": torch.zeros(2, W)}), "v": torch.zeros(n), "step": 1})
    t["ppo-load/exp_avg_sq-log_std"] = lambda: ppo_update().load_state_dict({"m": torch.zeros(n), "exp_avg_sq": ppo_sd(log_std=torch.zeros(1, A)), "step": 1})
    t["ppo-load/loss"] = lambda: ppo_update().load_state_dict(moments(n, loss="trpo"))
    t["ppo-load/betas"] = lambda: ppo_update().load_state_dict(moments(n, betas=(1.0, 0.5)))

    # the off-policy updaters' moments, the step's own checks
    def offpolicy_update(cls, **more):
        pol = types.SimpleNamespace(obs_dim=D, act_dim=A, pi=(W,), qf=(W,), n_critics=2, device=CPU)
        z = lambda: {"critic": torch.zeros(32), "actor": torch.zeros(16), **more}
        return bare(cls, policy=pol, m=z(), v=z(), steps=0, learning_rate=1e-3)
    t["sac-load/empty"] = lambda: offpolicy_update(SACUpdate).load_state_dict({})
    t["sac-load/m-shape"] = lambda: offpolicy_update(SACUpdate).load_state_dict({"m": {"critic": torch.zeros(32), "actor": torch.zeros(17)}, "v": {}})
    t["td3-load/no-v"] = lambda: offpolicy_update(TD3Update).load_state_dict({"m": {"critic": torch.zeros(32), "actor": torch.zeros(16)}})
    t["td3-load/v-float64"] = lambda: offpolicy_update(TD3Update).load_state_dict({"m": {"critic": torch.zeros(32), "actor": torch.zeros(16)},
                                                                                    "v": {"critic": torch.zeros(32, dtype=f64), "actor": torch.zeros(16)}})
    t["td3-load/exp_avg-misfit"] = lambda: offpolicy_update(TD3Update).load_state_dict({"exp_avg": {"critic.qf0.0.weight": torch.zeros(W, D), "critic.qf0.0.bias": torch.zeros(W)}})
    t["sac-step/learning_rate"] = lambda: bare(SACUpdate, policy=types.SimpleNamespace(), learning_rate=0.0)._inputs(replay())
    t["td3-step/learning_rate"] = lambda: bare(TD3Update, policy=types.SimpleNamespace(), learning_rate=float("inf"))._inputs(replay())
    t["ddpg-step/batch"] = lambda: offpolicy_update(DDPGUpdate)._inputs(replay(dones=None))
    t["sac-step/out-empty"] = lambda: offpolicy_update(SACUpdate)._check_out({}, B)
    t["td3-step/out-tensor"] = lambda: offpolicy_update(TD3Update)._check_out(torch.zeros(B), B)
    t["td3-step/out-unknown"] = lambda: offpolicy_update(TD3Update)._check_out({"noise": torch.zeros(B, A)}, B)
    t["sac-step/out-shape"] = lambda: offpolicy_update(SACUpdate)._check_out({"q_pi": torch.zeros(B, 2)}, B)

    # from_module, up to the constructor
    t["ppo-module/use_sde"] = lambda: ActorCritic.from_module(flagged(use_sde=True))
    t["ppo-module/squash_output"] = lambda: ActorCritic.from_module(flagged(squash_output=True))
    t["ppo-module/shared"] = lambda: ActorCritic.from_module(module(mlp_extractor__shared_net=[(W, D + 6)]))
    t["ppo-module/activation_fn-class"] = lambda: ActorCritic.from_module(flagged(activation_fn=nn.ELU))
    t["ppo-module/activation_fn-function"] = lambda: ActorCritic.from_module(flagged(activation_fn=torch.sigmoid))
    t["ppo-module/no-layers"] = lambda: ActorCritic.from_module(flagged(activation_fn=nn.Tanh))
    t["ppo-module/no-value-net"] = lambda: ActorCritic.from_module(module(mlp_extractor__policy_net=[(W, D + 6)]), activation="elu")
    t["sac-module/use_sde"] = lambda: SACPolicy.from_module(flagged(actor=flagged(use_sde=True)))
    t["sac-module/n_critics"] = lambda: SACPolicy.from_module(flagged(critic=flagged(n_critics=3)))
    t["sac-module/one-critic"] = lambda: SACPolicy.from_module(module(critic__qf0=[(1, W)]))
    t["sac-module/no-layers"] = lambda: SACPolicy.from_module(module(critic__qf1=[(1, W)]))
    t["sac-module/activation_fn"] = lambda: SACPolicy.from_module(sac_module(nn.LeakyReLU))
    t["td3-module/use_sde"] = lambda: TD3Policy.from_module(flagged(use_sde=True))
    t["td3-module/no-layers"] = lambda: TD3Policy.from_module(nn.Module())
    t["td3-module/head-only"] = lambda: TD3Policy.from_module(module(actor__mu=[(A, D + 6)], critic__qf0=[(W, D + 6 + A), (1, W)]))
    t["td3-module/activation_fn"] = lambda: TD3Policy.from_module(td3_module(nn.GELU))

    # the constructors, up to their first use of the library
    for name, cls, other in (("ppo", ActorCritic, "qf"), ("sac", SACPolicy, "vf"), ("td3", TD3Policy, "vf")):
        new = no_device(cls)
        t[name + "-new/hidden-keys"] = lambda new=new, other=other: new(hidden={"pi": [W], other: [W]})
        t[name + "-new/hidden-one-key"] = lambda new=new: new(hidden={"pi": [W]})
        t[name + "-new/activation"] = lambda new=new: new(hidden=(W,), activation="elu")
        t[name + "-new/four-layers"] = lambda new=new: new(hidden=(W, 32, 48, 64), activation="tanh")
        t[name + "-new/four-layer-critic"] = lambda new=new, own="vf" if cls is ActorCritic else "qf": new(hidden={"pi": (W,), own: (W,) * 4})
    t["sac-new/use_sde"] = lambda: no_device(SACPolicy)(use_sde=True)
    t["sac-new/n_critics"] = lambda: no_device(SACPolicy)(n_critics=1)
    t["td3-new/use_sde"] = lambda: no_device(TD3Policy)(use_sde=True)
    t["td3-new/n_critics"] = lambda: no_device(TD3Policy)(n_critics=3)
    t["td3-new/n_critics-bool"] = lambda: no_device(TD3Policy)(n_critics=True)
    t["td3-new/default-net_arch"] = lambda: no_device(TD3Policy)(hidden=(400, 300))
    t["td3-new/default-net_arch-critic"] = lambda: no_device(TD3Policy)(hidden={"pi": (256, 256), "qf": [400, 300]})
    t["ppo-new/no-dimensions"] = lambda: ActorCritic(num_envs=4)
    t["sac-new/no-dimensions"] = lambda: SACPolicy(obs_dim=D)
    t["td3-new/no-dimensions"] = lambda: TD3Policy()

    # load_state_dict, up to the repacking
    ppo = lambda: bare(ActorCritic, obs_dim=D, act_dim=A, pi=(W,), vf=(W,), device=CPU, seed=0, calls=0, _blob=torch.zeros(1))
    blobs = lambda *names: {k: torch.zeros(1) for k in names}
    sac = lambda: bare(SACPolicy, obs_dim=D, act_dim=A, pi=(W,), qf=(W, W), device=CPU, seed=0, calls=0, target_calls=0,
                       _t=blobs("actor", "critic", "critic_target", "log_ent_coef"))
    td3 = lambda nc: bare(TD3Policy, obs_dim=D, act_dim=A, pi=(W, W), qf=(W,), n_critics=nc, device=CPU, seed=0, calls=0, target_calls=0,
                          _t=blobs("actor", "actor_target", "critic", "critic_target"))
    t["ppo-load_state_dict/missing"] = lambda: ppo().load_state_dict(without(ppo_sd(seed=3, calls=9), "log_std"))
    t["ppo-load_state_dict/extra"] = lambda: ppo().load_state_dict(ppo_sd(**{"mlp_extractor.policy_net.2.weight": 0, "mlp_extractor.policy_net.2.bias": 0}))
    t["ppo-load_state_dict/foreign"] = lambda: ppo().load_state_dict(ppo_sd(**{"features_extractor.linear.weight": 0}))
    t["ppo-load_state_dict/shape"] = lambda: ppo().load_state_dict(ppo_sd(**{"value_net.bias": torch.zeros(2)}))
    t["sac-load_state_dict/empty"] = lambda: sac().load_state_dict({"critic.qf1.0.weight": 0, "log_ent_coef": 0.0, "target_calls": 2})
    t["sac-load_state_dict/foreign"] = lambda: sac().load_state_dict({"critic.qf0.0.weight": 0})
    t["td3-load_state_dict/empty"] = lambda: td3(2).load_state_dict({"seed": 1, "optimizer": 0})
    t["ddpg-load_state_dict/second-critic"] = lambda: td3(1).load_state_dict({"critic.qf1.0.weight": 0, "critic.qf1.0.bias": 0})
    t["td3-load_state_dict/foreign"] = lambda: td3(2).load_state_dict({"actor.log_std.bias": 0})
    # cnn_policy.py: _flat, _refuse_foreign, the constructor, load_state_dict, from_module, _pictures, evaluate_actions, forward's out
    S, u8 = 36, torch.uint8
    PI, VF = "pi_features_extractor.", "vf_features_extractor."
    t["cnn-flat/conv1-channels"] = lambda: cp._flat(cnn_sd(channels=2), 1)
    t["cnn-flat/conv3-flattened"] = lambda: cp._flat(cnn_sd(**{"features_extractor.cnn.4.weight": torch.zeros(64, 576)}), 1)
    t["cnn-pack/linear-shape"] = lambda: cp.pack(cnn_sd(), 1, 64, W, A)
    t["cnn-foreign/net_arch"] = lambda: cp._refuse_foreign(cnn_sd(**{"mlp_extractor.policy_net.0.weight": torch.zeros(W, W)}))
    t["cnn-foreign/alias-alone"] = lambda: cp._refuse_foreign({PI + "cnn.0.bias": torch.zeros(32)})
    t["cnn-foreign/alias-shape"] = lambda: cp._refuse_foreign(cnn_sd(aliases=(PI,), **{PI + "cnn.2.bias": torch.zeros(32)}))
    t["cnn-foreign/alias-differs"] = lambda: cp._refuse_foreign(cnn_sd(aliases=(PI, VF), **{VF + "linear.0.bias": torch.ones(W)}))
    cnn_new = no_device(CnnActorCritic, num_envs=4, channels=1, image_size=S, act_dim=A)
    t["cnn-new/num_envs"] = lambda: cnn_new(num_envs=0)
    t["cnn-new/channels"] = lambda: cnn_new(channels=17)
    t["cnn-new/image_size-small"] = lambda: cnn_new(image_size=35)
    t["cnn-new/image_size-large"] = lambda: cnn_new(image_size=97)
    t["cnn-new/features_dim-multiple"] = lambda: cnn_new(features_dim=24)
    t["cnn-new/features_dim-large"] = lambda: cnn_new(features_dim=528)
    t["cnn-new/act_dim"] = lambda: cnn_new(act_dim=17, seed=3)
    t["cnn-new/no-dimensions"] = lambda: CnnActorCritic(num_envs=4, image_size=S)
    cnn = lambda **more: bare(CnnActorCritic, **{**dict(num_envs=4, channels=1, image_size=S, features_dim=W, act_dim=A, device=CPU, seed=0,
                                                        calls=0, _blob=torch.zeros(1)), **more})
    t["cnn-load_state_dict/missing"] = lambda: cnn().load_state_dict(without(cnn_sd(seed=3, calls=9), "log_std"))
    t["cnn-load_state_dict/extra"] = lambda: cnn().load_state_dict(cnn_sd(**{"features_extractor.cnn.6.weight": 0, "optimizer": 0}))
    t["cnn-load_state_dict/net_arch"] = lambda: cnn().load_state_dict(cnn_sd(**{"mlp_extractor.value_net.0.bias": 0}))
    t["cnn-load_state_dict/alias-differs"] = lambda: cnn().load_state_dict(cnn_sd(aliases=(PI, VF), **{PI + "cnn.0.bias": torch.ones(32)}))
    t["cnn-load_state_dict/alias-missing"] = lambda: cnn().load_state_dict(without(cnn_sd(aliases=(PI,)), "features_extractor.cnn.4.bias"))
    t["cnn-load_state_dict/conv-shape"] = lambda: cnn().load_state_dict(cnn_sd(**{"features_extractor.cnn.2.weight": torch.zeros(64, 512)}))
    t["cnn-load_state_dict/head-shape"] = lambda: cnn().load_state_dict(cnn_sd(**{"action_net.weight": torch.zeros(A, W + 16)}))
    t["cnn-load_state_dict/log_std-shape"] = lambda: cnn().load_state_dict(cnn_sd(log_std=torch.zeros(A, A)))
    t["cnn-module/use_sde"] = lambda: CnnActorCritic.from_module(flagged(use_sde=True))
    t["cnn-module/squash_output"] = lambda: CnnActorCritic.from_module(flagged(squash_output=True))
    t["cnn-module/separate-extractors"] = lambda: CnnActorCritic.from_module(flagged(share_features_extractor=False))
    t["cnn-module/net_arch"] = lambda: CnnActorCritic.from_module(holding(cnn_sd(**{"mlp_extractor.policy_net.0.weight": torch.zeros(W, W)})))
    t["cnn-module/alias-differs"] = lambda: CnnActorCritic.from_module(holding(cnn_sd(aliases=(PI, VF), **{VF + "cnn.4.bias": torch.ones(64)})))
    t["cnn-module/no-linear"] = lambda: CnnActorCritic.from_module(nn.Linear(4, 4))
    t["cnn-module/no-dimensions"] = lambda: CnnActorCritic.from_module(holding(cnn_sd(aliases=(PI, VF))), num_envs=4)
    pics = lambda img, rows=B, dtypes=(u8,), **more: cnn(**more)._pictures(img, "forward: img", rows, dtypes)
    t["cnn-pictures/list"] = lambda: pics([[0]])
    t["cnn-pictures/dict"] = lambda: pics(obs(), dtypes=(u8, torch.float32))
    t["cnn-pictures/float32"] = lambda: pics(torch.zeros(B, 1, S, S))
    t["cnn-pictures/float64"] = lambda: pics(torch.zeros(B, 1, S, S, dtype=f64), dtypes=(u8, torch.float32))
    t["cnn-pictures/channels"] = lambda: pics(torch.zeros(B, 2, S, S, dtype=u8))
    t["cnn-pictures/rows"] = lambda: pics(torch.zeros(B - 1, 1, S, S, dtype=u8))
    t["cnn-pictures/channels-last"] = lambda: pics(torch.zeros(B, S, S, 2, dtype=u8), channels=2)
    img = lambda rows=B, dtype=torch.float32: torch.zeros(rows, 1, S, S, dtype=dtype)
    ev = lambda o, a, **kw: cnn().evaluate_actions(o, a, **kw)
    t["cnn-evaluate/state-dict"] = lambda: ev(obs(), torch.zeros(B, A))
    t["cnn-evaluate/actions-none"] = lambda: ev(img(), None)
    t["cnn-evaluate/actions-1d"] = lambda: ev(img(), torch.zeros(B))
    t["cnn-evaluate/actions-columns"] = lambda: ev(img(), torch.zeros(B, A - 1))
    t["cnn-evaluate/actions-float64"] = lambda: ev(img(), torch.zeros(B, A, dtype=f64))
    t["cnn-evaluate/empty"] = lambda: ev(img(0), torch.zeros(0, A))
    t["cnn-evaluate/observations-list"] = lambda: ev([0], torch.zeros(B, A))
    t["cnn-evaluate/observations-int32"] = lambda: ev(img(dtype=torch.int32), torch.zeros(B, A))
    t["cnn-evaluate/observations-rows"] = lambda: ev(img(B + 1, u8), torch.zeros(B, A))
    t["cnn-evaluate/out-tensor"] = lambda: ev(img(), torch.zeros(B, A), out=torch.zeros(B))
    t["cnn-evaluate/out-empty"] = lambda: ev(img(dtype=u8), torch.zeros(B, A), out={})
    t["cnn-evaluate/out-unknown"] = lambda: ev(img(), torch.zeros(B, A), out={"value": torch.zeros(B), "action": torch.zeros(B, A)})
    t["cnn-evaluate/out-shape"] = lambda: ev(img(), torch.zeros(B, A), out={"entropy": torch.zeros(B, 1)})
    t["cnn-evaluate/out-float64"] = lambda: ev(img(), torch.zeros(B, A), out={"log_prob": torch.zeros(B, dtype=f64)})
    fw = lambda out: cnn().forward(None, out=out)
    t["cnn-forward/out-tensor"] = lambda: fw(torch.zeros(4, A))
    t["cnn-forward/out-empty"] = lambda: fw({})
    t["cnn-forward/out-unknown"] = lambda: fw({"action": torch.zeros(4, A), "entropy": torch.zeros(4)})
    t["cnn-forward/out-features-shape"] = lambda: fw({"features": torch.zeros(4, W + 16)})
    t["cnn-forward/out-strided"] = lambda: fw({"mean": torch.zeros(A, 4).T})
    t["cnn-forward/out-list"] = lambda: fw({"value": [0.0] * 4})
    t["cnn-values/out-shape"] = lambda: cnn().values(None, out=torch.zeros(4, 1))
    t["cnn-values/out-float64"] = lambda: cnn().values(None, out=torch.zeros(4, dtype=f64))
    return t


def raised(case):
    try:
        case()
    except Exception as e:                # (any type: the type is what the fixture pins)
        return [type(e).__name__, str(e)]
    return ["no exception", ""]


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


NAMES = sorted(golden()) if os.path.exists(GOLDEN) else []


def test_the_fixture_lists_the_table():
    assert NAMES == sorted(cases()) and NAMES


@pytest.fixture(scope="module")
def table():
    return cases(), golden()


@pytest.mark.parametrize("name", NAMES)
def test_refusal(table, name):
    cs, want = table
    got = raised(cs[name])
    assert got[0] not in ("no exception", "AttributeError", "NameError", "KeyError"), got      # a refusal, not an accident of the case
    assert got == want[name]


if __name__ == "__main__":
    out = {name: raised(case) for name, case in sorted(cases().items())}
    for name, (kind, text) in out.items():
        print(f"{name:44s} {kind:12s} {text[:150]}")
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(len(out), "cases ->", GOLDEN)
