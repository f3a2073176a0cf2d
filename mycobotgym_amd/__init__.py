"""mycobotgym_amd -- MI355X-native vectorised rollout engine for the MyCobotGym step()/reset() hot path.

    from mycobotgym_amd import make
    envs = make("MyCobotReach-Dense-joint-v0", num_envs=8192, device="cuda:0")
    obs, info = envs.reset(seed=0)
    obs, reward, terminated, truncated, info = envs.step(actions)     # torch tensors on the GPU

The numeric path is the HIP library ``libmycobot_hip.so`` (C ABI in ``include/mcg.h``); importing the
package does not need a GPU, constructing an environment does.
"""
from .cnn_policy import CnnActorCritic  # noqa: F401
from .frame_stack import FrameStack  # noqa: F401
from .policy import ActorCritic  # noqa: F401
from .policy_update import PPOUpdate  # noqa: F401
from .sac_policy import SACPolicy  # noqa: F401
from .sac_update import SACUpdate  # noqa: F401
from .td3_policy import DDPGPolicy, TD3Policy  # noqa: F401
from .td3_update import DDPGUpdate, TD3Update  # noqa: F401
from .registry import REGISTRY, spec  # noqa: F401
from .replay import HerBuffer, HerSamples  # noqa: F401
from .replay_img import ImageReplayBuffer, ReplaySamples  # noqa: F401
from .rollout import RolloutBuffer, RolloutSamples  # noqa: F401
from .rollout_img import ImageRolloutBuffer  # noqa: F401
from .vec_env import MyCobotImgVecEnv, MyCobotVecEnv, env_class, load_scene, make, validate_scenes  # noqa: F401

__version__ = "0.1.0"
