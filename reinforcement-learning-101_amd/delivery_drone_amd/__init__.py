"""MI355X-native vectorised delivery-drone environment.

The per-frame step of vedant-jumle/reinforcement-learning-101's
``delivery_drone/game`` (physics, reward, termination) as HIP kernels for
gfx950 behind a C ABI (``include/dronestep.h``), with a gym-style batched
surface (:class:`VecDroneEnv`) and the reference's per-game APIs
(:class:`DroneGameClient`, :class:`DroneGame`) on top; the notebooks'
policy / value networks (:class:`MlpNet`, f32 MFMA) and GAE (:func:`gae`)
for on-device collection, and the notebooks' ``evaluate_policy`` (temperature
or greedy action selection, one episode per lane:
:meth:`VecDroneEnv.evaluate_policy`, with ``calc_reward``'s components kept
per lane and per frame on request: :func:`notebook_rewards`); and the
notebooks' training batches
built from rollout buffers on device (:func:`ppo_batch`,
:func:`reinforce_batch`, :func:`collect_ppo`), from each lane's first
episode or from every episode of an auto-reset rollout
(:func:`ppo_episodes_batch`, :func:`reinforce_episodes_batch`,
:func:`collect_ppo_steps`); and the PPO notebook's losses, ratio statistics and
head gradients on such a batch (:func:`ppo_losses`,
:meth:`MlpNet.evaluate_actions`, :meth:`MlpNet.load_state_dict`) and the two
networks' parameter gradients from them (:func:`ppo_grads`,
:meth:`MlpNet.backward`); and the notebook's two AdamW steps and its whole
epoch loop on device (:class:`AdamW`, :func:`ppo_update`,
:meth:`MlpNet.flat_parameters`), full-batch or in shuffled minibatches
(:func:`shuffle_batch`, :func:`shuffle_indices`: a keyed permutation computed
on device); and the other two training notebooks'
learners: REINFORCE (:func:`collect_reinforce`, :func:`reinforce_losses`,
:func:`reinforce_update`) and the one-step TD actor-critic
(:func:`td_losses`, :func:`actor_critic_update`); and several actors in one
fused launch, each on its own group of lanes (:class:`ActorPopulation`,
:func:`population_summary`: a checkpoint tournament or a sweep's collection),
and a sweep's learners updated in one fused launch (:class:`LearnerPopulation`,
:func:`collect_ppo_population`, :func:`ppo_update_population`), and the
one-step actor-critic loop itself, frame by frame, in one launch
(:func:`actor_critic_train`, :func:`actor_critic_train_population`), and
one whole REINFORCE iteration in one launch (:class:`ReinforcePopulation`,
:func:`reinforce_train`, :func:`reinforce_train_population`), and one whole
PPO iteration in one launch (:func:`ppo_train`, :func:`ppo_train_population`,
:func:`ppo_iteration_data`);
and the frames of ``DroneGame.render`` (:meth:`VecDroneEnv.render`) and the
labelled grid of ``--render-all`` (:meth:`VecDroneEnv.render_grid`,
:func:`grid_shape`).
"""
from .config import EnvConfig
from .vec_env import OBS_KEYS, StepInfo, VecDroneEnv, grid_shape
from .compat import DroneGame, DroneGameClient, DroneState, action_bits
from .sharding import dist_env, gather_obs, shard_bounds
from .gae import gae
from .policy import ActorPopulation, MlpNet, population_summary
from .train_batch import collect_ppo, ppo_batch, reinforce_batch
from .train_batch import collect_ppo_steps, ppo_episodes_batch, reinforce_episodes_batch
from .ppo_loss import PpoLosses, ppo_losses
from .ppo_grad import PpoGrads, ppo_grads
from .shuffle import ShuffledBatch, shuffle_batch, shuffle_indices
from .adamw import AdamW, PpoUpdate, ppo_update
from .pg_loss import ReinforceLosses, ReinforceUpdate, collect_reinforce, reinforce_losses, reinforce_update
from .pg_loss import ActorCriticUpdate, TdLosses, actor_critic_update, td_losses
from .reward_parts import notebook_rewards
from .population import LearnerPopulation, ReinforcePopulation, collect_ppo_population, ppo_update_population
from .actor_critic import AC_LOG_KEYS, ActorCriticRun, actor_critic_train, actor_critic_train_population
from .reinforce import REINFORCE_LOG_KEYS, ReinforceRun, reinforce_train, reinforce_train_population
from .ppo_train import PPO_BATCH_LOG_KEYS, PpoRun, ppo_iteration_data, ppo_train, ppo_train_population

__all__ = [
    "EnvConfig", "VecDroneEnv", "StepInfo", "OBS_KEYS", "grid_shape",
    "DroneGame", "DroneGameClient", "DroneState", "action_bits",
    "shard_bounds", "dist_env", "gather_obs", "gae", "MlpNet",
    "ppo_batch", "reinforce_batch", "collect_ppo",
    "ppo_episodes_batch", "reinforce_episodes_batch", "collect_ppo_steps",
    "ppo_losses", "PpoLosses", "ppo_grads", "PpoGrads",
    "AdamW", "ppo_update", "PpoUpdate",
    "shuffle_batch", "shuffle_indices", "ShuffledBatch",
    "reinforce_losses", "ReinforceLosses", "reinforce_update", "ReinforceUpdate", "collect_reinforce",
    "td_losses", "TdLosses", "actor_critic_update", "ActorCriticUpdate",
    "notebook_rewards", "ActorPopulation", "population_summary",
    "LearnerPopulation", "ppo_update_population", "collect_ppo_population",
    "ActorCriticRun", "actor_critic_train", "actor_critic_train_population", "AC_LOG_KEYS",
    "ReinforcePopulation", "ReinforceRun", "reinforce_train", "reinforce_train_population", "REINFORCE_LOG_KEYS",
    "PpoRun", "ppo_train", "ppo_train_population", "ppo_iteration_data", "PPO_BATCH_LOG_KEYS",
]
__version__ = "0.1.0"
