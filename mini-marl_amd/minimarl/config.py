"""Typed configuration of the QMIX / VDN trainer and presets for BASELINE.json's five configs.

Field names and defaults follow the reference's argparse flags (vdn/_config.py, qmix/_config.py;
``buffer_limit`` counts chunks, ``max_episodes`` / ``epsilon_anneal_episode`` count training
iterations = reference episodes). The reference's ``type=bool`` flags become
real booleans here. Lockstep-specific fields: ``n_envs`` (envs stepped together; one training
iteration = ``max_step`` lockstep steps of all of them) and ``test_envs`` (greedy test episodes run
in parallel, the reference's ``test_episodes``).
"""
from dataclasses import dataclass, field, replace
from typing import Optional


@dataclass
class QTrainConfig:
    algo: str = "vdn"                   # "vdn" | "vdn_double" | "qmix" | "qmix_min"
    # --env_name (vdn/_config.py:19-24 "ma_gym:Checkers-v0"; qmix/_config.py:14-19 "ma_gym:Switch2-v0"):
    # "checkers" | "switch"
    env: str = "checkers"
    n_envs: int = 32
    n_agents: int = 2
    full_observable: bool = True        # vdn/main.py:61-62 (Checkers full obs); QMIX uses partial obs
    max_step: int = 100                 # --max_step
    step_cost: float = -0.01            # --step_cost
    n_actions: int = 5
    # rollout step mode (RolloutEngine persistent=): None = the chunk-persistent launches where they fit, False = one
    # launch per step (e.g. several processes sharing one GPU: the chunk kernel needs every CU for its own blocks)
    persistent: Optional[bool] = None
    # agent Q_Net (vdn/_network.py:14-19): D -> f1 -> g (ReLU) -> GRUCell(g, h) -> A
    f1: int = 64
    g: int = 32
    h: int = 32
    # QMIX Mix_Net (qmix/_network.py:172-197): GRUCell(state, mixer_hidden), hypernet width k1
    mixer_hidden: int = 32
    mixer_k1: int = 32
    # learner (vdn/_config.py:84-121)
    lr: float = 1e-3
    gamma: float = 0.99
    batch_size: int = 32
    chunk_size: int = 10
    update_iter: int = 10
    grad_clip_norm: float = 5.0
    # exploration / target sync (vdn/_config.py:60-80,112-116)
    max_epsilon: float = 0.8
    min_epsilon: float = 0.05
    epsilon_anneal_episode: int = 15000
    update_target_interval: int = 20
    max_episodes: int = 30000
    # prioritized replay (vdn/_config.py:155-191)
    buffer_limit: int = 10000
    eps: float = 1e-6
    alpha: float = 0.4
    beta: float = 0.4
    update_alpha_beta: bool = True
    use_step_weight: bool = True
    step_weight: float = 0.99
    # evaluation (vdn/_config.py:145-152)
    test_interval: int = 1
    test_envs: int = 1
    double_epsilon: bool = True         # vdn_double: the double net explores with the current epsilon
    # True: the reference's TD target w * (sum r + N * gamma * (1-d) * Q'_tot);
    # False: sum r + gamma * (1-d) * Q'_tot (qmix/qmix.py:215-217)
    reference_compat: bool = True
    seed: int = 42

    @property
    def per_flavor(self):
        return "vdn" if self.algo.startswith("vdn") else "qmix"

    def epsilon(self, episode):
        """vdn/main.py:133-134 (qmix/main.py:173-177): linear anneal per training episode."""
        return max(self.min_epsilon, self.max_epsilon - (self.max_epsilon - self.min_epsilon)
                   * (episode / self.epsilon_anneal_episode))


def vdn_reference():
    """vdn/_config.py defaults: Checkers 2 agents, full obs (D = 94), GRU-32, PER alpha = beta = 0.4."""
    return QTrainConfig()


def qmix_reference():
    """qmix/_config.py defaults: the Switch2 env (2 agents, partial obs), alpha 0.8, beta 0.2, buffer
    1000, eps 0.9 -> 0.05 over 60000 episodes, 10 test episodes every 10 episodes."""
    return QTrainConfig(algo="qmix", env="switch", full_observable=False, max_epsilon=0.9, epsilon_anneal_episode=60000,
                        max_episodes=100000, buffer_limit=1000, alpha=0.8, beta=0.2, use_step_weight=False,
                        test_interval=10, test_envs=10)


@dataclass
class MappoTrainConfig:
    """mappo/_config.py values on the hot path (rmappo, shared policy, recurrent chunks; train_batch_size PPO
    minibatches per epoch = MappoTrainer / MappoRunner num_mini_batch). algorithm_name "mappo" (mappo/main.py:62-65):
    feed-forward nets and row minibatches, MappoPolicy(recurrent=False); data_chunk_length is then unused."""
    n_envs: int = 4096
    n_agents: int = 8
    episode_length: int = 100
    hidden: int = 32
    data_chunk_length: int = 5
    ppo_epoch: int = 15
    train_batch_size: int = 1          # the reference's name for the number of minibatches per epoch
    clip_param: float = 0.2
    huber_delta: float = 10.0
    entropy_coef: float = 0.01
    value_loss_coef: float = 0.5
    max_grad_norm: float = 0.5
    lr: float = 1e-4
    critic_lr: float = 1e-4
    opti_eps: float = 1e-5
    gamma: float = 0.99
    gae_lambda: float = 0.95
    seed: int = 1
    # centralized critic over the env's share_obs (mappo/_config.py use_centralized_V; MappoPolicy(cent_agents=n_agents))
    use_centralized_V: bool = False
    algorithm_name: str = "rmappo"     # "rmappo" | "mappo" (feed-forward, mappo/main.py:62-65)
    # --env_name (mappo/_config.py): "checkers" (ma_gym:Checkers-v0) | "switch" (ma_gym:Switch2-v0, local observations
    # with the clock: obs_dim 3, 2 agents; episode_length is also the env's max_steps there)
    env: str = "checkers"

    def __post_init__(self):
        if self.algorithm_name not in ("rmappo", "mappo"):
            raise ValueError(f"algorithm_name={self.algorithm_name!r}: expected 'rmappo' or 'mappo'")
        if self.env not in ("checkers", "switch"):
            raise ValueError(f"env={self.env!r}: expected 'checkers' or 'switch'")
        if self.env == "switch" and self.use_centralized_V and self.n_agents != 2:
            raise ValueError(f"env='switch' with use_centralized_V and n_agents={self.n_agents}: the 3-wide MAPPO "
                             "kernels are built with a decentralized critic or a centralized one over 2 agents")

    @property
    def recurrent(self):
        """The MappoPolicy(recurrent=...) argument of this configuration."""
        return self.algorithm_name != "mappo"


def mappo_switch_reference(**kw):
    """mappo/_config.py pointed at --env_name ma_gym:Switch2-v0: 2 agents, local observations with the clock
    (obs_dim 3), episode_length = the env's max_steps (100, the reference's --max_step)."""
    return MappoTrainConfig(**dict(dict(env="switch", n_agents=2, episode_length=100), **kw))


@dataclass
class OffQTrainConfig:
    """offpolicy/config.py defaults of the episode-level QMix / VDN runner (minimarl.offq_runner.OffQRunner).
    ``n_envs`` is lockstep-specific: the episodes collected per iteration (the reference's ``num_envs``, fixed at 1
    there, base_runner.py:51)."""
    algorithm_name: str = "qmix"        # "qmix" | "vdn"
    n_envs: int = 32
    n_agents: int = 2
    step_cost: float = -0.01
    episode_length: int = 100           # also the env's max_steps
    buffer_size: int = 10000
    batch_size: int = 32
    hidden_size: int = 64
    mixer_hidden_dim: int = 32
    hypernet_hidden_dim: int = 64
    lr: float = 5e-4
    opti_eps: float = 1e-5
    gamma: float = 0.99
    max_grad_norm: float = 10.0
    use_double_q: bool = True
    use_huber_loss: bool = False
    huber_delta: float = 10.0
    use_per: bool = True
    per_nu: float = 0.9
    per_alpha: float = 0.6
    per_eps: float = 1e-6
    per_beta_start: float = 0.4
    use_same_share_obs: bool = True
    use_common_reward: bool = True
    use_soft_update: bool = True
    tau: float = 0.005
    hard_update_interval_episode: int = 200
    epsilon_start: float = 1.0
    epsilon_finish: float = 0.05
    epsilon_anneal_time: int = 50000
    num_random_episodes: int = 5
    train_interval_episode: int = 1
    num_env_steps: int = 2000000
    seed: int = 1
    env: str = "checkers"               # "checkers" | "switch" (local observations with the clock, 2..4 agents)


@dataclass
class Preset:
    name: str
    description: str
    q: QTrainConfig = None
    mappo: MappoTrainConfig = None
    gpus: int = 1
    extra: dict = field(default_factory=dict)


def presets():
    """BASELINE.json configs[0..4] (SURVEY 8d shapes)."""
    cfg2 = replace(qmix_reference(), env="checkers", n_agents=8, n_envs=4096, g=64, h=64, mixer_hidden=64,
                   buffer_limit=65536)
    return {
        "cfg1": Preset("cfg1", "VDN on 2-agent cooperative gridworld, 32 parallel envs (D = 94 full obs, GRU-32)",
                       q=replace(vdn_reference(), n_envs=32)),
        "cfg2": Preset("cfg2", "QMIX 8-agent gridworld, 4096 envs, GRU-64 agents + Hm-64 hypernet mixer, 1 GPU",
                       q=cfg2),
        "cfg3": Preset("cfg3", "MAPPO 8-agent, 4096 envs, shared actor-critic, device GAE, 1 GPU",
                       mappo=MappoTrainConfig()),
        "cfg4": Preset("cfg4", "QMIX 8-agent, 32768 envs sharded 4096 per GPU over 8 GPUs, RCCL gradient all-reduce",
                       q=cfg2, gpus=8),
        "cfg5": Preset("cfg5", "QMIX SMAC-scale 27 agents, obs 300, 36 actions, 8192 envs, GRU-32, 8 GPUs "
                               "(no env of that shape exists: synthetic observations)",
                       q=replace(qmix_reference(), env="checkers", n_agents=27, n_envs=8192, n_actions=36, g=32, h=32,
                                 mixer_hidden=32, buffer_limit=65536),
                       gpus=8, extra={"obs_dim": 300}),
    }
