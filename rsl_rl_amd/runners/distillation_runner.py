"""Distillation runner (rsl_rl/runners/distillation_runner.py:21-180): student-teacher training behind the
OnPolicyRunner interface.

Construction (`class_name` "StudentTeacher" / "Distillation" resolved against rsl_rl_amd), learn(), and the inherited
save() / load() / log() / get_inference_policy() behave as in the reference: the "teacher" observation set defaults
like the reference's, the storage is the "distillation" RolloutStorage, learn() refuses to start before a teacher has
been loaded (load() of an RL checkpoint fills it; of a distillation checkpoint resumes), and the iteration timing is
returned through `last_iteration_stats` like the PPO runner's.
"""

from __future__ import annotations

import os
import time
from collections import deque

import torch

import rsl_rl_amd
from rsl_rl_amd.algorithms import Distillation
from rsl_rl_amd.env import VecEnv
from rsl_rl_amd.networks import fused_mlp
from rsl_rl_amd.utils import resolve_obs_groups, store_code_state

from .on_policy_runner import OnPolicyRunner, _resolve_class


class DistillationRunner(OnPolicyRunner):
    """On-policy runner for training and evaluation of teacher-student training."""

    def __init__(self, env: VecEnv, train_cfg: dict, log_dir: str | None = None, device="cpu"):
        self.cfg = train_cfg
        self.alg_cfg = train_cfg["algorithm"]
        self.policy_cfg = train_cfg["policy"]
        self.device = device
        self.env = env
        self._configure_multi_gpu()
        self.num_steps_per_env = self.cfg["num_steps_per_env"]
        self.save_interval = self.cfg["save_interval"]

        obs = self.env.get_observations()
        self.cfg["obs_groups"] = resolve_obs_groups(obs, self.cfg["obs_groups"], default_sets=["teacher"])
        self.alg = self._construct_algorithm(obs)

        self.disable_logs = self.is_distributed and self.gpu_global_rank != 0
        self.log_dir = log_dir
        self.writer = None
        self.logger_type = self.cfg.get("logger", "tensorboard").lower()
        self.tot_timesteps = 0
        self.tot_time = 0
        self.current_learning_iteration = 0
        self.git_status_repos = [rsl_rl_amd.__file__]
        self.last_iteration_stats: dict = {}
        self.iteration_stats_history: deque = deque(maxlen=1024)

    # ------------------------------------------------------------------ training loop (distillation_runner.py:57-150)
    def learn(self, num_learning_iterations: int, init_at_random_ep_len: bool = False):  # noqa: C901
        self._prepare_logging_writer()
        if not self.alg.policy.loaded_teacher:
            raise ValueError("Teacher model parameters not loaded. Please load a teacher model to distill.")
        if init_at_random_ep_len:
            self.env.episode_length_buf = torch.randint_like(
                self.env.episode_length_buf, high=int(self.env.max_episode_length)
            )
        obs = self.env.get_observations().to(self.device)
        self.train_mode()

        ep_infos = []
        rewbuffer, lenbuffer = deque(maxlen=100), deque(maxlen=100)
        n_env = self.env.num_envs
        cur_reward_sum = torch.zeros(n_env, dtype=torch.float, device=self.device)
        cur_episode_length = torch.zeros(n_env, dtype=torch.float, device=self.device)

        if self.is_distributed:
            print(f"Synchronizing parameters for rank {self.gpu_global_rank}...")
            self.alg.broadcast_parameters()

        start_iter = self.current_learning_iteration
        tot_iter = start_iter + num_learning_iterations
        for it in range(start_iter, tot_iter):
            start = time.time()
            with torch.inference_mode(), fused_mlp.frozen_weights():
                for _ in range(self.num_steps_per_env):
                    actions = self.alg.act(obs)
                    obs, rewards, dones, extras = self.env.step(actions.to(self.env.device))
                    obs, rewards, dones = obs.to(self.device), rewards.to(self.device), dones.to(self.device)
                    self.alg.process_env_step(obs, rewards, dones, extras)
                    if self.log_dir is not None:
                        if "episode" in extras:
                            ep_infos.append(extras["episode"])
                        elif "log" in extras:
                            ep_infos.append(extras["log"])
                        cur_reward_sum += rewards
                        cur_episode_length += 1
                        new_ids = (dones > 0).nonzero(as_tuple=False)
                        rewbuffer.extend(cur_reward_sum[new_ids][:, 0].cpu().numpy().tolist())
                        lenbuffer.extend(cur_episode_length[new_ids][:, 0].cpu().numpy().tolist())
                        cur_reward_sum[new_ids] = 0
                        cur_episode_length[new_ids] = 0
                stop = time.time()
                collection_time = stop - start
                start = stop

            loss_dict = self.alg.update()
            stop = time.time()
            learn_time = stop - start
            self.current_learning_iteration = it
            steps = self.num_steps_per_env * n_env * self.gpu_world_size
            self.last_iteration_stats = {
                "collection_time": collection_time,
                "learn_time": learn_time,
                "total_fps": steps / (collection_time + learn_time),
                "loss_dict": loss_dict,
            }
            self.iteration_stats_history.append((collection_time, learn_time))
            if self.log_dir is not None and not self.disable_logs:
                self.log(locals())
                if it % self.save_interval == 0:
                    self.save(os.path.join(self.log_dir, f"model_{it}.pt"))
            ep_infos.clear()
            if it == start_iter and not self.disable_logs and self.log_dir is not None:
                paths = store_code_state(self.log_dir, self.git_status_repos)
                if self.logger_type in ["wandb", "neptune"] and paths:
                    for path in paths:
                        self.writer.save_file(path)

        if self.log_dir is not None and not self.disable_logs:
            self.save(os.path.join(self.log_dir, f"model_{self.current_learning_iteration}.pt"))

    # ------------------------------------------------------------------ helpers (distillation_runner.py:156-179)
    def _construct_algorithm(self, obs) -> Distillation:
        policy_class = _resolve_class(self.policy_cfg.pop("class_name"))
        policy = policy_class(obs, self.cfg["obs_groups"], self.env.num_actions, **self.policy_cfg).to(self.device)
        alg_class = _resolve_class(self.alg_cfg.pop("class_name"))
        alg: Distillation = alg_class(policy, device=self.device, **self.alg_cfg, multi_gpu_cfg=self.multi_gpu_cfg)
        alg.init_storage("distillation", self.env.num_envs, self.num_steps_per_env, obs, [self.env.num_actions])
        return alg
