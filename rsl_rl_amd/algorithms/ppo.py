"""PPO with the fused HIP loss (rsl_rl/algorithms/ppo.py:19-469).

Constructor, attributes (policy, optimizer, storage, learning_rate, rnd, rnd_optimizer, transition,
intrinsic_rewards, ...) and methods (init_storage, act, process_env_step, compute_returns, update,
broadcast_parameters, reduce_parameters) keep the reference's signatures and semantics.  The update
differs in how each mini-batch is evaluated:

* for the standard ActorCritic the update runs without autograd: the actor and critic forwards keep
  their activations (networks/fused_mlp.train_forward), one fused kernel (kernels.ppo_loss_fwd_bwd)
  computes the KL, the clipped surrogate, the clipped value loss, the entropy and the exact gradients
  d(loss)/d(mean, sigma, V), and the MLP backward kernels write every parameter gradient straight into
  its slot of one contiguous gradient arena (GradArena) -- each parameter's .grad is a view of it;
* under multi-GPU the arena holds, after the gradients, the mini-batch KL: ONE RCCL all-reduce of that
  buffer (SUM, then / world size) averages the gradients and the KL together (ppo.py:271-273 and
  ppo.py:441-469 fused into one collective per mini-batch);
* the adaptive learning rate, the loss statistics, gradient clipping and the Adam step stay on the device
  (kernels.ppo_update_tail, kernels.FusedClipAdam): no host synchronisation per mini-batch.
* with a symmetry_cfg (ppo.py:213-257, :317-348) the actor runs once on the K augmented copies of the mini-batch and
  kernels.ppo_loss_sym_fwd_bwd adds the mirror term's gradient at the mean (PPO._symmetric_minibatch).
* a recurrent policy (ActorCriticRecurrent) takes RolloutStorage.recurrent_mini_batch_generator (whole trajectories per
  mini-batch, split and padded by the trajectory kernels) and the autograd path below with the [T, E, ...] fields
  flattened to the loss kernel's rows: two host read-backs per update (the trajectory boundaries, the statistics).
* a recurrent policy of two one-layer LSTMs, or of two one-layer GRUs, of hidden size 256 or 512 (§27) whose
  mini-batches hold a multiple of 64 envs takes RolloutStorage.recurrent_sequence_generator instead (env-major sequences, no padding) and
  PPO._recurrent_minibatch: the fused cell's training form and reverse step, the actor's and the
  critic's memories paired per launch, around the manual path's MLP pair, heads and loss; every gradient in the
  arena, one read-back per update.
  RSLRL_RECURRENT_FUSED=0 keeps the autograd path.
Any other policy keeps the autograd path (the reference's structure, with the KL appended to the
gradient concatenation of reduce_parameters).

update() reads as the reference's loop.  Per mini-batch (a MiniBatch), in this order: forward, loss and backward by the
strategy chosen at the first one (_symmetric_minibatch, _manual_minibatch or _autograd_minibatch; _recurrent_minibatch
is chosen with its generator: mini-batch in, stats out, gradients in the arena or in .grad), _rnd_minibatch,
_reduce_minibatch, _lr_rule_and_tail, _step_optimizers.

Multi-GPU LR rule: the reference all-reduces kl_mean, lets rank 0 decide, broadcasts the lr as an fp32
tensor and reads it back (ppo.py:272-290).  After the all-reduce every rank holds the same kl_mean, so
each rank applies the same rule locally and rounds the lr through fp32 exactly like the broadcast did:
same learning rates on every rank, no broadcast.
"""

from __future__ import annotations

import os
from itertools import chain
from types import SimpleNamespace

import torch
import torch.nn as nn
import torch.optim as optim

from .. import _lib, kernels
from ..modules import ActorCritic, ActorCriticRecurrent
from ..networks import fused_mlp
from ..modules.act_graph import RolloutActGraph
from ..modules.rnd import RandomNetworkDistillation
from ..modules.symmetry import SignedPermutationSymmetry
from ..storage import RolloutStorage
from ..utils import string_to_callable
from .arena import GradArena, all_reduce_arena, reduce_gradients  # (GradArena stays importable from here)

# RSLRL_FUSED_TAIL=0 (A/B; the same values): the per-mini-batch lr rule / loss sums as their own launch instead of
# inside the clip-and-Adam norm launch
_FUSED_TAIL = os.environ.get("RSLRL_FUSED_TAIL", "1") != "0"


def adapt_learning_rate(learning_rate: float, kl_mean: float, desired_kl: float) -> float:
    """The adaptive schedule of ppo.py:280-284."""
    if kl_mean > desired_kl * 2.0:
        return max(1e-5, learning_rate / 1.5)
    if kl_mean < desired_kl / 2.0 and kl_mean > 0.0:
        return min(1e-2, learning_rate * 1.5)
    return learning_rate


def adapt_learning_rate_device(lr: torch.Tensor, kl_mean: torch.Tensor, desired_kl: float) -> torch.Tensor:
    """ppo.py:280-284 without leaving the device: lr is an fp64 0-d tensor (the reference's Python float),
    kl_mean the fp32 KL; the comparisons happen in fp32 against fp32(2 * kl*) / fp32(kl* / 2), exactly as
    the reference's `tensor > python_float` does."""
    kl = kl_mean.reshape(())
    # Python-float operands: torch compares a fp32 tensor with a wrapped scalar in fp32, like the reference,
    # and no threshold tensor has to be copied to the device (a pageable copy would synchronise)
    down = torch.clamp(lr / 1.5, min=1e-5)
    up = torch.clamp(lr * 1.5, max=1e-2)
    return torch.where(kl > desired_kl * 2.0, down, torch.where((kl < desired_kl / 2.0) & (kl > 0.0), up, lr))


class MiniBatch:
    """The 10-tuple of RolloutStorage's mini-batch generators, named.  index: its slice of the update's permutation
    (the same in every epoch).  stored: what the loss wrappers take after (mean, sigma, value), in their order."""

    __slots__ = ("index", "obs", "actions", "target_values", "advantages", "returns", "old_log_prob", "old_mu",
                 "old_sigma", "hid_states", "masks", "stored")

    def __init__(self, index, fields):
        (self.obs, self.actions, self.target_values, self.advantages, self.returns, self.old_log_prob, self.old_mu,
         self.old_sigma, self.hid_states, self.masks) = fields
        self.index = index
        self.stored = (self.actions, self.old_log_prob, self.advantages, self.target_values, self.returns, self.old_mu,
                       self.old_sigma)


class PPO:
    """Proximal Policy Optimization algorithm (https://arxiv.org/abs/1707.06347)."""

    policy: ActorCritic

    def __init__(
        self,
        policy,
        num_learning_epochs=5,
        num_mini_batches=4,
        clip_param=0.2,
        gamma=0.99,
        lam=0.95,
        value_loss_coef=1.0,
        entropy_coef=0.01,
        learning_rate=0.001,
        max_grad_norm=1.0,
        use_clipped_value_loss=True,
        schedule="adaptive",
        desired_kl=0.01,
        device="cpu",
        normalize_advantage_per_mini_batch=False,
        rnd_cfg: dict | None = None,
        symmetry_cfg: dict | None = None,
        multi_gpu_cfg: dict | None = None,
    ):
        self.device = device
        self.is_multi_gpu = multi_gpu_cfg is not None
        if multi_gpu_cfg is not None:
            self.gpu_global_rank = multi_gpu_cfg["global_rank"]
            self.gpu_world_size = multi_gpu_cfg["world_size"]
        else:
            self.gpu_global_rank = 0
            self.gpu_world_size = 1

        if getattr(policy, "is_recurrent", False):
            # the reference hands zero-padded trajectories to both (ppo.py:226-257 / :317-348 augment and mirror the
            # padded batch, :352-363 runs RND on it); nothing here guesses at what that should mean
            if symmetry_cfg is not None:
                raise NotImplementedError(
                    "a recurrent policy with symmetry_cfg is not supported: rsl_rl/algorithms/ppo.py:226-257 and "
                    ":317-348 apply the augmentation and the mirror loss to zero-padded trajectories")
            if rnd_cfg is not None:
                raise NotImplementedError(
                    "a recurrent policy with rnd_cfg is not supported: rsl_rl/algorithms/ppo.py:352-363 evaluates the "
                    "RND loss on zero-padded trajectories")
        if rnd_cfg is not None:
            rnd_lr = rnd_cfg.pop("learning_rate", 1e-3)
            self.rnd = RandomNetworkDistillation(device=self.device, **rnd_cfg)
            self.rnd_optimizer = optim.Adam(self.rnd.predictor.parameters(), lr=rnd_lr)
        else:
            self.rnd = None
            self.rnd_optimizer = None
        self.intrinsic_rewards = None

        if symmetry_cfg is not None:
            use_symmetry = symmetry_cfg["use_data_augmentation"] or symmetry_cfg["use_mirror_loss"]
            if not use_symmetry:
                print("Symmetry not used for learning. We will use it for logging instead.")
            if isinstance(symmetry_cfg["data_augmentation_func"], str):
                symmetry_cfg["data_augmentation_func"] = string_to_callable(symmetry_cfg["data_augmentation_func"])
            if symmetry_cfg["use_data_augmentation"] and not callable(symmetry_cfg["data_augmentation_func"]):
                raise ValueError(
                    "Data augmentation enabled but the function is not callable:"
                    f" {symmetry_cfg['data_augmentation_func']}"
                )
            self.symmetry = symmetry_cfg
        else:
            self.symmetry = None

        self.policy = policy
        self.policy.to(self.device)
        # on a ROCm device Adam runs fused (one kernel per step) and accepts the device-resident lr of update()
        on_gpu = str(device).startswith("cuda")
        self.optimizer = optim.Adam(self.policy.parameters(), lr=learning_rate, fused=True if on_gpu else None)
        # clip_grad_norm_ + optimizer.step() as two launches (kernels.FusedClipAdam, ppo.py:373-374)
        self._clip_adam = (kernels.FusedClipAdam(self.optimizer, max_grad_norm)
                           if on_gpu and kernels.FusedClipAdam.supported(self.optimizer) else None)
        # the RND predictor's optimizer.step() (unclipped, ppo.py:383-384) as one fused launch pair, used when the
        # update runs the RND step on the fused kernels (_rnd_update_plan)
        self._rnd_adam = (kernels.FusedClipAdam(self.rnd_optimizer, 0.0)
                          if on_gpu and self.rnd_optimizer is not None
                          and kernels.FusedClipAdam.supported(self.rnd_optimizer) else None)
        self._act_graph = RolloutActGraph(self.policy) if on_gpu and isinstance(self.policy, ActorCritic) else None
        self.storage: RolloutStorage = None  # type: ignore
        self.transition = RolloutStorage.Transition()

        self.clip_param = clip_param
        self.num_learning_epochs = num_learning_epochs
        self.num_mini_batches = num_mini_batches
        self.value_loss_coef = value_loss_coef
        self.entropy_coef = entropy_coef
        self.gamma = gamma
        self.lam = lam
        self.max_grad_norm = max_grad_norm
        self.use_clipped_value_loss = use_clipped_value_loss
        self.desired_kl = desired_kl
        self.schedule = schedule
        self.learning_rate = learning_rate
        self.normalize_advantage_per_mini_batch = normalize_advantage_per_mini_batch

        self._arena: GradArena | None = None  # gradient arena of the manual update path (see update())
        # while update() runs: the fp64 device scalar that holds the reference's self.learning_rate (decided on the
        # device per mini-batch, read back once at the end); None otherwise.  Read by anything that wants the lr a
        # given optimizer step uses without a host sync point per mini-batch (tests/update_fixtures.py records the
        # lr trace through it)
        self.learning_rate_device = None

    def init_storage(self, training_type, num_envs, num_transitions_per_env, obs, actions_shape):
        self.storage = RolloutStorage(training_type, num_envs, num_transitions_per_env, obs, actions_shape,
                                      self.device)

    # ------------------------------------------------------------------ rollout (ppo.py:129-169)
    def act(self, obs):
        if self.policy.is_recurrent:
            self.transition.hidden_states = self.policy.get_hidden_states()
        pcls = type(self.policy)
        if isinstance(self.policy, ActorCritic) and pcls.act is ActorCritic.act and pcls.evaluate is ActorCritic.evaluate:
            # the actor's and critic's hidden layers batched into one launch each (same values and draws), replayed
            # as one captured HIP graph per configuration (modules/act_graph.py)
            res = None
            if self._act_graph is not None and RolloutActGraph.enabled():
                res = self._act_graph(obs)
            actions, values = res if res is not None else self.policy.act_and_evaluate(obs)
        elif (isinstance(self.policy, ActorCriticRecurrent) and pcls.act is ActorCriticRecurrent.act
              and pcls.evaluate is ActorCriticRecurrent.evaluate):
            # both memories' LSTM / GRU steps in one launch where the fused cell takes them (same values and draws)
            actions, values = self.policy.act_and_evaluate(obs)
        else:
            actions, values = self.policy.act(obs), self.policy.evaluate(obs)
        self.transition.actions = actions.detach()
        self.transition.values = values.detach()
        self.transition.action_mean = self.policy.action_mean.detach()
        self.transition.action_sigma = self.policy.action_std.detach()
        self.transition.observations = obs
        if not self._fused_rollout():
            self.transition.actions_log_prob = self.policy.get_actions_log_prob(self.transition.actions).detach()
        # else: the log-prob is computed by the fused record kernel in process_env_step
        return self.transition.actions

    def _fused_rollout(self) -> bool:
        return self.storage is not None and self.storage.fused_record_ok(self.transition)

    def _rnd_fused_args(self, obs):
        """Arguments of the RND part of the fused record, or None when the RND module is not of the fused
        form (one hidden ELU layer <= 64 wide, <= 8 outputs, no reward normalisation)."""
        rnd = self.rnd
        if rnd is None or rnd.reward_normalization:
            return None
        nets = []
        for mlp in (rnd.target, rnd.predictor):
            mods = [m for m in mlp]
            lin = [m for m in mods if isinstance(m, torch.nn.Linear)]
            if (len(mods) != 3 or len(lin) != 2 or not isinstance(mods[1], torch.nn.ELU) or mods[1].alpha != 1.0
                    or lin[0].in_features > 64 or lin[0].out_features > 64 or lin[1].out_features > 8):
                return None
            nets.append(lin)
        if nets[0][0].out_features != nets[1][0].out_features:
            return None
        groups = rnd.obs_groups["rnd_state"]
        state = obs[groups[0]] if len(groups) == 1 else torch.cat([obs[g] for g in groups], dim=-1)
        # weight schedule (rnd.py:128-132), evaluated on the host as the reference does
        rnd.update_counter += 1
        if rnd.weight_scheduler is not None:
            rnd.weight = rnd.weight_scheduler(step=rnd.update_counter, **rnd.weight_scheduler_params)
        else:
            rnd.weight = rnd.initial_weight
        args = {"obs": state, "hidden": nets[0][0].out_features, "out": nets[0][1].out_features,
                "target": kernels.pack_rnd_net(rnd.target), "predictor": kernels.pack_rnd_net(rnd.predictor),
                "weight": rnd.weight}
        if rnd.state_normalization:
            sn = rnd.state_normalizer
            args.update(state_mean=sn._mean, state_std=sn._std, state_eps=sn.eps)
        return args

    def process_env_step(self, obs, rewards, dones, extras):
        self.policy.update_normalization(obs)
        if self.rnd:
            self.rnd.update_normalization(obs)
        time_outs = extras.get("time_outs") if isinstance(extras, dict) else None
        if self._fused_rollout():
            # ppo.py:142-169 + rollout_storage.py:77-103 + rnd.py:113-135 in one launch
            rnd_args = self._rnd_fused_args(obs) if self.rnd else None
            extra = None
            if self.rnd and rnd_args is None:  # RND of a form the kernel does not evaluate: PyTorch, then fused add
                extra = self.rnd.get_intrinsic_reward(obs)
                self.intrinsic_rewards = extra
            elif rnd_args is not None:
                self.intrinsic_rewards = torch.empty(rewards.shape[0], dtype=torch.float32, device=rewards.device)
            if time_outs is not None:
                time_outs = time_outs.to(self.device)
            self.storage.add_transition_fused(self.transition, rewards, dones, time_outs, self.gamma,
                                              extra_reward=extra, rnd=rnd_args,
                                              intrinsic_out=self.intrinsic_rewards if rnd_args is not None else None)
        else:
            self.transition.rewards = rewards.clone()
            self.transition.dones = dones
            if self.rnd:
                self.intrinsic_rewards = self.rnd.get_intrinsic_reward(obs)
                self.transition.rewards += self.intrinsic_rewards
            if time_outs is not None:  # bootstrap on time-outs (ppo.py:161-164)
                self.transition.rewards += self.gamma * torch.squeeze(
                    self.transition.values * time_outs.unsqueeze(1).to(self.device), 1
                )
            self.storage.add_transitions(self.transition)
        self.transition.clear()
        self.policy.reset(dones)

    def compute_returns(self, obs):
        last_values = self.policy.evaluate(obs).detach()
        self.storage.compute_returns(last_values, self.gamma, self.lam,
                                     normalize_advantage=not self.normalize_advantage_per_mini_batch)

    # ------------------------------------------------------------------ update (ppo.py:178-422)
    def _trainable_params(self):
        params = list(self.policy.parameters())
        if self.rnd:  # only the predictor receives gradients (the target output is detached)
            params += list(self.rnd.predictor.parameters())
        return [p for p in params if p.requires_grad]

    def grad_arena(self) -> GradArena:
        """The gradient arena over the trainable parameters (+ one KL slot), created on first use and whenever
        the parameter list changes."""
        params = self._trainable_params()
        if self._arena is None or not self._arena.matches(params) or self._arena.flat.device != params[0].device:
            early = self._early_params() if self.is_multi_gpu else ()
            self._arena = GradArena(params, extra=1, device=params[0].device, early=early)
        return self._arena

    def _early_params(self):
        """Parameters whose gradients the manual backward completes before its last layer: every Linear of the actor
        and the critic but the first (the paired backward runs the output layers, then the hidden layers from the top;
        the first layers' weight gradients come last).  With RSLRL_OVERLAP_ALLREDUCE=1 their arena prefix is
        all-reduced while the first layers' backward runs.  Off by default since round 6: on RCCL at
        world 1 the two collectives cost what the single one does (profiles/r6_overlap_ab.json), and at world > 1 the
        fused backward holds every CU's registers and LDS (one 256-VGPR workgroup per CU), so the collective's kernel
        cannot co-run with it anyway -- the split only doubles the latency-bound calls."""
        if os.environ.get("RSLRL_OVERLAP_ALLREDUCE", "0") != "1" or not isinstance(self.policy, ActorCritic):
            return ()
        out = []
        for net in (self.policy.actor, self.policy.critic):
            lins = [m for m in net.modules() if isinstance(m, nn.Linear)]
            for m in lins[1:]:
                out += [m.weight, m.bias]
        return out

    def _host_lr_rule(self, kl: float) -> float:
        """The adaptive lr decided on the host (ppo.py:280-294) from a KL that is already averaged over ranks: the
        rule, under multi-GPU the fp32 round-trip of the reference's lr broadcast, then every param_group's lr."""
        self.learning_rate = adapt_learning_rate(self.learning_rate, kl, self.desired_kl)
        if self.is_multi_gpu:
            self.learning_rate = torch.tensor(self.learning_rate, dtype=torch.float32).item()
        for param_group in self.optimizer.param_groups:
            param_group["lr"] = self.learning_rate
        return self.learning_rate

    def _sync_kl_and_lr(self, kl_mean: torch.Tensor):
        """KL all-reduce + adaptive lr + fp32 lr rounding under multi-GPU (ppo.py:271-294), host version
        (one device read-back); the update keeps the lr on the device instead (kernels.ppo_update_tail)."""
        if self.is_multi_gpu:
            torch.distributed.all_reduce(kl_mean, op=torch.distributed.ReduceOp.SUM)
            kl_mean /= self.gpu_world_size
        kl = kl_mean.item()
        self._host_lr_rule(kl)
        return kl

    def update(self):
        adaptive = self.desired_kl is not None and self.schedule == "adaptive"
        dev = self.storage.values.device
        if self._clip_adam is not None:
            self._clip_adam.adopt_loaded_state()  # a checkpoint of a non-fused Adam may have been loaded
        sym = self.symmetry  # None: nothing below differs from the plain update
        u = SimpleNamespace(dev=dev, adaptive=adaptive)  # what lives for this call, for the steps below
        # value, surrogate, entropy, rnd (+ symmetry, summed by the symmetric loss kernel)
        sums = u.sums = torch.zeros(5 if sym else 4, dtype=torch.float64, device=dev)
        u.stats_buf = torch.empty(8, dtype=torch.float32, device=dev)
        # device-resident lr (needs an optimizer that takes a tensor lr: fused / capturable Adam)
        device_lr = adaptive and dev.type == "cuda" and self._optimizer_takes_tensor_lr()
        # torch.full, not torch.tensor: a fill launch instead of a pageable host-to-device copy, which would block the
        # host until the rollout's kernels have drained (the GPU then idles through the update's host prologue)
        lr_dev = torch.full((), self.learning_rate, dtype=torch.float64, device=dev) if device_lr else None
        self.learning_rate_device = lr_dev  # the reference's self.learning_rate during update() (fp64, device)
        lr32 = None
        if device_lr:  # the optimizer reads the lr as this fp32 device tensor (written by ppo_update_tail)
            lr32 = torch.full((), self.learning_rate, dtype=torch.float32, device=dev)
            for param_group in self.optimizer.param_groups:
                param_group["lr"] = lr32
        u.loss_kw = dict(clip_param=self.clip_param, value_loss_coef=self.value_loss_coef,
                         entropy_coef=self.entropy_coef, use_clipped_value_loss=self.use_clipped_value_loss,
                         compute_kl=adaptive, normalize_advantage=self.normalize_advantage_per_mini_batch,
                         stats=u.stats_buf)
        # the manual path's gradient arena (None: autograd) and the early prefix's pending all-reduces
        u.arena, u.early_work = None, []
        # the predictor's trainable parameters (_trainable_params' filter: exactly the arena's RND span)
        u.rnd_params = [p for p in self.rnd.predictor.parameters() if p.requires_grad] if self.rnd else []
        u.rnd_fused = None  # decided at the first mini-batch (needs the observation batch and the arena)
        # per MiniBatch.index: the RND target embedding; a recurrent policy's stored fields as the loss kernel's rows
        u.target_cache, u.flat_fields = {}, {}
        # decided at the first mini-batch (needs the observation batch) unless the generator comes with its strategy
        generator, strategy = self._mini_batches(u)
        for index, fields in enumerate(generator):
            mb = MiniBatch(index % self.num_mini_batches, fields)
            if strategy is None:
                strategy = self._choose_strategy(u, mb.obs)
            stats = strategy(u, mb)  # forward, loss, backward (ppo.py:246-253, :259-315, :367-372)
            self._rnd_minibatch(u, mb)  # RND loss and backward (ppo.py:352-363, :369-371)
            kl_src = self._reduce_minibatch(stats, u.arena, adaptive, u.early_work)  # (ppo.py:271-273, :376)
            tail = self._lr_rule_and_tail(stats, kl_src, adaptive, lr_dev, lr32, sums)  # (ppo.py:259-294, :387-395)
            self._step_optimizers(tail, u.rnd_fused)  # clip + Adam (ppo.py:373-374, :383-384)

        num_updates = self.num_learning_epochs * self.num_mini_batches
        # one read-back for the loss means and the device lr (back to a Python float, as the reference keeps it)
        # (+ compute_returns' grid-barrier status word, if its one-launch form ran: nonzero = NaN advantages, raise)
        gae_status = getattr(self.storage, "gae_status", None)
        parts = [sums / num_updates] + ([lr_dev.reshape(1)] if device_lr else [])
        if gae_status is not None:
            parts.append(gae_status.to(sums.dtype))
        host = torch.cat(parts).tolist()
        if device_lr:
            self.learning_rate = host[sums.numel()]
            self.learning_rate_device = None
            for param_group in self.optimizer.param_groups:
                param_group["lr"] = self.learning_rate
        self.storage.clear()
        if gae_status is not None:
            # the rollout's advantages were NaN, and so are this update's parameters: stop loudly
            self.storage.gae_status = None
            kernels.raise_on_gae_status(gae_status, host[-1])
        loss_dict = {"value_function": host[0], "surrogate": host[1], "entropy": host[2]}
        if self.rnd:
            loss_dict["rnd"] = host[3]
        if sym:
            loss_dict["symmetry"] = host[4]
        return loss_dict

    # ---- forward, loss and backward of one mini-batch: (u, mb) -> stats, gradients in the arena or in .grad
    def _mini_batches(self, u):
        """(generator, strategy or None).  A recurrent policy takes whole trajectories per mini-batch (ppo.py:194-195):
        as env-major sequences on the fused LSTM / GRU kernels where _recurrent_fused_ok (the arena is bound here), else
        zero-padded for the RNN library under autograd."""
        st, M, K = self.storage, self.num_mini_batches, self.num_learning_epochs
        if not self.policy.is_recurrent:
            return st.mini_batch_generator(M, K), None
        if self._recurrent_fused_ok():
            u.arena, u.seq = self.grad_arena(), None
            u.arena.bind()
            return st.recurrent_sequence_generator(M, K), self._recurrent_minibatch
        return st.recurrent_mini_batch_generator(M, K), None

    def _recurrent_fused_ok(self) -> bool:
        """The recurrent update runs on the fused LSTM or GRU kernels: our storage with one-layer fp32 states saved for
        both memories -- (h, c) for LSTMs, the bare h for GRUs -- a policy that qualifies at
        E = num_envs // num_mini_batches rows (ActorCriticRecurrent.manual_update_ok), and RSLRL_RECURRENT_FUSED not 0
        (it keeps the autograd path for both kinds)."""
        st, pol = self.storage, self.policy
        if (os.environ.get("RSLRL_RECURRENT_FUSED", "1") == "0" or not isinstance(pol, ActorCriticRecurrent)
                or not isinstance(st, RolloutStorage) or self.symmetry is not None or self.rnd is not None):
            return False
        saved = (st.saved_hidden_states_a, st.saved_hidden_states_c)
        cell = kernels.cell_of(pol.memory_a.rnn)
        n_states = cell.n_state if cell is not None else 0  # (no cell: manual_update_ok refuses below)
        if any(s is None or len(s) != n_states or any(h.dim() != 4 or h.shape[1] != 1 or h.dtype != torch.float32 for h in s)
               for s in saved):
            return False
        return pol.manual_update_ok(st.observations, st.num_envs // self.num_mini_batches)

    def _choose_strategy(self, u, obs_batch):
        """manual: the MLP passes run without autograd into the gradient arena (u.arena, bound here)."""
        manual = (isinstance(self.policy, ActorCritic) and self.policy.manual_update_ok(obs_batch)
                  and all(p.requires_grad for p in self.policy.parameters()))
        if self.symmetry and manual and (self.policy.has_wide_mlp or self.policy.has_ragged_mlp):
            # the symmetric update of a wide stack (hidden widths above 256) or a ragged one (an observation width that
            # is no multiple of 4) stays on autograd
            manual = False
        if manual:
            u.arena = self.grad_arena()
            u.arena.bind()
        if self.symmetry:
            return self._symmetric_minibatch
        return self._manual_minibatch if manual else self._autograd_minibatch

    def _grad_sigma_dest(self, arena, like=None, width=None, dev=None):
        """Where a loss kernel reduces the shared std's d sigma: the std's arena slot for "scalar" (the parameter is
        sigma), else a fresh buffer as the call site sizes it: like `like`, or an fp32 vector of `width` on `dev`."""
        if self.policy.noise_std_type == "scalar":
            return arena.slot(self.policy.std)
        return torch.empty_like(like) if like is not None else torch.empty(width, device=dev, dtype=torch.float32)

    def _loss_grad_buffers(self, arena, mean, sigma):
        g_mean, g_sigma = self.policy.train_grad_buffers(mean, sigma)
        if g_sigma is None:  # shared std: d sigma reduced by the loss kernel
            g_sigma = self._grad_sigma_dest(arena, like=sigma)
        return g_mean, g_sigma

    def _autograd_backward(self, mean, sigma, value, g_mean, g_sigma, g_value):
        """The loss kernel's gradients pushed through the policy's autograd graph (ppo.py:367-368)."""
        for p in self.policy.parameters():  # optimizer.zero_grad() (set_to_none)
            p.grad = None
        outs, grads = [mean, value], [g_mean, g_value]
        if sigma.requires_grad:
            outs.append(sigma)
            grads.append(g_sigma)
        torch.autograd.backward(outs, grads)

    def _loss_heads(self, u, stored):
        """(value head, actor head or None) of a mini-batch's stored rows.  The critic's last launch also runs d(value
        loss)/dV and the value head's backward (the same values as the loss kernel's d/dV followed by the output-layer
        backward); the actor's last launch may also run the loss and the output layer's backward (shared std, no
        per-mini-batch advantage normalisation): the same statistics and d sigma as the loss kernel."""
        actions, target_values, returns = stored[0], stored[3], stored[4]
        vh = fused_mlp.ValueHead(target_values, returns, self.clip_param, self.value_loss_coef,
                                 self.use_clipped_value_loss)
        ah = None
        if (not self.normalize_advantage_per_mini_batch and not self.policy.state_dependent_std
                and _lib.actor_head_width_ok(actions.shape[-1])):
            ah = fused_mlp.ActorHead(
                *stored, None, clip_param=self.clip_param, value_loss_coef=self.value_loss_coef,
                entropy_coef=self.entropy_coef, use_clipped=self.use_clipped_value_loss, compute_kl=u.adaptive,
                grad_sigma=self._grad_sigma_dest(u.arena, width=actions.shape[-1], dev=u.dev), stats=u.stats_buf)
        return vh, ah

    def _loss_after_forward(self, u, ah, mean, sigma, value, stored):
        """(stats, d mean, d sigma, d value): from the actor's launch where the head ran the loss there, else the loss
        kernel's."""
        if ah is not None and ah.done:  # loss and d loss / d mu ran inside the actor's launch
            return u.stats_buf, mean, ah.grad_sigma, value
        g_mean, g_sigma = self._loss_grad_buffers(u.arena, mean, sigma)
        # the value head's gradient: a contiguous [B, 1] (the critic's fused output-layer backward reads its
        # 1-wide rows as they are; a strided column of a padded buffer cost the loss ~2 us)
        return kernels.ppo_loss_fwd_bwd(mean, sigma, value, *stored, grad_mu=g_mean, grad_sigma=g_sigma, **u.loss_kw)

    def _manual_minibatch(self, u, mb):
        """Forward, fused loss and backward without autograd; the gradients land in the arena (ppo.py:246-253 forward,
        :221-223 + :259-315 loss, :367-368 backward)."""
        arena, dev = u.arena, u.dev
        with torch.no_grad():
            side = fused_mlp.side_stream(dev)  # a second stream for the critic's launches (RSLRL_TWO_STREAMS=1)
            vh, ah = self._loss_heads(u, mb.stored)
            mean, sigma, value, tape = self.policy.train_forward(mb.obs, side_stream=side, value_head=vh,
                                                                 actor_head=ah)
            stats, g_mean, g_sigma, g_value = self._loss_after_forward(u, ah, mean, sigma, value, mb.stored)
            on_early = None
            if self.is_multi_gpu and arena.early_numel:
                def on_early(buf=arena.flat[:arena.early_numel], work=u.early_work):
                    # the early prefix's gradients are enqueued: its all-reduce starts now and overlaps the first
                    # layers' backward (the collective's stream waits for this point of ours)
                    work.append(torch.distributed.all_reduce(buf, op=torch.distributed.ReduceOp.SUM, async_op=True))
            self.policy.train_backward(tape, g_mean, g_sigma, g_value, sigma, arena.slot, side_stream=side,
                                       on_early=on_early)
        return stats

    def _recurrent_minibatch(self, u, mb):
        """One env-major sequence of RolloutStorage.recurrent_sequence_generator without autograd: T
        paired LSTM launches into the tape allocated at the first mini-batch, the manual path's MLP pair, heads and loss
        over the [T * E, ...] rows, T paired reverse launches and the gate blocks' weight gradients; every gradient in
        the arena.  The slice's normalised observations and row views are made once per update."""
        pol = self.policy
        T, E = mb.masks.shape
        with torch.no_grad():
            if mb.index not in u.flat_fields:  # once per mini-batch slice (every epoch walks the same slices)
                x_a = pol.actor_obs_normalizer(pol.get_actor_obs(mb.obs)).contiguous()
                x_c = pol.critic_obs_normalizer(pol.get_critic_obs(mb.obs)).contiguous()
                u.flat_fields[mb.index] = (tuple(t.reshape(T * E, *t.shape[2:]) for t in mb.stored), x_a, x_c)
            stored, x_a, x_c = u.flat_fields[mb.index]
            if u.seq is None:
                u.seq = pol.train_tape(T, E, u.dev)
            vh, ah = self._loss_heads(u, stored)
            mean, sigma, value, tape = pol.train_forward(x_a, x_c, mb.masks, *mb.hid_states, u.seq, value_head=vh,
                                                         actor_head=ah)
            stats, g_mean, g_sigma, g_value = self._loss_after_forward(u, ah, mean, sigma, value, stored)
            pol.train_backward(tape, g_mean, g_sigma, g_value, sigma, u.arena.slot, u.seq)
        return stats

    def _autograd_minibatch(self, u, mb):
        """The autograd path for any other policy (ppo.py:246-253, :367-372), recurrent ones included."""
        pol, recurrent, stored = self.policy, bool(self.policy.is_recurrent), mb.stored
        if recurrent and hasattr(pol, "action_distribution_params"):
            mean, sigma = pol.action_distribution_params(mb.obs, masks=mb.masks, hidden_states=mb.hid_states[0])
        elif hasattr(pol, "action_distribution_params"):
            mean, sigma = pol.action_distribution_params(mb.obs)
        else:
            pol.act(mb.obs, masks=mb.masks, hidden_states=mb.hid_states[0])
            mean, sigma = pol.action_mean, pol.action_std
        value = pol.evaluate(mb.obs, masks=mb.masks, hidden_states=mb.hid_states[1])
        if recurrent:
            # [T, E, ...] -> [T * E, ...]: means, loss sums, the KL and the lr rule do not depend on the shape
            if sigma.dim() == 3 and sigma.stride(0) == 0 and sigma.stride(1) == 0:
                sigma = sigma[0, 0]  # the shared std behind Normal's expand: reduced by the loss kernel
            elif sigma.dim() != 1:  # (1-D: the shared std itself, reduced by the loss kernel too)
                sigma = sigma.flatten(0, 1)
            mean, value = mean.flatten(0, 1), value.flatten(0, 1)
            if mb.index not in u.flat_fields:  # once per mini-batch slice (every epoch walks the same slices)
                u.flat_fields[mb.index] = tuple(
                    t.reshape(t.shape[0] * t.shape[1], *t.shape[2:]).contiguous() for t in stored)
            stored = u.flat_fields[mb.index]
        stats, g_mean, g_sigma, g_value = kernels.ppo_loss_fwd_bwd(mean, sigma, value, *stored, **u.loss_kw)
        self._autograd_backward(mean, sigma, value, g_mean, g_sigma, g_value)
        return stats

    def _symmetric_minibatch(self, u, mb):
        """One mini-batch with symmetry_cfg set (ppo.py:226-257, :317-348): the observations (and, with
        use_data_augmentation, the actions) are augmented to K blocks of B rows, the actor runs once on all K * B rows
        -- the reference's second, deterministic forward for the mirror term has the same inputs, and both branches add
        their gradients at the mean -- the critic on the rows that carry PPO terms (K * B with augmentation, B
        without), and kernels.ppo_loss_sym_fwd_bwd writes the summed d loss / d mean; the stored fields stay the B
        rows', never repeated, and RND sees the original B rows (ppo.py:356).  On the manual path the MLP passes are
        the paired launches with augmentation, one pass per network without it (different row counts)."""
        sym = self.symmetry
        fn, env = sym["data_augmentation_func"], sym.get("_env")
        augment = bool(sym["use_data_augmentation"])
        coeff = float(sym["mirror_loss_coeff"]) if sym["use_mirror_loss"] else 0.0
        B = mb.obs.batch_size[0]
        with torch.no_grad():
            if augment:
                obs_aug, act_aug = fn(obs=mb.obs, actions=mb.actions, env=env)
            else:
                (obs_aug, _), act_aug = fn(obs=mb.obs, actions=None, env=env), mb.actions
        K = int(obs_aug.batch_size[0] / B)
        act_aug = act_aug if act_aug.is_contiguous() else act_aug.contiguous()
        critic_obs = obs_aug if augment else mb.obs

        def target_kw(mean):
            if K <= 1:
                return {}
            if isinstance(fn, SignedPermutationSymmetry):  # the kernel forms sign * mean[perm] itself
                perm, sign = fn.action_tables(mean.device)
                return dict(act_perm=perm, act_sign=sign)
            with torch.no_grad():  # any other callable: called as the reference calls it (ppo.py:334-337)
                _, tgt = fn(obs=None, actions=mean.detach()[:B], env=env)
            return dict(mirror_target=tgt.detach().to(torch.float32).contiguous())

        kw = dict(u.loss_kw, B=B, k_ppo=K if augment else 1, k_mir=K, mirror_coeff=coeff, symmetry_sum=u.sums[4:5])
        if u.arena is not None:
            with torch.no_grad():
                side = fused_mlp.side_stream(u.dev)
                mean, sigma, value, tape = self.policy.train_forward(
                    obs_aug, side_stream=side, critic_obs=None if augment else critic_obs)
                g_mean, g_sigma = self._loss_grad_buffers(u.arena, mean, sigma)
                stats, g_mean, g_sigma, g_value = kernels.ppo_loss_sym_fwd_bwd(
                    mean, sigma, value, act_aug, *mb.stored[1:], grad_mu=g_mean, grad_sigma=g_sigma,
                    **target_kw(mean), **kw)
                self.policy.train_backward(tape, g_mean, g_sigma, g_value, sigma, u.arena.slot, side_stream=side)
            return stats
        if hasattr(self.policy, "action_distribution_params"):
            mean, sigma = self.policy.action_distribution_params(obs_aug)
        else:
            self.policy.act(obs_aug)
            mean, sigma = self.policy.action_mean, self.policy.action_std
        value = self.policy.evaluate(critic_obs)
        stats, g_mean, g_sigma, g_value = kernels.ppo_loss_sym_fwd_bwd(
            mean, sigma, value, act_aug, *mb.stored[1:], **target_kw(mean), **kw)
        self._autograd_backward(mean, sigma, value, g_mean, g_sigma, g_value)
        return stats

    # ---- the rest of a mini-batch, in update()'s order
    def _rnd_minibatch(self, u, mb):
        """The RND predictor's loss and backward on the mini-batch's rows (ppo.py:352-363, :369-371), fused
        (_rnd_update_plan, decided at the first mini-batch) or under autograd; the statistic accumulates in sums[3]."""
        if not self.rnd:
            return
        arena = u.arena
        if u.rnd_fused is None:
            u.rnd_fused = self._rnd_update_plan(mb.obs, u.rnd_params, arena)
        if u.rnd_fused:
            # one launch pair: predictor forward, detached target (computed in the first epoch, then read from the
            # cache: its weights and inputs do not change within update()), MSE, backward into the arena span
            self._rnd_update_fused(mb.obs, arena.span(u.rnd_params), u.sums, u.target_cache, mb.index)
            return
        with torch.no_grad():
            rnd_state_batch = self.rnd.get_rnd_state(mb.obs)
            rnd_state_batch = self.rnd.state_normalizer(rnd_state_batch)
        predicted_embedding = self.rnd.predictor(rnd_state_batch)
        target_embedding = self.rnd.target(rnd_state_batch).detach()
        rnd_loss = nn.functional.mse_loss(predicted_embedding, target_embedding)
        if arena is None:
            for p in u.rnd_params:
                p.grad = None
        elif u.rnd_params:  # zeroed arena range + autograd's in-place accumulation = fresh gradients
            arena.span(u.rnd_params).zero_()
        rnd_loss.backward()
        u.sums[3] += rnd_loss.detach().double()

    def _reduce_minibatch(self, stats, arena, adaptive, early_work):
        """The collective (ppo.py:271-273, :376): the KL rides in the arena's all-reduce (early_work: the early prefix's
        pending ones, consumed here) or, without an arena, in reduce_parameters'.  Returns where the averaged KL is."""
        kl_src = stats[kernels.STATS_KL:kernels.STATS_KL + 1]
        if not self.is_multi_gpu:
            return kl_src
        if arena is None:
            kl_src = kl_src.clone() if adaptive else None
            self.reduce_parameters(kl_mean=kl_src)
            return kl_src
        if adaptive:
            arena.extra[:1].copy_(kl_src)
        self._all_reduce_arena(arena, with_kl=adaptive, skip=arena.early_numel if early_work else 0,
                               pending=early_work)
        early_work.clear()
        return arena.extra[:1]

    def _lr_rule_and_tail(self, stats, kl_src, adaptive, lr_dev, lr32, sums):
        """The adaptive lr (in the device tail when lr_dev is set, else _host_lr_rule on the averaged KL) and the loss
        sums (ppo.py:259-294, :387-395).  Returns the tail for FusedClipAdam's norm launch, or None: launched here."""
        if lr_dev is not None:  # (only ever set for the adaptive schedule)
            tail = kernels.ppo_tail_args(stats, kl_src, lr_dev, lr32, self.desired_kl, sums,
                                         round_fp32=self.is_multi_gpu)
        else:
            if adaptive:
                self._host_lr_rule(kl_src.item())
            tail = kernels.ppo_tail_args(stats, None, None, None, 0.0, sums)
        if self._clip_adam is not None and _FUSED_TAIL:
            return tail
        kernels.ppo_update_tail_args(tail, sums.device)
        return None

    def _step_optimizers(self, tail, rnd_fused):
        """clip + Adam on the policy (ppo.py:373-374; tail: see _lr_rule_and_tail), Adam on the RND predictor."""
        if self._clip_adam is None:
            nn.utils.clip_grad_norm_(self.policy.parameters(), self.max_grad_norm)
            self.optimizer.step()
        else:
            self._clip_adam.max_grad_norm = float(self.max_grad_norm)
            self._clip_adam.step(tail=tail)
        if self.rnd_optimizer:
            if rnd_fused and self._rnd_adam is not None:
                self._rnd_adam.step()  # the reference's unclipped Adam on the predictor (ppo.py:383-384)
            else:
                self.rnd_optimizer.step()

    def _rnd_update_plan(self, obs_batch, rnd_params, arena) -> bool:
        """Whether the RND predictor's step runs on the fused kernels (kernels.rnd_update): the manual update's
        gradient arena, Linear-ELU-Linear networks of the kernel's sizes, all four predictor parameters trainable
        (their arena span is then [W1 | b1 | W2 | b2]), an identity or empirical state normaliser, fp32 GPU
        observations, our RolloutStorage (its mini-batches are fixed slices of one gathered buffer per update,
        which the target cache relies on)."""
        from ..networks.normalization import EmpiricalNormalization
        rnd = self.rnd
        if arena is None or not isinstance(self.storage, RolloutStorage):
            return False
        pred, targ = kernels.rnd_linears(rnd.predictor), kernels.rnd_linears(rnd.target)
        if pred is None or targ is None:
            return False
        if [(m.in_features, m.out_features) for m in pred] != [(m.in_features, m.out_features) for m in targ]:
            return False
        if len(rnd_params) != 4 or any(a is not b for a, b in zip(rnd_params, [pred[0].weight, pred[0].bias,
                                                                                pred[1].weight, pred[1].bias])):
            return False
        sn = rnd.state_normalizer
        if not isinstance(sn, (nn.Identity, EmpiricalNormalization)):
            return False
        state = self._rnd_state(obs_batch)
        if state is None or not state.is_cuda or state.dtype != torch.float32 or state.shape[1] != pred[0].in_features:
            return False
        if self._rnd_adam is not None:
            self._rnd_adam.adopt_loaded_state()
        return True

    def _rnd_state(self, obs_batch):
        """The RND state of a mini-batch (rnd.py get_rnd_state) without a copy when it is one observation group."""
        groups = self.rnd.obs_groups["rnd_state"]
        if len(groups) == 1:
            s = obs_batch[groups[0]]
            return s if s.dim() == 2 and s.stride(1) == 1 else None
        return self.rnd.get_rnd_state(obs_batch)

    def _rnd_update_fused(self, obs_batch, grad_span, sums, target_cache, slice_index):
        """slice_index: the mini-batch's slice of the update's permutation (its index within the epoch).  The cache
        is keyed by it, not by the state's address: with several rnd_state groups the state is a fresh torch.cat per
        mini-batch, and the caching allocator hands the next mini-batch's cat the same address."""
        rnd = self.rnd
        state = self._rnd_state(obs_batch)
        B = state.shape[0]
        pred, targ = kernels.rnd_linears(rnd.predictor), kernels.rnd_linears(rnd.target)
        key = (slice_index, B)
        temb = target_cache.get(key)
        compute_target = temb is None
        if compute_target:
            temb = torch.empty(B, targ[1].out_features, dtype=torch.float32, device=state.device)
            target_cache[key] = temb
        kw = {}
        if rnd.state_normalization:
            sn = rnd.state_normalizer
            kw = dict(state_mean=sn._mean.reshape(-1), state_std=sn._std.reshape(-1), state_eps=sn.eps)
        kernels.rnd_update(state, pred, targ if compute_target else None, temb, grad_span, loss_sum=sums[3:4], **kw)

    def _optimizer_takes_tensor_lr(self) -> bool:
        d = self.optimizer.defaults
        return bool(d.get("fused") or d.get("capturable"))

    # ------------------------------------------------------------------ multi-GPU (ppo.py:428-469)
    def broadcast_parameters(self):
        """Broadcast model parameters from rank 0 to all ranks."""
        model_params = [self.policy.state_dict()]
        if self.rnd:
            model_params.append(self.rnd.predictor.state_dict())
        torch.distributed.broadcast_object_list(model_params, src=0)
        self.policy.load_state_dict(model_params[0])
        if self.rnd:
            self.rnd.predictor.load_state_dict(model_params[1])

    def _all_reduce_arena(self, arena: GradArena, with_kl: bool, skip: int = 0, pending=()):
        """The gradient collective per mini-batch (arena.all_reduce_arena at this world size)."""
        all_reduce_arena(arena, self.gpu_world_size, with_kl, skip, pending)

    def reduce_parameters(self, kl_mean: torch.Tensor | None = None):
        """Average gradients across ranks: SUM all-reduce then / world_size (ppo.py:441-469; arena.reduce_gradients),
        in place on the arena where the gradients are its views, otherwise the reference's concatenation (policy,
        then RND) / all-reduce / copy-back.  kl_mean: an optional fp32 1-element tensor appended to it (averaged)."""
        cat_params = chain(self.policy.parameters(), self.rnd.parameters()) if self.rnd else self.policy.parameters()
        reduce_gradients(self._arena, self._trainable_params(), cat_params, self.gpu_world_size, kl_mean)
