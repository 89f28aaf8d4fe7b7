"""Distillation: behaviour cloning of a frozen teacher by a student MLP (rsl_rl/algorithms/distillation.py:14-185).

Constructor, attributes (policy, optimizer, storage, transition, learning_rate, num_updates, ...) and methods
(init_storage, act, process_env_step, update, broadcast_parameters, reduce_parameters) keep the reference's
signatures and semantics.  What changes is how update() evaluates the reference's schedule
(distillation.py:105-151): there, every stored step runs its own small student forward, an mse_loss and a `.item()`
host read-back, and every `gradient_length` steps one autograd backward runs through that many chained graphs.  For
a feed-forward student the steps of such a window are independent rows, so one optimizer step is exactly

    one forward over the window's gradient_length * N rows  (networks/fused_mlp.train_forward; the rows are one
                                                              flattened view of the [T, N, .] storage)
    one loss launch                                           (kernels.bc_loss: every step's mean and d loss / d output)
    one backward                                              (fused_mlp.train_backward into a flat gradient arena)
    [one all-reduce of the arena / world size]                (multi-GPU)
    clip + Adam in two launches                               (kernels.FusedClipAdam)

and the whole update() reads the device once, at its end (the per-step losses).  `distillation_windows` is that
schedule as a pure function.  The student may be any stack train_forward / train_backward take
(fused_mlp.window_trainable): a fusable ELU stack, a wide one (hidden widths up to 1024, [512, 256, 128]) or one whose
observation width is no multiple of 4 (45, 235: the first layer on the ragged kernels, its rows read in place and its
[dW | db] written straight into the arena) -- the last two in x6 arithmetic and with RSLRL_WIDE_MLP / RSLRL_RAGGED_INPUT
not 0.  RSLRL_DISTILL_FUSED=0 -- and any other student -- keeps the reference's per-step loop: autograd
through policy.act_inference with kernels.bc_loss as the loss (kernels.BCLossFunction).

A recurrent student (modules/student_teacher_recurrent.StudentTeacherRecurrent).  Given the memory's outputs h_t, the
MLP over a window's rows is independent rows again, so for a one-layer LSTM or GRU of width 256 (what kernels.lstm_cell /
kernels.gru_cell take) the window is batched too (_update_fused_recurrent, written once over the kind, a kernels.Cell;
DESIGN.md §24): G cell_train launches (_window_forward: resets applied on read from the stored dones, the activated
gates kept -- i, f, g, o or r, z, n, a --, a GRU's h as consumed taken from the cell, an LSTM's composed on the host),
the MLP's forward / loss / backward over the [G * N, 256] view of the stored h (_mlp_step, shared with _update_fused;
the MLP may be wide), G cell_bwd launches in reverse (_window_backward: the chain cut at an epoch start inside the
window, recurrent_window_plan), and the gate blocks' weight gradients over the window's rows into the same arena
(fused_mlp.lstm_gate_wgrads / gru_gate_wgrads, the recurrent PPO update's, here with one memory).  Any other
memory (other hidden sizes, several layers, N not a multiple of 64), RSLRL_LSTM_CELL=0 / RSLRL_GRU_CELL=0 for the
respective kind and RSLRL_DISTILL_FUSED=0 take the per-step loop, whose backward through time runs under autograd (the
RNN library for the memory, the fused MLP path behind it).  On both, the clip spans the student MLP only, as the
reference's (distillation.py:134), through FusedClipAdam's clipped set; the memory's gradients are stepped unclipped.
A policy that says is_recurrent without being a StudentTeacherRecurrent is refused.

The rollout step's storage row (process_env_step -> add_transitions: a copy per observation group plus four) goes out in
one launch (RolloutStorage.add_transition_distill, csrc/distill_record.hip) where the sources can be read in place, up
to DISTILL_RECORD_MAX_ROWS envs; RSLRL_DISTILL_RECORD=0 keeps the copies, =1 takes the launch at any size.
"""

from __future__ import annotations

import os
from types import SimpleNamespace

import torch
import torch.nn as nn

from .. import kernels
from ..modules.student_teacher import StudentTeacher
from ..modules.student_teacher_recurrent import StudentTeacherRecurrent
from ..networks import fused_mlp
from ..storage import RolloutStorage
from ..utils import resolve_optimizer
from .arena import GradArena, reduce_gradients


# The rollout step's storage row goes out in one launch (kernels.distill_record) up to this many envs: there the step is
# launch-bound and one launch in place of the five or more copies saves host time; above, the step is bound by the GPU,
# where torch's copies move the same bytes no slower (scripts/distill_default_probe.py, profiles/distill_default_probe
# .json; the figures are in DESIGN.md §23).  RSLRL_DISTILL_RECORD=1 takes the launch at any size, =0 never.
DISTILL_RECORD_MAX_ROWS = 8192


def distillation_windows(T: int, E: int, G: int):
    """The optimizer schedule of one update() (distillation.py:105-151) over seq = [(e, t) for e < E for t < T]:
    consecutive runs of G entries, each a full window that gets one optimizer step (a window may span the epoch
    boundary: the reference's step counter runs on across epochs and restarts at every update()), and at most one
    trailing window shorter than G whose losses only feed the statistic (the reference never takes its gradient).
    Returns [(steps, full)] with `steps` the window's storage step indices t in order; with E * T < G there is no
    full window at all."""
    if T < 1 or E < 1 or G < 1:
        raise ValueError(f"distillation_windows: T, E and G must be positive, got {(T, E, G)}")
    seq = [t for _ in range(E) for t in range(T)]
    return [(tuple(seq[i:i + G]), len(seq[i:i + G]) == G) for i in range(0, len(seq), G)]


def recurrent_window_plan(steps):
    """Where the backward-through-time chain of a window's steps is cut: [(t, starts, chained)] per step, `starts`
    when the step begins an epoch (t == 0: the state restarts from last_hidden_states, distillation.py:112-113) and
    `chained` when the next step of the window continues from this one's state (it exists and does not start an
    epoch).  Resets by dones do not cut the schedule: they zero rows, which the kernels do from the reset vectors."""
    return [(t, t == 0, k + 1 < len(steps) and steps[k + 1] != 0) for k, t in enumerate(steps)]


def _runs(steps):
    """Maximal runs of consecutive step indices: [(first, last + 1)]."""
    runs, start = [], 0
    for i in range(1, len(steps) + 1):
        if i == len(steps) or steps[i] != steps[i - 1] + 1:
            runs.append((steps[start], steps[i - 1] + 1))
            start = i
    return runs


class Distillation:
    """Distillation algorithm for training a student model to mimic a teacher model."""

    policy: StudentTeacher

    def __init__(
        self,
        policy,
        num_learning_epochs=1,
        gradient_length=15,
        learning_rate=1e-3,
        max_grad_norm=None,
        loss_type="mse",
        optimizer="adam",
        device="cpu",
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
        self.rnd = None  # the runner's logging / checkpoint code asks (PPO may carry an RND module)

        self.policy = policy
        self.policy.to(self.device)
        self.storage: RolloutStorage = None  # type: ignore

        on_gpu = str(device).startswith("cuda")
        opt_cls = resolve_optimizer(optimizer)
        if opt_cls is torch.optim.Adam:  # fused on a ROCm device, as PPO's
            self.optimizer = opt_cls(self.policy.parameters(), lr=learning_rate, fused=True if on_gpu else None)
        else:
            self.optimizer = opt_cls(self.policy.parameters(), lr=learning_rate)
        # clip_grad_norm_ + optimizer.step() as two launches (distillation.py:133-135); parameters without a gradient
        # (std, the teacher) are skipped, as torch's Adam skips them.  The norm spans policy.student.parameters() only
        # (distillation.py:134): a recurrent student's memory is stepped with its gradient unclipped
        student = getattr(self.policy, "student", None)
        # a recurrent pair's optimizer also holds the frozen teacher and its memory, which never carry a gradient:
        # the fused step's tensor limit counts the student's memory and MLP (other policies: every parameter, as before)
        trained = None
        if isinstance(self.policy, StudentTeacherRecurrent):
            trained = list(self.policy.memory_s.parameters()) + list(self.policy.student.parameters())
        self._clip_adam = (kernels.FusedClipAdam(self.optimizer, max_grad_norm,
                                                 clip_params=None if student is None else list(student.parameters()))
                           if on_gpu and kernels.FusedClipAdam.supported(self.optimizer, trained) else None)

        self.transition = RolloutStorage.Transition()
        self.last_hidden_states = None

        self.num_learning_epochs = num_learning_epochs
        self.gradient_length = gradient_length
        self.learning_rate = learning_rate
        self.max_grad_norm = max_grad_norm

        loss_types = ("mse", "huber")  # nn.functional.mse_loss / huber_loss, evaluated by kernels.bc_loss
        if loss_type not in loss_types:
            raise ValueError(f"Unknown loss type: {loss_type}. Supported types are: {list(loss_types)}")
        self.loss_type = loss_type

        self.num_updates = 0
        self._arena: GradArena | None = None
        self.last_step_losses: list = []  # the E * T per-step losses of the latest update(), in schedule order

    def init_storage(self, training_type, num_envs, num_transitions_per_env, obs, actions_shape):
        self.storage = RolloutStorage(training_type, num_envs, num_transitions_per_env, obs, actions_shape,
                                      self.device)

    # ------------------------------------------------------------------ rollout (distillation.py:85-103)
    def act(self, obs):
        pcls = type(self.policy)
        base = next((c for c in (StudentTeacher, StudentTeacherRecurrent) if isinstance(self.policy, c)), None)
        if base is not None and pcls.act is base.act and pcls.evaluate is base.evaluate:
            actions, privileged = self.policy.act_and_evaluate(obs)  # the same values and draws, paired launches
        else:
            actions, privileged = self.policy.act(obs), self.policy.evaluate(obs)
        self.transition.actions = actions.detach()
        self.transition.privileged_actions = privileged.detach()
        self.transition.observations = obs
        return self.transition.actions

    def process_env_step(self, obs, rewards, dones, extras):
        self.policy.update_normalization(obs)
        self.transition.rewards = rewards
        self.transition.dones = dones
        # one launch for the step's row (storage.add_transition_distill) where the sources can be read in place and the
        # step is launch-bound (DISTILL_RECORD_MAX_ROWS; RSLRL_DISTILL_RECORD=1 takes it at any size);
        # RSLRL_DISTILL_RECORD=0 and anything else keep the per-field copies
        knob = os.environ.get("RSLRL_DISTILL_RECORD")
        if (knob != "0" and (knob == "1" or self.storage.num_envs <= DISTILL_RECORD_MAX_ROWS)
                and self.storage.distill_record_ok(self.transition)):
            self.storage.add_transition_distill(self.transition)
        else:
            self.storage.add_transitions(self.transition)
        self.transition.clear()
        self.policy.reset(dones)

    # ------------------------------------------------------------------ update (distillation.py:105-151)
    def _student_params(self):
        return [p for p in self.policy.student.parameters() if p.requires_grad]

    def grad_arena(self) -> GradArena:
        """One flat gradient buffer behind the student's parameters -- a recurrent student's memory first, then its
        MLP -- (their .grad are views of it): the multi-GPU all-reduce is one call on it, without the reference's
        cat / copy-back."""
        params = self._student_params()
        if isinstance(self.policy, StudentTeacherRecurrent):
            params = [p for p in self.policy.memory_s.rnn.parameters() if p.requires_grad] + params
        if self._arena is None or not self._arena.matches(params) or self._arena.flat.device != params[0].device:
            self._arena = GradArena(params, extra=0, device=params[0].device)
        return self._arena

    def _fused_common(self, base, mlp_width=None) -> int:
        """What both window-batched updates need: the knob, an optimizer FusedClipAdam takes, an unmodified `base`
        policy, fp32 [T, N, .] observations on a ROCm device and a student MLP that fused_mlp.window_trainable takes (no
        Unflatten) at its input width, mlp_width(policy) or else the observations' -- a fusable stack, or a wide or a
        ragged one where those run fused (their flags on the MLP, x6 arithmetic).  Returns that width, or 0."""
        if os.environ.get("RSLRL_DISTILL_FUSED", "1") == "0" or self._clip_adam is None:
            return 0
        pol = self.policy
        if not isinstance(pol, base) or type(pol).act_inference is not base.act_inference:
            return 0
        groups = pol.obs_groups["policy"]
        obs = self.storage.observations
        if not all(obs[g].is_cuda and obs[g].dtype == torch.float32 and obs[g].dim() == 3 for g in groups):
            return 0
        width = sum(obs[g].shape[-1] for g in groups)
        student = pol.student
        form = fused_mlp.window_trainable(student, mlp_width(pol) if mlp_width else width)
        # a wide or ragged stack runs fused in x6 arithmetic only, and its knob keeps it on the per-step path
        if form == "fused":
            ok = getattr(student, "_fused", False)
        elif form == "wide":
            ok = getattr(student, "_wide", False) and fused_mlp.wide_enabled()
        elif form == "ragged":
            ok = (getattr(student, "_ragged", False) and fused_mlp.ragged_enabled()
                  and (fused_mlp.wide_enabled() or not fused_mlp.ragged_wide_stack(student)))
        else:
            ok = False
        return width if ok else 0

    def _fused_ok(self) -> bool:
        """The window-batched update applies: _fused_common for a StudentTeacher, every student parameter trainable."""
        return self._fused_common(StudentTeacher) > 0 and all(p.requires_grad for p in self.policy.student.parameters())

    def _fused_recurrent_ok(self) -> bool:
        """The window-batched recurrent update applies: _fused_common for a StudentTeacherRecurrent, a student memory
        that is a one-layer LSTM or GRU the fused cell takes at this number of envs and observation width (its knob,
        RSLRL_LSTM_CELL / RSLRL_GRU_CELL, not 0), a stored state of its form -- (h, c) for an LSTM, the bare tensor for
        a GRU -- and every parameter of memory and MLP trainable."""
        width = self._fused_common(StudentTeacherRecurrent, lambda pol: pol.memory_s.rnn.hidden_size)
        if not width:
            return False
        rnn = self.policy.memory_s.rnn
        cell = kernels.cell_of(rnn)
        if (cell is None or not rnn.bias or rnn.bidirectional or rnn.input_size != width or rnn.proj_size != 0
                or not cell.enabled()
                or not cell.supported(self.storage.num_envs, width, rnn.hidden_size, rnn.num_layers)):
            return False
        last = self.last_hidden_states
        if last is not None and last[0] is not None:
            stored = last[0]
            if not (isinstance(stored, torch.Tensor) if cell.n_state == 1
                    else isinstance(stored, tuple) and len(stored) == cell.n_state):
                return False
        return all(p.requires_grad for m in (rnn, self.policy.student) for p in m.parameters())

    def _window_rows(self, steps):
        """(student observations [S*N, O], teacher actions [S*N, A]) of a window's steps: flattened views of the
        storage for one observation group and consecutive steps, else one torch.cat."""
        st = self.storage
        groups = self.policy.obs_groups["policy"]
        runs = _runs(steps)

        def rows(buf):
            parts = [buf[a:b].flatten(0, 1) for a, b in runs]
            return parts[0] if len(parts) == 1 else torch.cat(parts, dim=0)

        obs = rows(st.observations[groups[0]]) if len(groups) == 1 else torch.cat(
            [rows(st.observations[g]) for g in groups], dim=-1)
        target = rows(st.privileged_actions)
        return obs, target if target.is_contiguous() else target.contiguous()

    def _reduce_and_step(self):
        """The multi-GPU average, the clip over the student MLP and the optimizer step (distillation.py:131-135)."""
        if self.is_multi_gpu:
            self.reduce_parameters()
        if self._clip_adam is not None:
            self._clip_adam.max_grad_norm = float(self.max_grad_norm) if self.max_grad_norm else 0.0
            self._clip_adam.step()
        else:
            if self.max_grad_norm:
                nn.utils.clip_grad_norm_(self.policy.student.parameters(), self.max_grad_norm)
            self.optimizer.step()

    def update(self):
        if self.policy.is_recurrent and not isinstance(self.policy, StudentTeacherRecurrent):
            # StudentTeacherRecurrent's hidden-state protocol (reset / detach_hidden_states / get_hidden_states with a
            # (student, teacher) pair) is the one the loop below follows; another recurrent policy's is unknown
            raise NotImplementedError(
                "recurrent policies other than StudentTeacherRecurrent (the hidden-state handling of "
                "rsl_rl/algorithms/distillation.py:112-113, :136-141, :145-146 follows "
                "rsl_rl/modules/student_teacher_recurrent.py) are outside this build's scope")
        self.num_updates += 1
        if self._clip_adam is not None:
            self._clip_adam.adopt_loaded_state()  # a checkpoint of a non-fused Adam may have been loaded
        T, E, G = self.storage.num_transitions_per_env, self.num_learning_epochs, self.gradient_length
        if self._fused_ok():
            losses = self._update_fused(T, E, G)
        elif self._fused_recurrent_ok():
            losses = self._update_fused_recurrent(T, E, G)
        else:
            losses = self._update_per_step(T, E, G)
        # the one read-back of update(): the reference's `mean_behavior_loss += behavior_loss.item()` (Python floats,
        # in schedule order), then / cnt
        self.last_step_losses = losses.tolist()
        mean_behavior_loss = 0.0
        for v in self.last_step_losses:
            mean_behavior_loss += v
        mean_behavior_loss /= len(self.last_step_losses)
        self.storage.clear()
        self.last_hidden_states = self.policy.get_hidden_states()
        self.policy.detach_hidden_states()
        return {"behavior": mean_behavior_loss}

    # ---- what the two window-batched updates share
    def _bind_fused(self):
        """The bound arena (optimizer.zero_grad() for what it does not back) and the student MLP as (weights, biases,
        their (dW, db) arena slots)."""
        lin = [m for m in self.policy.student if isinstance(m, nn.Linear)]
        ws, bs = [m.weight for m in lin], [m.bias for m in lin]
        arena = self.grad_arena()
        arena.bind()
        for p in self.policy.parameters():
            if id(p) not in arena._slot:
                p.grad = None
        return arena, (ws, bs, [(arena.slot(w), arena.slot(b)) for w, b in zip(ws, bs)])

    def _windows(self, T, E, G, losses):
        """Per window of the schedule: (steps, full, normalised observation rows, teacher actions, its `losses`)."""
        done = 0
        for steps, full in distillation_windows(T, E, G):
            obs, target = self._window_rows(steps)
            x = self.policy.student_obs_normalizer(obs)
            x = x if x.is_contiguous() else x.contiguous()
            if x.shape[1] % 4:
                # a ragged width: the first layer's forward and its weight gradient read these rows in place.  A window
                # of the storage starts at a multiple of N * O floats (16-byte aligned whenever N % 4 == 0), a window
                # across the epoch boundary is a torch.cat and a normaliser's output an allocation of its own; any
                # other start is realigned here, once, and counted in fused_mlp.ragged_realign_copies
                x = fused_mlp._aligned_rows(x)
            yield steps, full, x, target, losses[done:done + len(steps)]
            done += len(steps)

    def _mlp_step(self, x, target, out, mlp, gbuf, need_dx=False):
        """Forward, loss and backward of the student MLP over a full window's rows x, into the arena; gbuf: d loss /
        d output, zero-padded to 4 columns (train_backward's dy_padded operand).  Returns d loss / d x when asked."""
        ws, bs, outs = mlp
        A, padded = target.shape[-1], gbuf.shape[1]
        y, tape = fused_mlp.train_forward(x, ws, bs)
        kernels.bc_loss(y, target, self.storage.num_envs, self.loss_type, out, grad_out=gbuf)
        dy = gbuf if padded == A else gbuf[:, :A]
        return fused_mlp.train_backward(tape, dy, need_dx=need_dx, outs=outs,
                                        dy_padded=gbuf if padded != A else None)[0]

    def _update_fused(self, T, E, G):
        pol, N, A = self.policy, self.storage.num_envs, self.storage.privileged_actions.shape[-1]
        dev = self.storage.privileged_actions.device
        _, mlp = self._bind_fused()
        losses = torch.empty(E * T, dtype=torch.float32, device=dev)
        gbuf = None
        with torch.no_grad():
            for steps, full, x, target, out in self._windows(T, E, G, losses):
                if not full:
                    # the trailing window: its losses feed the statistic, its gradient is never taken
                    # (distillation.py:123-128: the reference drops it with `loss = 0` at the next update())
                    kernels.bc_loss(pol.student(x), target, N, self.loss_type, out)
                    continue
                if gbuf is None:
                    gbuf = torch.empty(G * N, A + (-A) % 4, dtype=torch.float32, device=dev)
                self._mlp_step(x, target, out, mlp, gbuf)
                self._reduce_and_step()
        return losses

    # ---- the recurrent one, written once over the kind of the student's memory (a kernels.Cell)
    def _window_forward(self, cell, w, x, plan, full, state, first, dones):
        """The window's cell_train launches from `state` (a tuple of cell.n_state [N, 256] tensors or None; `first` at an
        epoch start): a row whose previous step was done (reset = dones[t - 1]) restarts from zero inside the cell.  A
        full window keeps the h as consumed, dW_hh's operand and a GRU's reverse step's: the GRU's cell writes it
        (h_in_out), the LSTM's is composed here (cell.window_hin_from_cell), as is "no state at all".  Returns the
        backward's tape -- per step the record kernels' *_operands take -- and the end state."""
        N, rnn = self.storage.num_envs, self.policy.memory_s.rnn
        image = cell.image(rnn.weight_ih_l0, rnn.weight_hh_l0)
        tape = []
        for k, (t, starts, _) in enumerate(plan):
            reset = None if starts else dones[t - 1]
            if starts:
                state = first
            hin = w.hin[k] if full else None
            from_cell = full and cell.window_hin_from_cell and state is not None
            if full and not from_cell:  # the state as consumed (reset rows zero)
                if state is None:
                    hin.zero_()
                elif reset is None:
                    hin.copy_(state[0])
                else:
                    torch.mul(state[0], reset.view(N, 1) == 0, out=hin)
            step = (state, tuple([o[k] for o in w.out]), reset, None, hin)
            cell.train(cell.train_operands(x[k * N:(k + 1) * N], image, rnn.bias_ih_l0, rnn.bias_hh_l0,
                                           w.gates[:, k], step, hin if from_cell else None))
            tape.append(step)
            state = step[1]
        return tape, state

    def _window_backward(self, cell, w, dh, plan, tape):
        """The window's cell_bwd launches in reverse from dh [G, N, H] with the two alternating carries (an LSTM's d c,
        a GRU's dhz), the chain cut where the plan says so (a done row is cut inside the cell, from the reset vectors)."""
        whh_t = cell.whh_t_image(self.policy.memory_s.rnn.weight_hh_l0)
        for k in range(len(plan) - 1, -1, -1):
            chained = plan[k][2]
            cell.bwd(cell.bwd_operands(dh[k], w.gates[:, k], tape[k], w.dg[:, k + 1] if chained else None,
                                       w.dc[(k + 1) & 1] if chained else None, tape[k + 1][2] if chained else None,
                                       whh_t, w.dg[:, k], w.dc[k & 1]))

    def _update_fused_recurrent(self, T, E, G):
        """The window-batched update of an LSTM or a GRU student (the module docstring's pipeline), one body for both
        kinds: the state is a tuple of [N, 256] tensors ((h, c) or (h,)).
        Per full window: the cell's forward -> the MLP's forward, loss and backward over the [G * N, 256] view of the
        stored h, down to d loss / d h -> the cell's backward -> the gate blocks' weight gradients -> the optional
        all-reduce, clip (the MLP only) and Adam.  A trailing window runs the forward and the loss; the end state goes
        to the policy as the reference's replay leaves it."""
        pol, st = self.policy, self.storage
        N, H = st.num_envs, kernels.LSTM_CELL_HIDDEN
        A = st.privileged_actions.shape[-1]
        f32 = dict(dtype=torch.float32, device=st.privileged_actions.device)
        rnn = pol.memory_s.rnn
        cell = kernels.cell_of(rnn)
        arena, mlp = self._bind_fused()
        losses = torch.empty(E * T, **f32)
        # the window's tape (per step the state leaving it, the h as consumed and the four activated gate tensors -- an
        # LSTM's i, f, g, o, a GRU's r, z, n, a), the gate gradients, the two alternating carries (an LSTM's d c, a
        # GRU's dhz) and the gate-block views of the memory's arena slots (dW_ih, dW_hh, db_ih, db_hh)
        w = SimpleNamespace()
        w.out = tuple(torch.empty(G, N, H, **f32) for _ in range(cell.n_state))
        w.hout, w.hin = w.out[0], torch.empty(G, N, H, **f32)
        w.gates, w.dg = torch.empty(4, G, N, H, **f32), torch.empty(4, G, N, H, **f32)
        w.dc = [torch.empty(N, H, **f32) for _ in range(2)]
        grads = fused_mlp.gate_grad_views(cell, rnn, arena.slot)
        gbuf = torch.empty(G * N, A + (-A) % 4, **f32)
        dones = st.dones.view(-1, N)[:T]
        last = cell.unpack(self.last_hidden_states[0] if self.last_hidden_states is not None else None)
        first = None if last is None else tuple(s.detach().reshape(N, H).contiguous() for s in last)
        state = None
        with torch.no_grad():
            for steps, full, x, target, out in self._windows(T, E, G, losses):
                S = len(steps)
                plan = recurrent_window_plan(steps)
                tape, state = self._window_forward(cell, w, x, plan, full, state, first, dones)
                if full:
                    dh = self._mlp_step(w.hout.view(G * N, H), target, out, mlp, gbuf, need_dx=True)
                    self._window_backward(cell, w, dh.view(G, N, H), plan, tape)
                    # the gate blocks' weight gradients over the whole window's rows into the arena: the PPO update's
                    fused_mlp.GATE_WGRADS[cell.name]([w.dg.view(4, G * N, H)], [x.view(G * N, -1)],
                                                     [w.hin.view(G * N, H)], [grads])
                    self._reduce_and_step()
                else:  # the trailing window: its losses feed the statistic, its gradient is never taken
                    kernels.bc_loss(pol.student(w.hout[:S].view(S * N, H)), target, N, self.loss_type, out)
                # the next window continues from this one's last state, which the tape is about to overwrite
                state = tuple(o[S - 1].clone() for o in w.out)
        # what the reference's replay leaves in the policy: the student's end state with the last step's done rows
        # zeroed; the teacher's memory, never advanced, with the rows of every env that was done zeroed
        gone = (dones[T - 1] != 0).view(1, N, 1)
        pol.memory_s.hidden_states = cell.pack(tuple(torch.where(gone, 0.0, s.unsqueeze(0)) for s in state))
        if pol.teacher_recurrent:
            t_last = self.last_hidden_states[1] if self.last_hidden_states is not None else None
            if t_last is not None:  # (both memories are built from one rnn_type: the teacher's state has the same form)
                ever = (dones != 0).any(dim=0).view(1, N, 1)
                t_last = cell.pack(tuple(torch.where(ever, 0.0, s.detach()) for s in cell.unpack(t_last)))
            pol.memory_t.hidden_states = t_last
        return losses

    def _update_per_step(self, T, E, G):
        """The reference's loop (distillation.py:107-141) with kernels.bc_loss behind autograd as the loss; the
        per-step losses stay on the device until the end of update().  For a StudentTeacherRecurrent this is the
        backward through time of the reference: every epoch restarts from last_hidden_states, done rows are zeroed
        after the step's output has been used (Memory.reset's masked_fill_ stays on the autograd tape, and
        detach_hidden_states(dones) cuts the done rows off it), and no gradient crosses a reset, a window end or an
        epoch start.  None of it reads the device back."""
        step_losses = []
        loss = 0
        cnt = 0
        for _ in range(E):
            self.policy.reset(hidden_states=self.last_hidden_states)
            self.policy.detach_hidden_states()
            for obs, _, privileged_actions, dones in self.storage.generator():
                actions = self.policy.act_inference(obs)
                behavior_loss = kernels.BCLossFunction.apply(actions, privileged_actions, self.loss_type)
                loss = loss + behavior_loss
                step_losses.append(behavior_loss.detach())
                cnt += 1
                if cnt % G == 0:
                    self.optimizer.zero_grad()
                    loss.backward()
                    self._reduce_and_step()
                    self.policy.detach_hidden_states()
                    loss = 0
                self.policy.reset(dones.view(-1))
                self.policy.detach_hidden_states(dones.view(-1))
        return torch.stack(step_losses)

    # ------------------------------------------------------------------ multi-GPU (distillation.py:157-185)
    def broadcast_parameters(self):
        """Broadcast model parameters from rank 0 to all ranks."""
        model_params = [self.policy.state_dict()]
        torch.distributed.broadcast_object_list(model_params, src=0)
        self.policy.load_state_dict(model_params[0])

    def reduce_parameters(self):
        """Average gradients across ranks: SUM all-reduce then / world_size (distillation.py:166-185), in place on the
        arena where the gradients are its views, otherwise the reference's concatenation (arena.reduce_gradients)."""
        with_grad = [p for p in self.policy.parameters() if p.grad is not None]
        reduce_gradients(self._arena, with_grad, with_grad, self.gpu_world_size)
