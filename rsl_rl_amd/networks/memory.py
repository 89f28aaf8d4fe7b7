"""Recurrent memory of a policy (rsl_rl/networks/memory.py:13-70).

nn.LSTM / nn.GRU hold the parameters, so state_dict keys (rnn.weight_ih_l0, ...) and checkpoints are the
reference's.  Two things differ in how it runs, not in what it computes:

* reset(dones) / detach_hidden_states(dones) never index with a boolean mask (on a GPU that is a nonzero and a
  host read-back per env step): done rows are set with masked_fill_ / torch.where -- exactly 0.0, as the reference;
* in batch mode the sequence output is unpadded through utils.unpad_trajectories, which on a ROCm device follows
  the trajectory index map that RolloutStorage.recurrent_mini_batch_generator attached to the masks (one gather
  kernel, the scatter as its backward); a hand-made bool mask takes the reference's boolean indexing;
* a one-layer LSTM of hidden size 256 takes its rollout steps (no autograd, a ROCm device, an input width from 1 to
  1024 -- a multiple of 16 up to 256 with RSLRL_RNN_ANY_INPUT=0, DESIGN.md §22 --, a multiple of 64 rows) on the fused
  cell kernel (kernels.lstm_cell: one launch per step instead of
  the RNN library's several).  Memory.forward's batch mode stays on nn.LSTM under autograd; the PPO update of a
  policy whose two memories qualify does not call it (ActorCriticRecurrent.train_forward).
  RSLRL_LSTM_CELL=0 keeps nn.LSTM everywhere.  The cell's weight image is built per call, or once per
  fused_mlp.frozen_weights() scope (the runner's rollout): the fused Adam step writes parameters without moving
  their version counters, so versions alone cannot tell whether an image is stale.
* a one-layer GRU of hidden size 256 takes the same steps, under the same conditions, on the fused GRU cell
  (kernels.gru_cell, gru_cell_ok); hidden_states stays the bare [1, M, 256] tensor.  cell_ok keeps its
  meaning -- the fused LSTM cell -- and is False for a GRU.  RSLRL_GRU_CELL=0 keeps nn.GRU everywhere; batch mode stays
  on nn.GRU under autograd, and the PPO update of a policy whose two GRUs qualify does not call it.
* distillation: a student memory of either kind that qualifies is trained on the cells' training and reverse forms by
  Distillation's window-batched update (algorithms/distillation.py), not through forward(); a GRU student
  and a GRU teacher that both qualify take their rollout step as one launch (kernels.gru_cell_pair,
  StudentTeacherRecurrent.act_and_evaluate), as two LSTMs do.

* hidden size 512 (legged_gym's rnn_hidden_size) takes the same steps of either kind, under the same conditions, on the
  cells' `_h` forms (kernels.Cell.takes): hidden_states are [1, M, 512], the step's output [M, 512].
  RSLRL_RNN_HIDDEN_512=0 keeps a 512-wide memory on the RNN library.  The distillation update stays at 256.

Both kinds go through one predicate, Memory.fused_cell (the kernels.Cell of the step, or None; cell_ok / gru_cell_ok are
views of it), one fused branch in forward, and paired_step for two memories.
"""

from __future__ import annotations

import torch
import torch.nn as nn

from .. import kernels
from ..utils import unpad_trajectories
from . import fused_mlp


def _done_mask(dones: torch.Tensor) -> torch.Tensor:
    """[N] dones -> bool [N, 1], broadcast over [layers, N, hidden]."""
    return (dones == 1).reshape(-1, 1)


class Memory(nn.Module):
    """GRU or LSTM with the hidden states of the last step kept between calls."""

    def __init__(self, input_size, type="lstm", num_layers=1, hidden_size=256):
        super().__init__()
        # (anything but "gru" is an LSTM, as in the reference)
        kinds = {"gru": nn.GRU}
        self.rnn = kinds.get(type.lower(), nn.LSTM)(input_size, hidden_size, num_layers)
        self.hidden_states = None
        self._cell_image = None  # (key, image) of the fused cell's weights

    def fused_cell(self, input):
        """The kernels.Cell this step runs on, or None for the RNN library: see the module docstring."""
        cell = kernels.cell_of(self.rnn)
        return cell if cell is not None and cell.enabled() and self._takes(cell, input) else None

    def _takes(self, cell, input) -> bool:
        """fused_cell's conditions on the input and the RNN, for the enabled `cell` of self.rnn."""
        rnn = self.rnn
        return (not torch.is_grad_enabled() and input.is_cuda and input.dim() == 2
                and input.dtype == torch.float32 and rnn.bias and not rnn.bidirectional
                and (cell is kernels.GRU or rnn.proj_size == 0)
                and cell.takes(input.shape[0], input.shape[1], rnn.hidden_size, rnn.num_layers))

    def cell_ok(self, input) -> bool:
        """Whether this step runs on the fused LSTM cell (kernels.lstm_cell)."""
        return self.fused_cell(input) is kernels.LSTM

    def gru_cell_ok(self, input) -> bool:
        """Whether this step runs on the fused GRU cell (kernels.gru_cell)."""
        return self.fused_cell(input) is kernels.GRU

    def cell_operands(self):
        """(image, b_ih, b_hh) of the fused cell (the LSTM's or the GRU's, by the kind of self.rnn); the image is
        reused only inside one frozen_weights() scope."""
        rnn = self.rnn
        w_ih, w_hh = rnn.weight_ih_l0, rnn.weight_hh_l0
        key = (fused_mlp._frozen_gen, w_ih.data_ptr(), w_hh.data_ptr(), w_ih._version, w_hh._version)
        if not fused_mlp._frozen_depth or self._cell_image is None or self._cell_image[0] != key:
            self._cell_image = (key, kernels.cell_of(rnn).image(w_ih, w_hh))
        return self._cell_image[1], rnn.bias_ih_l0, rnn.bias_hh_l0

    def _keep(self, cell, state):
        """A fused step's new state tuple as hidden_states; returns its h [1, M, H], the step's output."""
        h = state[0].unsqueeze(0)
        self.hidden_states = (h, state[1].unsqueeze(0)) if cell.n_state == 2 else h
        return h

    def cell_state(self):
        """The (h, c) the fused cell continues from, or None."""
        return self.hidden_states

    def forward(self, input, masks=None, hidden_states=None):
        if masks is not None:
            # batch mode (policy update): whole padded trajectories from their saved first hidden states
            if hidden_states is None:
                raise ValueError("Hidden states not passed to memory module during policy update")
            out, _ = self.rnn(input, hidden_states)
            return unpad_trajectories(out, masks)
        # inference mode (rollout, play): one step from the hidden states of the last one
        cell = self.fused_cell(input)
        if cell is not None:
            return self._keep(cell, cell.step(input, cell.unpack(self.hidden_states), *self.cell_operands()))
        out, self.hidden_states = self.rnn(input.unsqueeze(0), self.hidden_states)
        return out

    def reset(self, dones=None, hidden_states=None):
        if dones is None:
            self.hidden_states = hidden_states
        elif self.hidden_states is not None and hidden_states is None:
            mask = _done_mask(dones)
            states = self.hidden_states if isinstance(self.hidden_states, tuple) else (self.hidden_states,)
            for h in states:
                h.masked_fill_(mask, 0.0)

    def detach_hidden_states(self, dones=None):
        if self.hidden_states is None:
            return
        is_tuple = isinstance(self.hidden_states, tuple)
        states = self.hidden_states if is_tuple else (self.hidden_states,)
        if dones is None:
            states = tuple(h.detach() for h in states)
        else:
            # the rows of done envs stop carrying gradients; values are unchanged
            mask = _done_mask(dones)
            states = tuple(torch.where(mask, h.detach(), h) for h in states)
        self.hidden_states = states if is_tuple else states[0]


def paired_step(m0: Memory, x0, m1: Memory, x1):
    """The rollout step of two memories as one launch (Cell.step_pair: the bits of the two single launches) when both
    qualify for the fused cell of one kind at one row count: writes both hidden_states and returns the two outputs
    [M, H]; otherwise None, and nothing has run."""
    cell = m0.fused_cell(x0)
    # (one kind, so one knob: it is read once)
    if (cell is None or kernels.cell_of(m1.rnn) is not cell or x0.shape[0] != x1.shape[0]
            or not m1._takes(cell, x1)):
        return None
    s0, s1 = cell.step_pair(x0, cell.unpack(m0.hidden_states), *m0.cell_operands(),
                            x1, cell.unpack(m1.hidden_states), *m1.cell_operands())
    m0._keep(cell, s0)
    m1._keep(cell, s1)
    return s0[0], s1[0]
