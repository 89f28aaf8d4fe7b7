"""The flat gradient buffer of the kernel-written updates (PPO's manual path, Distillation's window-batched ones) and
the multi-GPU gradient average over it (rsl_rl/algorithms/ppo.py:441-469, distillation.py:166-185)."""

from __future__ import annotations

import torch


class GradArena:
    """One contiguous fp32 buffer behind every trainable parameter's gradient, followed by `extra` scalar slots (the
    mini-batch KL) that travel in the same all-reduce.  The reference concatenates the gradients in parameters() order
    (policy.parameters(), then the RND predictor's; ppo.py:447-450); here `early` parameters (those whose gradients are
    complete before the rest of the backward, see PPO._early_params) come first, so that the all-reduce can start on
    that prefix while the backward still runs (`early_numel`).  The order of a SUM all-reduce's elements does not change
    any element's sum; every other parameter keeps its relative order (the RND predictor's span stays contiguous)."""

    def __init__(self, params, extra: int, device, early=()):
        self.params = list(params)
        ids = {id(p) for p in early}
        order = [p for p in self.params if id(p) in ids] + [p for p in self.params if id(p) not in ids]
        self.numel = sum(p.numel() for p in self.params)
        self.early_numel = sum(p.numel() for p in order if id(p) in ids)
        self.flat = torch.zeros(self.numel + extra, dtype=torch.float32, device=device)
        slots, off = {}, 0
        for p in order:
            slots[id(p)] = self.flat[off:off + p.numel()].view_as(p)
            off += p.numel()
        self.views = [slots[id(p)] for p in self.params]
        self._slot = slots
        self.extra = self.flat[self.numel:]

    def matches(self, params) -> bool:
        return len(params) == len(self.params) and all(a is b for a, b in zip(params, self.params))

    def slot(self, p) -> torch.Tensor:
        return self._slot[id(p)]

    def bind(self):
        """Make each parameter's .grad its arena view (the optimizers read and write gradients there)."""
        for p, v in zip(self.params, self.views):
            if p.grad is None or p.grad.data_ptr() != v.data_ptr():
                p.grad = v

    def span(self, params) -> torch.Tensor:
        """The contiguous arena range of consecutive parameters (e.g. the RND predictor's)."""
        first, last = self.slot(params[0]), self.slot(params[-1])
        start = first.data_ptr() - self.flat.data_ptr()
        stop = last.data_ptr() - self.flat.data_ptr() + 4 * last.numel()
        return self.flat[start // 4: stop // 4]


def all_reduce_arena(arena: GradArena, world_size: int, with_kl: bool, skip: int = 0, pending=()):
    """SUM all-reduce of the arena's gradients (+ its KL slot), then / world size (ppo.py:453-454 for the gradients,
    :273-274 for the KL).  skip / pending: the first `skip` elements were already handed to the asynchronous
    all-reduce(s) `pending` during the backward (the early prefix); the rest is reduced here, then the current stream
    waits for them before the division."""
    buf = arena.flat[:arena.numel + (1 if with_kl else 0)]
    if skip < buf.numel():
        torch.distributed.all_reduce(buf[skip:], op=torch.distributed.ReduceOp.SUM)
    for w in pending:
        w.wait()
    buf /= world_size


def reduce_gradients(arena, arena_params, cat_params, world_size: int, kl_mean: torch.Tensor | None = None):
    """Average gradients across ranks: in place as one buffer when the gradients of `arena_params` are exactly the
    arena's views (and no kl_mean rides along), otherwise the reference's concatenation / all-reduce / copy-back over
    those of `cat_params` that have one, with kl_mean (fp32, 1 element, averaged in place) appended."""
    if arena is not None and kl_mean is None and arena.matches(arena_params) and all(
            p.grad is not None and p.grad.data_ptr() == v.data_ptr() for p, v in zip(arena_params, arena.views)):
        all_reduce_arena(arena, world_size, with_kl=False)
        return
    with_grad = [p for p in cat_params if p.grad is not None]
    grads = [p.grad.view(-1) for p in with_grad]
    if kl_mean is not None:
        grads.append(kl_mean.reshape(1).to(grads[0].dtype))
    all_grads = torch.cat(grads)
    torch.distributed.all_reduce(all_grads, op=torch.distributed.ReduceOp.SUM)
    all_grads /= world_size
    if kl_mean is not None:
        kl_mean.copy_(all_grads[-1:].reshape(kl_mean.shape))
        all_grads = all_grads[:-1]
    # copy back (ppo.py:464-469) as one multi-tensor copy
    dst = [p.grad.data for p in with_grad]
    torch._foreach_copy_(dst, [g.view_as(d) for g, d in zip(all_grads.split([d.numel() for d in dst]), dst)])
