"""Tensor-level wrappers over the C ABI (include/rslrl_amd.h) -- the hot path's Python face.

Every device entry point takes torch tensors that live on a ROCm device, launches on the current
torch stream and never synchronises.  CPU tensors are rejected: there is no CPU fallback.
"""

from __future__ import annotations

import contextlib
import ctypes
import dataclasses
import os
from collections import defaultdict
from typing import Callable

import torch

from . import _lib

__all__ = [
    "compute_returns",
    "compute_returns_records",
    "normalize_advantages_",
    "randperm_mt19937",
    "gather_rows",
    "gather_records",
    "record_fill_slot",
    "ppo_loss_fwd_bwd",
    "ppo_loss_sym_fwd_bwd",
    "symmetry_augment",
    "PPOLossFunction",
    "rollout_record",
    "distill_record",
    "bc_loss",
    "BCLossFunction",
    "trajectory_index",
    "trajectory_pad",
    "trajectory_unpad",
    "TrajectoryUnpadFunction",
    "lstm_image",
    "lstm_cell",
    "lstm_cell_pair",
    "lstm_cell_train_pair",
    "lstm_cell_bwd_pair",
    "gru_cell_supported",
    "lstm_cell_anyd_supported",
    "gru_cell_anyd_supported",
    "gru_image",
    "gru_cell",
    "gru_cell_pair",
    "gru_cell_train",
    "gru_cell_train_pair",
    "gru_whh_t_image",
    "gru_cell_bwd",
    "gru_cell_bwd_pair",
]


def _require_device(*tensors: torch.Tensor):
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError(
                "rsl_rl_amd: the PPO hot path runs only on a ROCm GPU (torch 'cuda' device); got a tensor "
                f"on {t.device}. There is no CPU fallback."
            )


def _stream(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class _Workspace:
    """Per-(device, purpose) scratch buffers from torch's caching allocator, grown on demand.

    Reuse across calls is stream-ordered (all launches go to the current stream of the device).
    """

    def __init__(self):
        self._bufs = {}

    def get(self, device: torch.device, key: str, nbytes: int) -> torch.Tensor:
        # zero-filled on allocation: the loss workspace begins with an arrival counter that the library
        # expects to be zero before its first use and leaves zero after every call
        k = (device, key)
        buf = self._bufs.get(k)
        if buf is None or buf.numel() < nbytes:
            buf = torch.zeros(max(nbytes, 256), dtype=torch.uint8, device=device)
            self._bufs[k] = buf
        return buf


_ws = _Workspace()


_NO_SPAN = contextlib.nullcontext()


class KernelTimer:
    """Optional HIP-event timing of each C-ABI call, recorded on the stream the kernels launch on.

    bench.py enables it over its timed region to report the dominant kernel's live launch duration
    (roofline.achieved); disabled it costs one attribute check per call.
    """

    def __init__(self):
        self.enabled = False
        self.mlp_enabled = False  # the (many) MLP GEMM launches are timed separately from the hot path
        self.spans = defaultdict(list)
        self.bytes = defaultdict(list)
        self.flops = defaultdict(list)

    def reset(self):
        self.spans.clear()
        self.bytes.clear()
        self.flops.clear()

    def span(self, name: str, device: torch.device, algorithmic_bytes: int, flops: int = 0):
        # disabled (every call outside bench.py's timed region): one shared no-op context, no generator per call
        if not (self.mlp_enabled if name.startswith("linear_") else self.enabled):
            return _NO_SPAN
        return self._span(name, device, algorithmic_bytes, flops)

    @contextlib.contextmanager
    def _span(self, name: str, device: torch.device, algorithmic_bytes: int, flops: int = 0):
        stream = torch.cuda.current_stream(device)
        start = torch.cuda.Event(enable_timing=True)
        end = torch.cuda.Event(enable_timing=True)
        start.record(stream)
        yield
        end.record(stream)
        self.spans[name].append((start, end))
        self.bytes[name].append(algorithmic_bytes)
        self.flops[name].append(flops)

    # launches of the loss kernel, the rollout record and the record gather bound to their own event pair inside the
    # library (rslrl_launch_timing_*, one tag per kernel): the dispatch's begin-to-end time, the duration rocprofv3
    # reports, next to the marker span of the C-ABI call
    def arm_launch_events(self, capacity: int = 4096):
        _lib.check(_lib.lib().rslrl_launch_timing_enable(capacity), "rslrl_launch_timing_enable")

    def disarm_launch_events(self):
        _lib.check(_lib.lib().rslrl_launch_timing_enable(0), "rslrl_launch_timing_enable")

    LAUNCH_TAGS = {"ppo_loss": _lib.LAUNCH_TAG_PPO_LOSS, "rollout_record": _lib.LAUNCH_TAG_ROLLOUT_RECORD,
                   "gather_rows": _lib.LAUNCH_TAG_GATHER_RECORDS}

    @staticmethod
    def launch_events(kernel: str = "ppo_loss"):
        """(total_ms, launches) of `kernel`'s launches bound to events since the last arm_launch_events()."""
        ms, n = ctypes.c_double(0.0), ctypes.c_int64(0)
        tag = KernelTimer.LAUNCH_TAGS[kernel]
        _lib.check(_lib.lib().rslrl_launch_timing_read_tag(tag, ctypes.byref(ms), ctypes.byref(n)),
                   "rslrl_launch_timing_read_tag")
        return ms.value, n.value

    def summary(self):
        """name -> {launches, mean_ms, total_ms, bytes_per_launch}; synchronises the events."""
        out = {}
        for name, evs in self.spans.items():
            ms = [s.elapsed_time(e) for s, e in evs]
            out[name] = {
                "launches": len(ms),
                "mean_ms": sum(ms) / len(ms),
                "total_ms": sum(ms),
                "bytes_per_launch": sum(self.bytes[name]) / len(self.bytes[name]),
                "flops_per_launch": sum(self.flops[name]) / len(self.flops[name]),
            }
        return out


timer = KernelTimer()


def normal_affine_(x: torch.Tensor, scale: torch.Tensor, loc: torch.Tensor) -> torch.Tensor:
    """x <- x * scale + loc in place (torch's mul_ then add_ roundings) in one launch (rslrl_normal_affine): the
    rollout's Normal sample from standard normals x [N, A] contiguous; scale / loc [N, A] with unit column stride
    (row stride 0 for an expanded shared std)."""
    _require_device(x, scale, loc)
    if x.dim() != 2 or not x.is_contiguous() or scale.shape != x.shape or loc.shape != x.shape:
        raise ValueError("normal_affine_: x [N, A] contiguous, scale / loc of its shape")
    if (scale.stride(1) != 1 and x.shape[1] > 1) or (loc.stride(1) != 1 and x.shape[1] > 1):
        raise ValueError("normal_affine_: scale / loc need unit column stride")
    N, A = x.shape
    rc = _lib.lib().rslrl_normal_affine(x.data_ptr(), scale.data_ptr(), scale.stride(0), loc.data_ptr(), loc.stride(0),
                                        N, A, ctypes.c_void_p(_stream(x.device)))
    _lib.check(rc, "rslrl_normal_affine")
    return x


# ------------------------------------------------------------------------------------------------
# rollout_storage.py:127-149
# ------------------------------------------------------------------------------------------------
def _gae_workspace(dev: torch.device, T: int, N: int) -> torch.Tensor:
    """compute_returns' workspace of the current stream: the one-launch forms keep a grid barrier's ticket in it, so two
    streams must not share one (include/rslrl_amd.h, ABI 18)."""
    return _ws.get(dev, ("gae", _stream(dev)), _lib.lib().rslrl_compute_returns_workspace_bytes(T, N))


def gae_status_word(ws: torch.Tensor) -> torch.Tensor:
    """The workspace's uint32 grid-barrier status word as a 1-element int32 device view (0 = ok)."""
    off = _lib.lib().rslrl_compute_returns_status_offset()
    return ws[off:off + 4].view(torch.int32)


class GAEBarrierTimeout(RuntimeError):
    """compute_returns' one-launch grid barrier timed out: its blocks were not co-resident (another kernel or process
    held CUs), so that call's advantages are NaN."""


def raise_on_gae_status(status: torch.Tensor, value: float | int | None = None) -> None:
    """Raise GAEBarrierTimeout if the status word (or its already read-back `value`) is set; clears the word."""
    v = int(status.item()) if value is None else int(value)
    if v != 0:
        with torch.inference_mode():  # the word may be a view made under the runner's inference mode
            status.zero_()
        raise GAEBarrierTimeout(
            "rsl_rl_amd compute_returns: the one-launch GAE's grid barrier timed out (its blocks were not all resident "
            "at once), so the advantages of that rollout are NaN; set RSLRL_GAE_FUSED=0 to use the two-launch form")


def debug_knob(name: str, value: int) -> int:
    """Set one of the library's test knobs (include/rslrl_amd.h rslrl_debug_knob); returns the previous value."""
    prev = ctypes.c_int64(0)
    _lib.check(_lib.lib().rslrl_debug_knob(name.encode(), int(value), ctypes.byref(prev)), "rslrl_debug_knob")
    return prev.value


def compute_returns(values, rewards, dones, last_values, gamma, lam, normalize_advantage, returns, advantages):
    """GAE + (optional) normalisation, written into `returns` / `advantages` ([T, N, 1] fp32, in place).

    values/rewards [T, N, 1] fp32, dones [T, N, 1] uint8, last_values [N, 1] fp32, all contiguous.
    """
    _require_device(values, rewards, dones, last_values, returns, advantages)
    T, N = values.shape[0], values.shape[1]
    for t, dt in ((values, torch.float32), (rewards, torch.float32), (dones, torch.uint8),
                  (last_values, torch.float32), (returns, torch.float32), (advantages, torch.float32)):
        if t.dtype != dt or not t.is_contiguous():
            raise ValueError(f"compute_returns: expected contiguous {dt}, got {t.dtype} (contiguous={t.is_contiguous()})")
    if values.numel() != T * N or last_values.numel() != N or dones.numel() != T * N or rewards.numel() != T * N:
        raise ValueError("compute_returns: inconsistent shapes")
    L = _lib.lib()
    dev = values.device
    ws = _gae_workspace(dev, T, N)
    # one span over the production entry point (scan + fused normalisation): algorithmic bytes of both passes
    moved = 17 * T * N + 4 * N + (8 * T * N if normalize_advantage else 0)
    with timer.span("compute_returns", dev, moved):
        rc = L.rslrl_compute_returns(
            _ptr(values), _ptr(rewards), _ptr(dones), _ptr(last_values), ctypes.c_float(gamma), ctypes.c_float(lam),
            T, N, int(bool(normalize_advantage)), _ptr(returns), _ptr(advantages), _ptr(ws),
            ws.numel(), ctypes.c_void_p(_stream(dev)),
        )
    _lib.check(rc, "rslrl_compute_returns")


def compute_returns_records(values, rewards, dones, last_values, gamma, lam, returns, advantages, log_prob, records,
                            slot_offset: int):
    """compute_returns with normalisation whose last pass also writes every record's slot
    {value, log-prob, return, advantage, 0, 0, 0, 0} at `slot_offset` (include/rslrl_amd.h
    rslrl_compute_returns_records): records [T, N, R] contiguous fp32, log_prob [T, N, 1] contiguous fp32."""
    _require_device(values, rewards, dones, last_values, returns, advantages, log_prob, records)
    T, N = values.shape[0], values.shape[1]
    for t, dt in ((values, torch.float32), (rewards, torch.float32), (dones, torch.uint8), (last_values, torch.float32),
                  (returns, torch.float32), (advantages, torch.float32), (log_prob, torch.float32),
                  (records, torch.float32)):
        if t.dtype != dt or not t.is_contiguous():
            raise ValueError(f"compute_returns_records: expected contiguous {dt}, got {t.dtype} "
                             f"(contiguous={t.is_contiguous()})")
    if (values.numel() != T * N or last_values.numel() != N or dones.numel() != T * N or rewards.numel() != T * N
            or log_prob.numel() != T * N or records.dim() != 3 or records.shape[:2] != values.shape[:2]):
        raise ValueError("compute_returns_records: inconsistent shapes")
    R = records.shape[2]
    L = _lib.lib()
    dev = values.device
    ws = _gae_workspace(dev, T, N)
    # scan (17 B + 4 B per env) + normalisation reading adv / value / log-prob / return and writing adv + the slot
    moved = 17 * T * N + 4 * N + (4 * 4 + 4 + 32) * T * N
    with timer.span("compute_returns", dev, moved):
        rc = L.rslrl_compute_returns_records(
            _ptr(values), _ptr(rewards), _ptr(dones), _ptr(last_values), ctypes.c_float(gamma), ctypes.c_float(lam),
            T, N, _ptr(returns), _ptr(advantages), _ptr(log_prob), _ptr(records), R, int(slot_offset), _ptr(ws),
            ws.numel(), ctypes.c_void_p(_stream(dev)),
        )
    _lib.check(rc, "rslrl_compute_returns_records")


def compute_returns_slots(values, rewards, dones, last_values, gamma, lam, returns, advantages, log_prob, slots):
    """compute_returns with normalisation whose last pass also writes the scalar slot array
    slots[t, n] = {value, log-prob, return, advantage} (include/rslrl_amd.h rslrl_compute_returns_slots): slots
    [T, N, 4] contiguous fp32, log_prob [T, N, 1] contiguous fp32.  Returns the workspace's barrier status word (a
    1-element int32 device tensor, read it with raise_on_gae_status at the next synchronisation)."""
    _require_device(values, rewards, dones, last_values, returns, advantages, log_prob, slots)
    T, N = values.shape[0], values.shape[1]
    for t, dt in ((values, torch.float32), (rewards, torch.float32), (dones, torch.uint8), (last_values, torch.float32),
                  (returns, torch.float32), (advantages, torch.float32), (log_prob, torch.float32),
                  (slots, torch.float32)):
        if t.dtype != dt or not t.is_contiguous():
            raise ValueError(f"compute_returns_slots: expected contiguous {dt}, got {t.dtype} "
                             f"(contiguous={t.is_contiguous()})")
    if (values.numel() != T * N or last_values.numel() != N or dones.numel() != T * N or rewards.numel() != T * N
            or log_prob.numel() != T * N or slots.numel() != 4 * T * N):
        raise ValueError("compute_returns_slots: inconsistent shapes")
    L = _lib.lib()
    dev = values.device
    ws = _gae_workspace(dev, T, N)
    form = L.rslrl_compute_returns_slots_form(T, N, _ptr(values), _ptr(rewards), _ptr(dones), _ptr(log_prob),
                                              _ptr(returns), _ptr(advantages))
    if form != 0:
        # the one-launch forms (ABI 16 / 18): read value, reward, done, log-prob (13 B) + last value per env, write
        # return, advantage and the 16-byte slot (24 B)
        moved = 37 * T * N + 4 * N
    else:
        # scan (17 B + 4 B per env) + normalisation reading adv / value / log-prob / return, writing adv + the slot
        moved = 17 * T * N + 4 * N + (4 * 4 + 4 + 16) * T * N
    with timer.span("compute_returns", dev, moved):
        rc = L.rslrl_compute_returns_slots(
            _ptr(values), _ptr(rewards), _ptr(dones), _ptr(last_values), ctypes.c_float(gamma), ctypes.c_float(lam),
            T, N, _ptr(returns), _ptr(advantages), _ptr(log_prob), _ptr(slots), _ptr(ws), ws.numel(),
            ctypes.c_void_p(_stream(dev)),
        )
    _lib.check(rc, "rslrl_compute_returns_slots")
    return gae_status_word(ws)


def normalize_advantages_(adv: torch.Tensor, eps: float = 1e-8) -> torch.Tensor:
    """In-place (adv - mean) / (std_unbiased + eps) over all elements (rollout_storage.py:149)."""
    _require_device(adv)
    if adv.dtype != torch.float32 or not adv.is_contiguous():
        raise ValueError("normalize_advantages_: expected a contiguous fp32 tensor")
    L = _lib.lib()
    n = adv.numel()
    ws = _ws.get(adv.device, "norm", L.rslrl_normalize_workspace_bytes(n))
    with timer.span("adv_normalize", adv.device, 12 * n):
        rc = L.rslrl_normalize_advantages(_ptr(adv), n, ctypes.c_float(eps), _ptr(ws), ws.numel(),
                                          ctypes.c_void_p(_stream(adv.device)))
    _lib.check(rc, "rslrl_normalize_advantages")
    return adv


# ------------------------------------------------------------------------------------------------
# rollout_storage.py:165 -- torch CPU randperm semantics, host mt19937
# ------------------------------------------------------------------------------------------------
def randperm_mt19937(n: int, generator: torch.Generator | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
    """Exactly torch.randperm(n, generator=generator) for a CPU generator (default: the process default
    CPU generator), returned as int32 and advancing the generator identically.  Host code."""
    gen = torch.default_generator if generator is None else generator
    if gen.device.type != "cpu":
        raise ValueError("randperm_mt19937 follows torch's CPU generator; pass a CPU torch.Generator")
    state = gen.get_state()
    if out is None:
        out = torch.empty(n, dtype=torch.int32)
    if out.dtype != torch.int32 or out.device.type != "cpu" or not out.is_contiguous() or out.numel() < n:
        raise ValueError("randperm_mt19937: `out` must be a contiguous CPU int32 tensor with >= n elements")
    rc = _lib.lib().rslrl_randperm_mt19937(_ptr(state), state.numel(), n, _ptr(out))
    _lib.check(rc, "rslrl_randperm_mt19937")
    gen.set_state(state)
    return out[:n]


def randperm_mt19937_state(n: int, state: torch.Tensor, out: torch.Tensor) -> None:
    """randperm_mt19937 on a CPU generator-state blob (torch.Generator.get_state()) instead of a generator:
    writes the permutation into `out` (contiguous CPU int32, >= n elements) and advances `state` in place to
    what the generator's state would be afterwards.  Touches no torch state, so it may run on a worker thread
    (ctypes releases the GIL for the call)."""
    if out.dtype != torch.int32 or out.device.type != "cpu" or not out.is_contiguous() or out.numel() < n:
        raise ValueError("randperm_mt19937_state: `out` must be a contiguous CPU int32 tensor with >= n elements")
    rc = _lib.lib().rslrl_randperm_mt19937(_ptr(state), state.numel(), n, _ptr(out))
    _lib.check(rc, "rslrl_randperm_mt19937")


# ------------------------------------------------------------------------------------------------
# rollout_storage.py:168-197 -- all mini-batch fields in one launch
# ------------------------------------------------------------------------------------------------
def gather_rows(pairs, indices: torch.Tensor):
    """pairs: list of (src [rows, ...], dst [count, ...]) contiguous tensors; dst[r] = src[indices[r]]."""
    if len(pairs) > _lib.MAX_GATHER_FIELDS:
        for i in range(0, len(pairs), _lib.MAX_GATHER_FIELDS):
            gather_rows(pairs[i:i + _lib.MAX_GATHER_FIELDS], indices)
        return
    _require_device(indices, *[t for p in pairs for t in p])
    if indices.dtype != torch.int32 or not indices.is_contiguous():
        raise ValueError("gather_rows: indices must be contiguous int32")
    count = indices.numel()
    arr = (_lib.GatherField * max(len(pairs), 1))()
    moved = 0
    for i, (src, dst) in enumerate(pairs):
        if not (src.is_contiguous() and dst.is_contiguous()) or src.dtype != dst.dtype:
            raise ValueError("gather_rows: fields must be contiguous and of matching dtype")
        if dst.shape[0] != count or src.shape[1:] != dst.shape[1:]:
            raise ValueError("gather_rows: shape mismatch")
        row_bytes = dst[0].numel() * dst.element_size() if dst.dim() > 1 else dst.element_size()
        arr[i] = _lib.GatherField(src.data_ptr(), dst.data_ptr(), row_bytes)
        moved += 2 * row_bytes * count
    dev = indices.device
    with timer.span("gather_rows", dev, moved + 4 * count):
        rc = _lib.lib().rslrl_gather_rows(arr, len(pairs), _ptr(indices), count, ctypes.c_void_p(_stream(dev)))
    _lib.check(rc, "rslrl_gather_rows")


def gather_records(records: torch.Tensor, fields, indices: torch.Tensor):
    """Mini-batch gather over transition records (include/rslrl_amd.h rslrl_gather_records).

    records: [..., R] contiguous fp32 (one record of R floats per env-step, R % 4 == 0); fields: list of
    (offset, width, dst [count, width] contiguous fp32); dst[r] = records.view(-1, R)[indices[r], offset:offset+width].
    """
    if len(fields) > _lib.MAX_GATHER_FIELDS:
        raise ValueError(f"gather_records: at most {_lib.MAX_GATHER_FIELDS} fields per launch")
    _require_device(records, indices, *[f[2] for f in fields])
    if records.dtype != torch.float32 or not records.is_contiguous():
        raise ValueError("gather_records: records must be contiguous fp32")
    if indices.dtype != torch.int32 or not indices.is_contiguous():
        raise ValueError("gather_records: indices must be contiguous int32")
    R = records.shape[-1]
    count = indices.numel()
    arr = (_lib.RecordField * max(len(fields), 1))()
    used, moved = 0, 0
    for i, (off, width, dst) in enumerate(fields):
        if dst.dtype != torch.float32 or not dst.is_contiguous() or dst.numel() != count * width:
            raise ValueError("gather_records: dst must be contiguous fp32 [count, width]")
        arr[i] = _lib.RecordField(int(off), int(width), dst.data_ptr())
        used = max(used, off + width)
        moved += 8 * width * count
    dev = indices.device
    with timer.span("gather_rows", dev, moved + 4 * count):
        rc = _lib.lib().rslrl_gather_records(_ptr(records), R, arr, len(fields), _ptr(indices), count,
                                             ctypes.c_void_p(_stream(dev)))
    _lib.check(rc, "rslrl_gather_records")


def gather_records_side(records: torch.Tensor, fields, side: torch.Tensor, side_fields, indices: torch.Tensor):
    """gather_records plus fields of a side array (include/rslrl_amd.h rslrl_gather_records_side): side [..., 4]
    contiguous fp32 (one 16-byte unit per record index); side_fields: (offset, width, dst) with offset + width <= 4,
    dst[r] = side.view(-1, 4)[indices[r], offset:offset+width]."""
    if len(fields) + len(side_fields) > _lib.MAX_GATHER_FIELDS:
        raise ValueError(f"gather_records_side: at most {_lib.MAX_GATHER_FIELDS} fields per launch")
    _require_device(records, side, indices, *[f[2] for f in fields], *[f[2] for f in side_fields])
    if records.dtype != torch.float32 or not records.is_contiguous():
        raise ValueError("gather_records_side: records must be contiguous fp32")
    if side.dtype != torch.float32 or not side.is_contiguous() or side.shape[-1] != 4 or \
            side.numel() // 4 != records.numel() // records.shape[-1]:
        raise ValueError("gather_records_side: side must be contiguous fp32 [..., 4], one row per record")
    if indices.dtype != torch.int32 or not indices.is_contiguous():
        raise ValueError("gather_records_side: indices must be contiguous int32")
    R = records.shape[-1]
    count = indices.numel()
    arrs, moved = [], 0
    for fl in (fields, side_fields):
        arr = (_lib.RecordField * max(len(fl), 1))()
        for i, (off, width, dst) in enumerate(fl):
            if dst.dtype != torch.float32 or not dst.is_contiguous() or dst.numel() != count * width:
                raise ValueError("gather_records_side: dst must be contiguous fp32 [count, width]")
            arr[i] = _lib.RecordField(int(off), int(width), dst.data_ptr())
            moved += 8 * width * count
        arrs.append(arr)
    dev = indices.device
    with timer.span("gather_rows", dev, moved + 4 * count):
        rc = _lib.lib().rslrl_gather_records_side(_ptr(records), R, arrs[0], len(fields), _ptr(side), arrs[1],
                                                  len(side_fields), _ptr(indices), count, ctypes.c_void_p(_stream(dev)))
    _lib.check(rc, "rslrl_gather_records_side")


def record_fill_slot(records: torch.Tensor, offset: int, slot_floats: int, row=None, columns=()):
    """records.view(-1, R)[:, offset:offset + slot_floats] = [row | columns... | zeros] per record
    (include/rslrl_amd.h rslrl_record_fill_slot): row [.., w] and up to 4 columns [..] contiguous fp32, one
    entry per record."""
    _require_device(records, row, *columns)
    if records.dtype != torch.float32 or not records.is_contiguous():
        raise ValueError("record_fill_slot: records must be contiguous fp32")
    R = records.shape[-1]
    n = records.numel() // R
    rw = 0 if row is None else row.shape[-1]
    for t in ([row] if row is not None else []) + list(columns):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError("record_fill_slot: row and columns must be contiguous fp32")
    if (row is not None and row.numel() != n * rw) or any(c.numel() != n for c in columns) or len(columns) > 4:
        raise ValueError("record_fill_slot: one row / value per record, at most 4 columns")
    ptrs = (ctypes.c_void_p * 4)(*[c.data_ptr() for c in columns])
    with timer.span("record_fill_slot", records.device, (4 * rw + 4 * len(columns) + 4 * slot_floats) * n):
        rc = _lib.lib().rslrl_record_fill_slot(_ptr(records), R, int(offset), int(slot_floats), _ptr(row), rw, ptrs,
                                               len(columns), n, ctypes.c_void_p(_stream(records.device)))
    _lib.check(rc, "rslrl_record_fill_slot")


# ------------------------------------------------------------------------------------------------
# ppo.py:221-315 + backward of :368
# ------------------------------------------------------------------------------------------------
STATS_LOSS, STATS_SURROGATE, STATS_VALUE, STATS_ENTROPY, STATS_KL, STATS_ADV_MEAN, STATS_ADV_STD = range(7)


def _row_stride(t: torch.Tensor, A: int) -> int:
    if t.dim() != 2 or t.shape[1] != A or t.stride(1) != 1:
        raise ValueError("ppo_loss: [B, A] operands need unit stride along actions")
    return t.stride(0)


def ppo_loss_fwd_bwd(mu, sigma, values, actions, old_logp, advantages, target_values, returns, old_mu, old_sigma, *,
                     clip_param=0.2, value_loss_coef=1.0, entropy_coef=0.01, use_clipped_value_loss=True,
                     compute_kl=True, normalize_advantage=False, grad_mu=None, grad_sigma=None, grad_values=None,
                     stats=None):
    """One fused launch sequence: loss scalars + d(loss)/d(mu, sigma, V).

    mu [B, A]; sigma [A] (shared, e.g. ActorCritic.std) or [B, A] (state-dependent std); values [B] or
    [B, 1]; actions/old_mu/old_sigma [B, A] contiguous; old_logp/advantages/target_values/returns [B]/[B, 1].
    Returns (stats[8], grad_mu [B, A], grad_sigma (shape of sigma), grad_values (shape of values)).
    """
    mu_d, sg_d, v_d = mu.detach(), sigma.detach(), values.detach()
    _require_device(mu_d, sg_d, v_d, actions, old_logp, advantages, target_values, returns, old_mu, old_sigma)
    B, A = mu_d.shape
    if A > _lib.PPO_LOSS_MAX_ACTIONS:
        raise ValueError(f"ppo_loss: at most {_lib.PPO_LOSS_MAX_ACTIONS} actions supported")
    sigma_mode = 0 if sg_d.dim() == 1 else 1
    if sigma_mode == 0 and (sg_d.numel() != A or not sg_d.is_contiguous()):
        raise ValueError("ppo_loss: shared sigma must be a contiguous [A] tensor")
    for t in (v_d, old_logp, advantages, target_values, returns):
        if t.numel() != B or not t.is_contiguous():
            raise ValueError("ppo_loss: [B] operands must be contiguous with B elements")
    gv_stride = 1
    if grad_values is not None:  # [B] / [B, 1] contiguous, or a [B, 1] column of a wider buffer
        if grad_values.numel() != B or (grad_values.dim() == 2 and grad_values.shape[1] != 1) or grad_values.dim() > 2:
            raise ValueError("ppo_loss: grad_values must hold B values ([B] or [B, 1])")
        gv_stride = grad_values.stride(0) if grad_values.dim() == 2 else (1 if grad_values.is_contiguous() else 0)
        if gv_stride < 1:
            raise ValueError("ppo_loss: grad_values rows must be evenly spaced")
    for t in (actions, old_mu, old_sigma):
        if tuple(t.shape) != (B, A) or not t.is_contiguous():
            raise ValueError("ppo_loss: actions/old_mu/old_sigma must be contiguous [B, A]")
    dev = mu_d.device
    if grad_mu is None:
        grad_mu = torch.empty((B, A), dtype=torch.float32, device=dev)
    if grad_sigma is None:
        grad_sigma = torch.empty(sg_d.shape, dtype=torch.float32, device=dev)
    if grad_values is None:
        grad_values = torch.empty(v_d.shape, dtype=torch.float32, device=dev)
    if stats is None:
        stats = torch.empty(8, dtype=torch.float32, device=dev)
    args = _lib.PPOLossArgs()
    args.B, args.A, args.sigma_mode = B, A, sigma_mode
    args.mu, args.mu_stride = mu_d.data_ptr(), _row_stride(mu_d, A)
    args.sigma = sg_d.data_ptr()
    args.sigma_stride = _row_stride(sg_d, A) if sigma_mode == 1 else 0
    args.values = v_d.data_ptr()
    args.actions, args.old_logp, args.advantages = actions.data_ptr(), old_logp.data_ptr(), advantages.data_ptr()
    args.target_values, args.returns = target_values.data_ptr(), returns.data_ptr()
    args.old_mu, args.old_sigma = old_mu.data_ptr(), old_sigma.data_ptr()
    args.clip_param, args.value_loss_coef, args.entropy_coef = clip_param, value_loss_coef, entropy_coef
    args.use_clipped_value_loss = 1 if use_clipped_value_loss else 0
    args.compute_kl = 1 if compute_kl else 0
    args.normalize_advantage = 1 if normalize_advantage else 0
    args.grad_mu, args.grad_mu_stride = grad_mu.data_ptr(), _row_stride(grad_mu, A)
    args.grad_sigma = grad_sigma.data_ptr()
    args.grad_sigma_stride = _row_stride(grad_sigma, A) if sigma_mode == 1 else 0
    args.grad_values = grad_values.data_ptr()
    args.grad_values_stride = gv_stride
    args.stats = stats.data_ptr()
    L = _lib.lib()
    ws = _ws.get(dev, "ppo_loss", L.rslrl_ppo_loss_workspace_bytes(B, A))
    # algorithmic bytes: read mu, actions, old_mu, old_sigma (+ per-row sigma) and 5 scalars per row;
    # write d mu, d V (+ per-row d sigma)
    row_bytes = 4 * (4 * A + 5) + 4 * (A + 1) + (8 * A if sigma_mode == 1 else 0)
    with timer.span("ppo_loss", dev, row_bytes * B):
        rc = L.rslrl_ppo_loss_fwd_bwd(ctypes.byref(args), _ptr(ws), ws.numel(), ctypes.c_void_p(_stream(dev)))
    _lib.check(rc, "rslrl_ppo_loss_fwd_bwd")
    return stats, grad_mu, grad_sigma, grad_values


STATS_SYMMETRY = 7  # the symmetry loss (ppo_loss_sym_fwd_bwd; 0 from ppo_loss_fwd_bwd)


def ppo_loss_sym_fwd_bwd(mu, sigma, values, actions, old_logp, advantages, target_values, returns, old_mu, old_sigma, *,
                         B, k_ppo, k_mir, mirror_coeff=0.0, mirror_target=None, act_perm=None, act_sign=None,
                         symmetry_sum=None, clip_param=0.2, value_loss_coef=1.0, entropy_coef=0.01,
                         use_clipped_value_loss=True, compute_kl=True, normalize_advantage=False, grad_mu=None,
                         grad_sigma=None, grad_values=None, stats=None):
    """The fused PPO loss of a mini-batch of B stored rows evaluated on symmetry-augmented copies (ppo.py:213-257,
    :317-348; include/rslrl_amd.h rslrl_ppo_loss_sym_fwd_bwd).

    mu [k_mir * B, A]; sigma [A] or [k_mir * B, A]; values and actions k_ppo * B rows (k_ppo = 1 or k_mir); old_logp /
    advantages / target_values / returns [B] and old_mu / old_sigma [B, A]: the stored rows, read at row i mod B.  The
    mirror target (k_mir > 1) is either mirror_target [k_mir * B, A] (the caller's augmented means) or the device
    tables act_perm (int32) / act_sign (fp32) [k_mir, A].  symmetry_sum: optional fp64 device scalar, += stats[7].
    Returns (stats[8], grad_mu [k_mir * B, A], grad_sigma (shape of sigma), grad_values (shape of values))."""
    mu_d, sg_d, v_d = mu.detach(), sigma.detach(), values.detach()
    _require_device(mu_d, sg_d, v_d, actions, old_logp, advantages, target_values, returns, old_mu, old_sigma,
                    mirror_target, act_perm, act_sign, symmetry_sum)
    rows, A = mu_d.shape
    if A > _lib.PPO_LOSS_MAX_ACTIONS:
        raise ValueError(f"ppo_loss_sym: at most {_lib.PPO_LOSS_MAX_ACTIONS} actions supported")
    if not 1 <= k_mir <= _lib.SYMMETRY_MAX_AUG or k_ppo not in (1, k_mir):
        raise ValueError(f"ppo_loss_sym: 1 <= k_mir <= {_lib.SYMMETRY_MAX_AUG} and k_ppo in (1, k_mir) required")
    if rows != k_mir * B:
        raise ValueError("ppo_loss_sym: mu must hold k_mir * B rows")
    n_ppo = k_ppo * B
    sigma_mode = 0 if sg_d.dim() == 1 else 1
    if sigma_mode == 0 and (sg_d.numel() != A or not sg_d.is_contiguous()):
        raise ValueError("ppo_loss_sym: shared sigma must be a contiguous [A] tensor")
    if sigma_mode == 1 and sg_d.shape[0] != rows:
        raise ValueError("ppo_loss_sym: per-row sigma must hold k_mir * B rows")
    if v_d.numel() != n_ppo or not v_d.is_contiguous():
        raise ValueError("ppo_loss_sym: values must be contiguous with k_ppo * B elements")
    for t in (old_logp, advantages, target_values, returns):
        if t.numel() != B or not t.is_contiguous():
            raise ValueError("ppo_loss_sym: the stored [B] operands must be contiguous with B elements")
    if tuple(actions.shape) != (n_ppo, A) or not actions.is_contiguous():
        raise ValueError("ppo_loss_sym: actions must be contiguous [k_ppo * B, A]")
    for t in (old_mu, old_sigma):
        if tuple(t.shape) != (B, A) or not t.is_contiguous():
            raise ValueError("ppo_loss_sym: old_mu / old_sigma must be contiguous [B, A]")
    tables = act_perm is not None or act_sign is not None
    if tables:
        if act_perm is None or act_sign is None or act_perm.dtype != torch.int32 or act_sign.dtype != torch.float32 \
                or tuple(act_perm.shape) != (k_mir, A) or tuple(act_sign.shape) != (k_mir, A) \
                or not act_perm.is_contiguous() or not act_sign.is_contiguous():
            raise ValueError("ppo_loss_sym: act_perm (int32) and act_sign (fp32) must both be contiguous [k_mir, A]")
    if mirror_target is not None and (tuple(mirror_target.shape) != (rows, A) or not mirror_target.is_contiguous()
                                      or mirror_target.dtype != torch.float32):
        raise ValueError("ppo_loss_sym: mirror_target must be contiguous fp32 [k_mir * B, A]")
    if symmetry_sum is not None and (symmetry_sum.dtype != torch.float64 or symmetry_sum.numel() != 1):
        raise ValueError("ppo_loss_sym: symmetry_sum must be one fp64 element")
    dev = mu_d.device
    if grad_mu is None:
        grad_mu = torch.empty((rows, A), dtype=torch.float32, device=dev)
    if grad_sigma is None:
        grad_sigma = torch.empty(sg_d.shape, dtype=torch.float32, device=dev)
    if grad_values is None:
        grad_values = torch.empty(v_d.shape, dtype=torch.float32, device=dev)
    if grad_mu.shape[0] != rows or grad_values.numel() != n_ppo or not grad_values.is_contiguous():
        raise ValueError("ppo_loss_sym: grad_mu needs k_mir * B rows, grad_values k_ppo * B contiguous values")
    if stats is None:
        stats = torch.empty(8, dtype=torch.float32, device=dev)
    sargs = _lib.PPOLossSymArgs()
    args = sargs.loss
    args.B, args.A, args.sigma_mode = B, A, sigma_mode
    args.mu, args.mu_stride = mu_d.data_ptr(), _row_stride(mu_d, A)
    args.sigma = sg_d.data_ptr()
    args.sigma_stride = _row_stride(sg_d, A) if sigma_mode == 1 else 0
    args.values = v_d.data_ptr()
    args.actions, args.old_logp, args.advantages = actions.data_ptr(), old_logp.data_ptr(), advantages.data_ptr()
    args.target_values, args.returns = target_values.data_ptr(), returns.data_ptr()
    args.old_mu, args.old_sigma = old_mu.data_ptr(), old_sigma.data_ptr()
    args.clip_param, args.value_loss_coef, args.entropy_coef = clip_param, value_loss_coef, entropy_coef
    args.use_clipped_value_loss = 1 if use_clipped_value_loss else 0
    args.compute_kl = 1 if compute_kl else 0
    args.normalize_advantage = 1 if normalize_advantage else 0
    args.grad_mu, args.grad_mu_stride = grad_mu.data_ptr(), _row_stride(grad_mu, A)
    args.grad_sigma = grad_sigma.data_ptr()
    args.grad_sigma_stride = _row_stride(grad_sigma, A) if sigma_mode == 1 else 0
    args.grad_values = grad_values.data_ptr()
    args.grad_values_stride = 1
    args.stats = stats.data_ptr()
    sargs.k_ppo, sargs.k_mir, sargs.mirror_coeff = k_ppo, k_mir, float(mirror_coeff)
    sargs.mirror_target = mirror_target.data_ptr() if mirror_target is not None else None
    sargs.act_perm = act_perm.data_ptr() if act_perm is not None else None
    sargs.act_sign = act_sign.data_ptr() if act_sign is not None else None
    sargs.symmetry_sum = symmetry_sum.data_ptr() if symmetry_sum is not None else None
    L = _lib.lib()
    ws = _ws.get(dev, "ppo_loss_sym", L.rslrl_ppo_loss_sym_workspace_bytes(B, A, k_mir))
    with timer.span("ppo_loss_sym", dev, ppo_loss_sym_bytes(B, A, k_ppo, k_mir, sigma_mode, compute_kl,
                                                            mirror_target is not None)):
        rc = L.rslrl_ppo_loss_sym_fwd_bwd(ctypes.byref(sargs), _ptr(ws), ws.numel(), ctypes.c_void_p(_stream(dev)))
    _lib.check(rc, "rslrl_ppo_loss_sym_fwd_bwd")
    return stats, grad_mu, grad_sigma, grad_values


def ppo_loss_sym_bytes(B, A, k_ppo, k_mir, sigma_mode=0, compute_kl=True, pointer_target=False) -> int:
    """Algorithmic bytes of one ppo_loss_sym_fwd_bwd call (csrc/ppo_loss_sym.hip): every row reads its mu and writes
    d mu; PPO rows add the actions, five scalars and d V; block 0 the old mu / sigma of the KL; a per-row sigma its
    read and its gradient; the pointer form its target rows."""
    b = 8 * A * k_mir * B + (4 * A + 24) * k_ppo * B + (8 * A * B if compute_kl else 0)
    if sigma_mode == 1:
        b += 8 * A * k_mir * B
    if pointer_target:
        b += 4 * A * (k_mir - 1) * B
    return b


def symmetry_augment(fields, B: int, K: int):
    """One launch of signed, column-permuted copies (include/rslrl_amd.h rslrl_symmetry_augment).  fields: list of
    (src [B, w] fp32 with unit column stride, dst [K * B, w] contiguous fp32, perm [K, w] int32 or None, sign [K, w]
    fp32 or None); dst[k * B + r, c] = sign[k, c] * src[r, perm[k, c]] (perm None: the rows repeated)."""
    if len(fields) > _lib.SYMMETRY_MAX_FIELDS or not 1 <= K <= _lib.SYMMETRY_MAX_AUG:
        raise ValueError(f"symmetry_augment: at most {_lib.SYMMETRY_MAX_FIELDS} fields and {_lib.SYMMETRY_MAX_AUG} "
                         "augmentations per launch")
    arr = (_lib.SymmetryField * max(len(fields), 1))()
    moved = 0
    dev = None
    for i, (src, dst, perm, sign) in enumerate(fields):
        _require_device(src, dst, perm, sign)
        w = src.shape[-1]
        if src.dtype != torch.float32 or dst.dtype != torch.float32 or src.dim() != 2 or src.shape[0] != B \
                or (B > 1 and src.stride(0) < w) or (w > 1 and src.stride(1) != 1) or tuple(dst.shape) != (K * B, w) \
                or not dst.is_contiguous() or not 1 <= w <= _lib.SYMMETRY_MAX_WIDTH:
            raise ValueError("symmetry_augment: src [B, w] fp32 rows (unit column stride), dst contiguous [K * B, w], "
                             f"w <= {_lib.SYMMETRY_MAX_WIDTH}")
        if (perm is None) != (sign is None) or (perm is not None and (
                perm.dtype != torch.int32 or sign.dtype != torch.float32 or tuple(perm.shape) != (K, w)
                or tuple(sign.shape) != (K, w) or not perm.is_contiguous() or not sign.is_contiguous())):
            raise ValueError("symmetry_augment: perm (int32) and sign (fp32) must both be contiguous [K, w] or None")
        stride = src.stride(0) if B > 1 else w
        arr[i] = _lib.SymmetryField(src.data_ptr(), stride, dst.data_ptr(), w, 0,
                                    perm.data_ptr() if perm is not None else None,
                                    sign.data_ptr() if sign is not None else None)
        moved += 4 * w * B * (1 + K)
        dev = src.device
    if not fields or B == 0:
        return
    with timer.span("symmetry_augment", dev, moved):
        rc = _lib.lib().rslrl_symmetry_augment(arr, len(fields), B, K, ctypes.c_void_p(_stream(dev)))
    _lib.check(rc, "rslrl_symmetry_augment")


class PPOLossFunction(torch.autograd.Function):
    """Autograd wrapper: loss = PPOLossFunction.apply(mu, sigma, values, batch..., hyper) -> scalar.

    Forward runs the fused kernel (it also produces the gradients); backward scales them by the
    upstream gradient.  The second output is the stats vector (no gradient).
    """

    @staticmethod
    def forward(ctx, mu, sigma, values, actions, old_logp, advantages, target_values, returns, old_mu, old_sigma,
                clip_param, value_loss_coef, entropy_coef, use_clipped_value_loss, compute_kl, normalize_advantage):
        stats, gmu, gsig, gv = ppo_loss_fwd_bwd(
            mu, sigma, values, actions, old_logp, advantages, target_values, returns, old_mu, old_sigma,
            clip_param=clip_param, value_loss_coef=value_loss_coef, entropy_coef=entropy_coef,
            use_clipped_value_loss=use_clipped_value_loss, compute_kl=compute_kl,
            normalize_advantage=normalize_advantage)
        ctx.save_for_backward(gmu, gsig, gv)
        ctx.mark_non_differentiable(stats)
        return stats[STATS_LOSS], stats

    @staticmethod
    def backward(ctx, g_loss, g_stats):
        gmu, gsig, gv = ctx.saved_tensors
        return (gmu * g_loss, gsig * g_loss, gv * g_loss) + (None,) * 13


# --------------------------------------------------------------------------------------------------
# rollout-side record (include/rslrl_amd.h rslrl_rollout_record)
# --------------------------------------------------------------------------------------------------
_DTYPE_CODES = {torch.float32: _lib.DTYPE_F32, torch.uint8: _lib.DTYPE_U8, torch.bool: _lib.DTYPE_U8,
                torch.int32: _lib.DTYPE_I32, torch.int64: _lib.DTYPE_I64}


def _flag_array(t, n):
    """(tensor, dtype code) for a [N] / [N, 1] flag array, converted only if its dtype is not native."""
    t = t.reshape(n)
    if t.dtype not in _DTYPE_CODES:
        t = t.float()
    if not t.is_contiguous():
        t = t.contiguous()
    return t, _DTYPE_CODES[t.dtype]


def pack_rnd_net(mlp) -> torch.Tensor:
    """[W1 | b1 | W2 | b2] of a Linear-ELU-Linear MLP (the layout rslrl_rollout_record reads)."""
    lin = [m for m in mlp if isinstance(m, torch.nn.Linear)]
    return torch.cat([lin[0].weight.reshape(-1), lin[0].bias, lin[1].weight.reshape(-1), lin[1].bias]).detach()


def rollout_record(step, *, obs_pairs, actions, mu, sigma, values, rewards, dones, time_outs, gamma,
                   out_actions, out_rewards, out_dones, out_values, out_logp, out_mu, out_sigma,
                   extra_reward=None, rnd=None, intrinsic_out=None, out_records=None):
    """One launch for the transition of env step `step` (ppo.py:142-169 + rollout_storage.py:77-103).

    obs_pairs: [(src [N, d], dst [N, d]), ...] observation groups to store.  out_records [N, R]: the obs, actions,
    mu and sigma destinations are fields of these transition records (written whole, zeros elsewhere).  rnd: None or a dict with
    keys obs [N, in], target / predictor (packed, pack_rnd_net), hidden, out, weight, and optionally
    state_mean / state_std / state_eps.  Returns nothing; all outputs are written in place."""
    _require_device(actions, mu, values, rewards)
    N, A = actions.shape
    L = _lib.lib()
    a = _lib.RolloutArgs()
    a.N, a.A = N, A
    sigma = sigma.detach()
    a.sigma_mode = 1 if sigma.dim() == 2 else 0
    keep = []

    def c(t):
        t = t.detach()
        t = t if t.is_contiguous() else t.contiguous()
        keep.append(t)
        return t.data_ptr()

    a.actions, a.mu, a.sigma, a.values, a.rewards = c(actions), c(mu), c(sigma), c(values), c(rewards.reshape(N))
    d, a.dones_dtype = _flag_array(dones, N)
    keep.append(d)
    a.dones = d.data_ptr()
    if time_outs is not None:
        to, a.time_outs_dtype = _flag_array(time_outs, N)
        keep.append(to)
        a.time_outs = to.data_ptr()
    a.gamma = float(gamma)
    if extra_reward is not None:
        a.extra_reward = c(extra_reward.reshape(N))
    if rnd is not None:
        ro = rnd["obs"]
        if ro.stride(-1) != 1:
            ro = ro.contiguous()
        keep.append(ro)
        a.rnd_obs, a.rnd_obs_stride = ro.data_ptr(), ro.stride(0)
        a.rnd_in, a.rnd_hidden, a.rnd_out = ro.shape[1], rnd["hidden"], rnd["out"]
        a.rnd_target, a.rnd_predictor = c(rnd["target"]), c(rnd["predictor"])
        a.rnd_weight = float(rnd["weight"])
        if rnd.get("state_mean") is not None:
            a.rnd_state_mean = c(rnd["state_mean"].reshape(-1))
            a.rnd_state_std = c(rnd["state_std"].reshape(-1))
            a.rnd_state_eps = float(rnd["state_eps"])
        if intrinsic_out is not None:
            a.intrinsic_out = intrinsic_out.data_ptr()
    if len(obs_pairs) > _lib.ROLLOUT_MAX_OBS:
        raise ValueError(f"at most {_lib.ROLLOUT_MAX_OBS} observation groups")
    a.n_obs = len(obs_pairs)
    for i, (src, dst) in enumerate(obs_pairs):
        a.obs[i].src, a.obs[i].dst, a.obs[i].row_floats = c(src), dst.data_ptr(), src.shape[-1]
    a.out_actions, a.out_rewards, a.out_dones = out_actions.data_ptr(), out_rewards.data_ptr(), out_dones.data_ptr()
    a.out_values, a.out_logp = out_values.data_ptr(), out_logp.data_ptr()
    a.out_mu, a.out_sigma = out_mu.data_ptr(), out_sigma.data_ptr()
    if out_records is not None:
        if out_records.dim() != 2 or out_records.shape[0] != N or not out_records.is_contiguous():
            raise ValueError("rollout_record: out_records must be contiguous [N, R]")
        a.record_floats, a.out_records = out_records.shape[1], out_records.data_ptr()
    # algorithmic bytes per env (SURVEY §8d style): obs groups in+out, actions/mu in+out, sigma out (+in if
    # per row), values/rewards/dones/time-outs in, reward/value/log-prob/done out
    obs_b = sum(8 * src.shape[-1] for src, _ in obs_pairs)
    per_env = obs_b + 4 * A * (5 + a.sigma_mode) + 4 + 4 + d.element_size() + 4 + (4 if time_outs is not None else 0) + 13
    with timer.span("rollout_record", actions.device, per_env * N):
        rc = L.rslrl_rollout_record(ctypes.byref(a), _stream(actions.device))
    _lib.check(rc, "rslrl_rollout_record")
    return keep  # the caller may hold these until the stream has consumed them (torch's allocator is stream-ordered)


class RolloutRecordPlan:
    """rollout_record's launch arguments for one storage (record layout, no RND / extra reward): the output bases, row
    strides and static fields are set once, and a step only writes its input pointers and its rows' addresses into the
    cached argument struct (rollout_record builds and checks everything per call: ~30 us of host time per env step at
    16384 envs, where the rollout is launch-bound).  `matches` tells whether a step's inputs fit the plan; the caller
    takes rollout_record otherwise."""

    _OUTS = ("out_actions", "out_rewards", "out_dones", "out_values", "out_logp", "out_mu", "out_sigma", "out_records")

    def __init__(self, outs: dict, obs_dsts, obs_widths, N: int, A: int, gamma: float, dones_dtype, time_outs_dtype,
                 shared_sigma: bool, device):
        a = _lib.RolloutArgs()
        a.N, a.A, a.sigma_mode, a.gamma = N, A, 0 if shared_sigma else 1, float(gamma)
        a.dones_dtype = _DTYPE_CODES[dones_dtype]
        self.time_outs_dtype = time_outs_dtype
        if time_outs_dtype is not None:
            a.time_outs_dtype = _DTYPE_CODES[time_outs_dtype]
        a.n_obs = len(obs_dsts)
        for i, w in enumerate(obs_widths):
            a.obs[i].row_floats = w
        rec = outs["out_records"]
        a.record_floats = rec.shape[-1]
        # [T, N, ...] buffers: row t of field f at base_f + t * stride_f (bytes)
        self.rows = [(k, outs[k].data_ptr(), outs[k].stride(0) * outs[k].element_size()) for k in self._OUTS]
        self.obs_rows = [(d.data_ptr(), d.stride(0) * d.element_size()) for d in obs_dsts]
        self.a, self.N, self.A, self.device, self.gamma = a, N, A, device, float(gamma)  # (a.gamma reads back as fp32)
        self._fn = _lib.lib().rslrl_rollout_record  # bound once: the launch runs every env step
        self.dones_dtype, self.shared_sigma, self.obs_widths = dones_dtype, shared_sigma, tuple(obs_widths)
        self.key = (self.obs_widths, dones_dtype, time_outs_dtype, self.gamma, shared_sigma)
        obs_b = sum(8 * w for w in obs_widths)
        self.bytes = (obs_b + 4 * A * (5 + (0 if shared_sigma else 1)) + 4 + 4 + torch.tensor([], dtype=dones_dtype)
                      .element_size() + 4 + (4 if time_outs_dtype is not None else 0) + 13) * N

    @staticmethod
    def signature(sigma, dones, time_outs, obs_srcs, gamma):
        """What a plan is built for (its static fields): steps with another signature need another plan."""
        return (tuple(s.shape[-1] for s in obs_srcs), dones.dtype, None if time_outs is None else time_outs.dtype,
                float(gamma), sigma.dim() == 1)

    def fits(self, actions, mu, sigma, values, rewards, dones, time_outs, obs_srcs) -> bool:
        """This step's inputs can be passed by pointer: every array dense with the element count the kernel reads
        (the general path reshapes / copies what is not), the [N, A] rows and the observation rows 16-byte aligned."""
        N, A = self.N, self.A
        for t, n in ((actions, N * A), (mu, N * A), (values, N), (rewards, N), (dones, N)):
            if t.numel() != n or not t.is_contiguous() or t.data_ptr() % 16 and n == N * A:
                return False
        if time_outs is not None and (time_outs.numel() != N or not time_outs.is_contiguous()):
            return False
        if sigma.numel() != (A if self.shared_sigma else N * A) or not sigma.is_contiguous():
            return False
        return all(s.dtype == torch.float32 and s.dim() == 2 and s.shape[0] == N and s.is_contiguous()
                   and s.data_ptr() % 16 == 0 for s in obs_srcs)

    def matches(self, actions, mu, sigma, values, rewards, dones, time_outs, obs_srcs, gamma) -> bool:
        return (self.signature(sigma, dones, time_outs, obs_srcs, gamma) == self.key
                and self.fits(actions, mu, sigma, values, rewards, dones, time_outs, obs_srcs))

    def launch(self, t: int, actions, mu, sigma, values, rewards, dones, time_outs, obs_srcs):
        a = self.a
        a.actions, a.mu, a.sigma = actions.data_ptr(), mu.data_ptr(), sigma.data_ptr()
        a.values, a.rewards, a.dones = values.data_ptr(), rewards.data_ptr(), dones.data_ptr()
        if time_outs is not None:
            a.time_outs = time_outs.data_ptr()
        for k, base, st in self.rows:
            setattr(a, k, base + t * st)
        for i, (src, (base, st)) in enumerate(zip(obs_srcs, self.obs_rows)):
            a.obs[i].src, a.obs[i].dst = src.data_ptr(), base + t * st
        with timer.span("rollout_record", self.device, self.bytes):
            rc = self._fn(ctypes.byref(a), _stream(self.device))  # the caller's current stream
        _lib.check(rc, "rslrl_rollout_record")


def distill_record_ok(obs_srcs, actions, privileged_actions, rewards, dones) -> bool:
    """distill_record takes this step's sources as they are: at most 4 observation groups, every source a contiguous
    fp32 device tensor, dones of a dtype with a code (fp32, uint8, bool, int32, int64)."""
    if len(obs_srcs) > _lib.ROLLOUT_MAX_OBS or actions.dim() != 2:
        return False
    N = actions.shape[0]
    for t, n in [(s, None) for s in obs_srcs] + [(actions, None), (privileged_actions, None), (rewards, N)]:
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.shape[0] == N
                and (t.dim() == 2 and t.shape[1] >= 1 if n is None else t.numel() == n)):
            return False
    return (privileged_actions.shape == actions.shape and dones.is_cuda and dones.dtype in _DTYPE_CODES
            and dones.numel() == N and dones.is_contiguous())


def distill_record(*, obs_pairs, actions, privileged_actions, rewards, dones, out_actions, out_privileged_actions,
                   out_rewards, out_dones):
    """One launch for the transition of a distillation env step (rollout_storage.py:77-103, include/rslrl_amd.h
    rslrl_distill_record): obs_pairs [(src [N, w], dst [N, w]), ...] (at most 4, any w), actions and
    privileged_actions [N, A], rewards [N] -> out_rewards [N, 1], dones [N] -> out_dones uint8 [N, 1].  Every tensor
    contiguous (distill_record_ok for the sources; the destinations are rows of the storage).  A group moves in
    16-byte units where w % 4 == 0 and both of its pointers are 16-byte aligned, in dwords otherwise."""
    _require_device(actions, privileged_actions, rewards, dones)
    if not distill_record_ok([s for s, _ in obs_pairs], actions, privileged_actions, rewards, dones):
        raise ValueError("distill_record: contiguous fp32 device sources (dones: fp32, uint8, bool, int32 or int64) "
                         f"and at most {_lib.ROLLOUT_MAX_OBS} observation groups")
    N, A = actions.shape
    a = _lib.DistillRecordArgs()
    a.N, a.A, a.n_obs = N, A, len(obs_pairs)
    nbytes = 0
    for i, (src, dst) in enumerate(obs_pairs):
        w = src.shape[1]
        if dst.shape != src.shape or dst.dtype != torch.float32 or not dst.is_contiguous():
            raise ValueError("distill_record: an observation destination must be a contiguous fp32 [N, w] row")
        o = a.obs[i]
        o.src, o.dst, o.row_floats = src.data_ptr(), dst.data_ptr(), w
        o.unit_bytes = 16 if w % 4 == 0 and src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0 else 4
        nbytes += 8 * w
    for dst, shape, dtype in ((out_actions, (N, A), torch.float32), (out_privileged_actions, (N, A), torch.float32),
                              (out_rewards, (N, 1), torch.float32), (out_dones, (N, 1), torch.uint8)):
        if tuple(dst.shape) != shape or dst.dtype != dtype or not dst.is_contiguous():
            raise ValueError("distill_record: the destinations are contiguous rows [N, A], [N, A], [N, 1], uint8 [N, 1]")
    a.actions, a.privileged_actions = actions.data_ptr(), privileged_actions.data_ptr()
    a.rewards, a.dones, a.dones_dtype = rewards.data_ptr(), dones.data_ptr(), _DTYPE_CODES[dones.dtype]
    a.out_actions, a.out_privileged_actions = out_actions.data_ptr(), out_privileged_actions.data_ptr()
    a.out_rewards, a.out_dones = out_rewards.data_ptr(), out_dones.data_ptr()
    with timer.span("distill_record", actions.device, (nbytes + 16 * A + 9 + dones.element_size()) * N):
        rc = _lib.lib().rslrl_distill_record(ctypes.byref(a), _stream(actions.device))
    _lib.check(rc, "rslrl_distill_record")


class DistillRecordPlan:
    """distill_record's launch arguments for one distillation storage: the static fields, the destinations' bases and
    row strides are set once, and a step writes only its source pointers and its rows' addresses into the cached struct
    (the rollout step is launch-bound up to tens of thousands of envs: what distill_record builds and checks per call
    costs as much host time as the copies it replaces).  `fits` tells whether a step's sources can be passed by
    pointer; the caller keeps add_transitions otherwise."""

    def __init__(self, obs_dsts, actions, privileged_actions, rewards, dones, dones_dtype, device):
        T, N, A = actions.shape
        a = _lib.DistillRecordArgs()
        a.N, a.A, a.n_obs, a.dones_dtype = N, A, len(obs_dsts), _DTYPE_CODES[dones_dtype]
        self.widths = [d.shape[-1] for d in obs_dsts]
        for i, w in enumerate(self.widths):
            a.obs[i].row_floats = w
        outs = (("out_actions", actions), ("out_privileged_actions", privileged_actions), ("out_rewards", rewards),
                ("out_dones", dones))
        if not all(d.is_contiguous() for d in list(obs_dsts) + [t for _, t in outs]):
            raise ValueError("DistillRecordPlan: the storage's [T, N, .] buffers are contiguous")
        # [T, N, ...] buffers: row t of field f at base_f + t * stride_f (bytes)
        self.rows = [(k, t.data_ptr(), t.stride(0) * t.element_size()) for k, t in outs]
        self.obs_rows = [(d.data_ptr(), d.stride(0) * d.element_size()) for d in obs_dsts]
        # (source, element count) pairs `fits` walks: the groups, then actions, privileged actions, rewards
        self.counts = [N * w for w in self.widths] + [N * A, N * A, N]
        self.a, self.N, self.A, self.device, self.dones_dtype = a, N, A, device, dones_dtype
        self._fn = _lib.lib().rslrl_distill_record  # bound once: the launch runs every env step
        self.bytes = (8 * sum(self.widths) + 16 * A + 9 + torch.tensor([], dtype=dones_dtype).element_size()) * N

    def fits(self, obs_srcs, actions, privileged_actions, rewards, dones) -> bool:
        """Every source is a dense fp32 device array of the element count the kernel reads, dones of the plan's
        dtype."""
        f32 = torch.float32
        for t, n in zip((*obs_srcs, actions, privileged_actions, rewards), self.counts):
            if t.dtype != f32 or t.numel() != n or not t.is_contiguous() or not t.is_cuda:
                return False
        return (dones.dtype == self.dones_dtype and dones.numel() == self.N and dones.is_contiguous()
                and dones.is_cuda)

    def launch(self, t: int, obs_srcs, actions, privileged_actions, rewards, dones):
        a = self.a
        a.actions, a.privileged_actions = actions.data_ptr(), privileged_actions.data_ptr()
        a.rewards, a.dones = rewards.data_ptr(), dones.data_ptr()
        for k, base, st in self.rows:
            setattr(a, k, base + t * st)
        for o, src, w, (base, st) in zip(a.obs, obs_srcs, self.widths, self.obs_rows):
            sp, dp = src.data_ptr(), base + t * st
            o.src, o.dst = sp, dp
            o.unit_bytes = 4 if (w & 3) or ((sp | dp) & 15) else 16
        with timer.span("distill_record", self.device, self.bytes):
            rc = self._fn(ctypes.byref(a), _stream(self.device))  # the caller's current stream
        _lib.check(rc, "rslrl_distill_record")


def ppo_tail_args(stats, kl, lr, lr32, desired_kl, sums, round_fp32=False) -> _lib.PpoTail:
    """rslrl_ppo_tail_t of the per-mini-batch tail (ppo_update_tail's arguments)."""
    _require_device(stats, kl, lr, lr32, sums)
    on = lr is not None
    return _lib.PpoTail(stats.data_ptr(), kl.data_ptr() if on else None, lr.data_ptr() if on else None,
                        lr32.data_ptr() if on else None, 1 if round_fp32 else 0,
                        float(desired_kl) * 2.0 if on else 0.0, float(desired_kl) / 2.0 if on else 0.0,
                        sums.data_ptr() if sums is not None else None)


def ppo_update_tail_args(t: _lib.PpoTail, device) -> None:
    """rslrl_ppo_update_tail of a ppo_tail_args struct (its own launch)."""
    rc = _lib.lib().rslrl_ppo_update_tail(t.stats, t.kl, t.lr, t.lr32, t.round_fp32, t.kl_hi, t.kl_lo, t.sums,
                                          _stream(device))
    _lib.check(rc, "rslrl_ppo_update_tail")


def ppo_update_tail(stats, kl, lr, lr32, desired_kl, sums, round_fp32=False):
    """One launch for the per-mini-batch tail of PPO.update (include/rslrl_amd.h rslrl_ppo_update_tail):
    the adaptive-KL lr rule on the fp64 device lr (when lr is not None; kl: fp32 device scalar) and the loss
    statistics accumulation sums[0:3] += (value, surrogate, entropy) of stats.  FusedClipAdam.step(tail=...) runs
    the same inside its norm launch."""
    ppo_update_tail_args(ppo_tail_args(stats, kl, lr, lr32, desired_kl, sums, round_fp32), stats.device)


class FusedClipAdam:
    """optimizer.step() for a torch.optim.Adam over ROCm parameters as two launches (include/rslrl_amd.h
    rslrl_clip_adam_step): gradient-norm clipping at max_grad_norm (ppo.py:373, clip_grad_norm_) folded into
    torch's fused-Adam arithmetic (ppo.py:374).  The optimizer's state (step / exp_avg / exp_avg_sq, torch's
    fused layout) and state_dict stay torch's; parameters whose grad is None are skipped, as torch does.
    Supported: one group of contiguous fp32 device parameters (at most ADAM_MAX_TENSORS), weight_decay 0,
    no amsgrad / maximize / differentiable; anything else keeps torch's clip_grad_norm_ + step."""

    def __init__(self, optimizer, max_grad_norm, clip_params=None):
        """clip_params: the parameters clip_grad_norm_ spans (distillation.py:134 clips policy.student only); the
        others are stepped with their gradients as they are.  None: every parameter, as ppo.py:373."""
        self.opt = optimizer
        self.max_grad_norm = float(max_grad_norm) if max_grad_norm is not None else 0.0
        self.clip_params = clip_params
        L = _lib.lib()
        dev = optimizer.param_groups[0]["params"][0].device
        self.ws = torch.zeros(max(L.rslrl_adam_workspace_bytes() // 4, 1), dtype=torch.int32, device=dev)
        self.args = _lib.AdamArgs()

    @staticmethod
    def supported(optimizer, trained=None) -> bool:
        """trained: the parameters that will ever carry a gradient, when the caller knows them (a distillation
        policy's optimizer also holds the frozen teacher): the tensor limit then counts these."""
        if not isinstance(optimizer, torch.optim.Adam) or len(optimizer.param_groups) != 1:
            return False  # the clip norm spans every gradient: one launch pair over one group
        stepped = optimizer.param_groups[0]["params"] if trained is None else list(trained)
        if len(stepped) > _lib.ADAM_MAX_TENSORS:
            return False
        for g in optimizer.param_groups:
            if g["weight_decay"] != 0 or g["amsgrad"] or g["maximize"] or g.get("differentiable", False):
                return False
            if not all(p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() for p in g["params"]):
                return False
        return True

    def _state(self, p):
        st = self.opt.state[p]
        if len(st) == 0:  # torch's lazy init for fused Adam (optim/adam.py _init_group)
            st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            return st
        # a state_dict saved by a plain (non-fused) Adam -- e.g. a reference checkpoint -- loads its step as a
        # CPU tensor (torch keeps non-fused steps on the host); the kernels read and increment it on the device
        step = st["step"]
        if not (isinstance(step, torch.Tensor) and step.device == p.device and step.dtype == torch.float32
                and step.dim() == 0):
            st["step"] = torch.tensor(float(step), dtype=torch.float32, device=p.device)
        for k in ("exp_avg", "exp_avg_sq"):
            v = st[k]
            if v.device != p.device or v.dtype != p.dtype or not v.is_contiguous():
                st[k] = v.to(device=p.device, dtype=p.dtype).contiguous()
        return st

    def adopt_loaded_state(self):
        """After optimizer.load_state_dict of a checkpoint written by a non-fused Adam: the loaded param group
        carries fused=None and CPU steps.  Re-mark the group fused (torch's fallback step then takes the tensor
        lr of update()) and move every step to its parameter's device as fp32."""
        for g in self.opt.param_groups:
            g["fused"] = True
            g["foreach"] = None
            for p in g["params"]:
                if self.opt.state.get(p):
                    self._state(p)

    def step(self, closure=None, tail=None):
        """tail: an rslrl_ppo_tail_t (ppo_tail_args) run inside the norm launch before the step sizes take the lr
        (rslrl_clip_adam_step_tail: one launch less per mini-batch than ppo_update_tail + step)."""
        if closure is not None:
            raise RuntimeError("FusedClipAdam.step: closures are not supported")
        L = _lib.lib()
        keep = []  # contiguous copies (if any) stay alive until the launch is queued
        back = []  # (grad, copy): the kernel writes the clipped gradient into the copy; .grad gets it back
        clipped = None if self.clip_params is None else {id(p) for p in self.clip_params}
        for g in self.opt.param_groups:
            chunk = [p for p in g["params"] if p.grad is not None]
            if len(chunk) > _lib.ADAM_MAX_TENSORS:
                raise RuntimeError(f"FusedClipAdam.step: {len(chunk)} tensors carry a gradient, the limit is "
                                   f"{_lib.ADAM_MAX_TENSORS}")
            if chunk:
                a = self.args
                a.n = len(chunk)
                a.max_grad_norm = self.max_grad_norm
                lr = g["lr"]
                if isinstance(lr, torch.Tensor):
                    a.lr_dev = lr.data_ptr() if lr.is_cuda and lr.dtype == torch.float32 else None
                    a.lr = float(lr) if a.lr_dev is None else 0.0
                else:
                    a.lr_dev = None
                    a.lr = float(lr)
                a.beta1, a.beta2 = float(g["betas"][0]), float(g["betas"][1])
                a.eps = float(g["eps"])
                a.no_clip_mask = 0 if clipped is None else sum(
                    1 << i for i, p in enumerate(chunk) if id(p) not in clipped)
                for i, p in enumerate(chunk):
                    st = self._state(p)
                    grad = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                    keep.append(grad)
                    if grad is not p.grad:
                        back.append((p.grad, grad))
                    t = a.t[i]
                    t.param, t.grad = p.data_ptr(), grad.data_ptr()
                    t.exp_avg, t.exp_avg_sq = st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()
                    t.step, t.numel = st["step"].data_ptr(), p.numel()
                if tail is not None:
                    rc = L.rslrl_clip_adam_step_tail(ctypes.byref(a), ctypes.byref(tail), self.ws.data_ptr(),
                                                     self.ws.numel() * 4, _stream(self.ws.device))
                    tail = None
                else:
                    rc = L.rslrl_clip_adam_step(ctypes.byref(a), self.ws.data_ptr(), self.ws.numel() * 4,
                                                _stream(self.ws.device))
                _lib.check(rc, "rslrl_clip_adam_step")
        if tail is not None:  # no group had gradients: the tail still runs
            ppo_update_tail_args(tail, self.ws.device)
        for g, c in back:
            g.copy_(c)
        return None



# --------------------------------------------------------------------------------------------------
# ppo.py:352-363 + :369-372 -- RND predictor loss and gradient of one mini-batch
# --------------------------------------------------------------------------------------------------
def rnd_linears(mlp):
    """(Linear, Linear) of a Linear-ELU(alpha 1)-Linear MLP whose sizes the fused RND kernels take, else None."""
    mods = list(mlp)
    lin = [m for m in mods if isinstance(m, torch.nn.Linear)]
    if (len(mods) != 3 or len(lin) != 2 or not isinstance(mods[1], torch.nn.ELU) or mods[1].alpha != 1.0
            or lin[0].in_features > _lib.RND_MAX_IN or lin[0].out_features > _lib.RND_MAX_HIDDEN
            or lin[1].out_features > _lib.RND_MAX_OUT or lin[1].in_features != lin[0].out_features):
        return None
    if any(not (t.is_contiguous() and t.dtype == torch.float32) for m in lin for t in (m.weight, m.bias)):
        return None
    return lin[0], lin[1]


def rnd_update(state, predictor, target, target_embedding, grad, loss_sum=None, loss=None, state_mean=None,
               state_std=None, state_eps=0.0):
    """One launch pair for the RND predictor's training step of a mini-batch (include/rslrl_amd.h rslrl_rnd_update).

    state [B, in] fp32 (unit column stride); predictor / target: (Linear, Linear) of rnd_linears; target None:
    target_embedding [B, out] holds the (detached) target values already, else they are computed and, when
    target_embedding is given, stored there.  grad: contiguous fp32 of the predictor's parameter count, packed
    [dW1 | db1 | dW2 | db2] -- overwritten.  loss_sum (fp64 [1], optional) += the fp32 mse; loss (fp32 [1]) = mse."""
    l1, l2 = predictor
    B, n_in = state.shape
    H, Q = l1.out_features, l2.out_features
    _require_device(state, grad, target_embedding, loss_sum, loss, state_mean, state_std)
    if state.dtype != torch.float32 or state.stride(1) != 1:
        raise ValueError("rnd_update: state must be fp32 with unit column stride")
    if n_in != l1.in_features:
        raise ValueError(f"rnd_update: state has {n_in} columns, the predictor takes {l1.in_features}")
    P = H * n_in + H + Q * H + Q
    if grad.dtype != torch.float32 or not grad.is_contiguous() or grad.numel() != P:
        raise ValueError("rnd_update: grad must be a contiguous fp32 buffer of the predictor's parameter count")
    if target_embedding is not None and (target_embedding.dtype != torch.float32 or not target_embedding.is_contiguous()
                                         or target_embedding.numel() != B * Q):
        raise ValueError("rnd_update: target_embedding must be contiguous fp32 [B, out]")
    a = _lib.RndUpdateArgs()
    a.B, a.in_, a.hidden, a.out = B, n_in, H, Q
    a.state, a.state_stride = state.data_ptr(), state.stride(0)
    if state_mean is not None:
        a.state_mean, a.state_std, a.state_eps = state_mean.data_ptr(), state_std.data_ptr(), float(state_eps)
    a.pred_w1, a.pred_b1 = l1.weight.data_ptr(), l1.bias.data_ptr()
    a.pred_w2, a.pred_b2 = l2.weight.data_ptr(), l2.bias.data_ptr()
    if target is not None:
        t1, t2 = target
        if (t1.in_features, t1.out_features, t2.out_features) != (n_in, H, Q):
            raise ValueError("rnd_update: predictor and target must have the same shapes")
        a.target_w1, a.target_b1 = t1.weight.data_ptr(), t1.bias.data_ptr()
        a.target_w2, a.target_b2 = t2.weight.data_ptr(), t2.bias.data_ptr()
    elif target_embedding is None:
        raise ValueError("rnd_update: without the target network the target embedding must be given")
    a.target_embedding = target_embedding.data_ptr() if target_embedding is not None else None
    a.grad = grad.data_ptr()
    a.loss_sum = loss_sum.data_ptr() if loss_sum is not None else None
    a.loss = loss.data_ptr() if loss is not None else None
    L = _lib.lib()
    dev = state.device
    ws = _ws.get(dev, "rnd", L.rslrl_rnd_update_workspace_bytes(B, n_in, H, Q))
    with timer.span("rnd_update", dev, 4 * (n_in + Q) * B, 2 * B * (3 if target is not None else 2) * (H * n_in + Q * H)):
        rc = L.rslrl_rnd_update(ctypes.byref(a), _ptr(ws), ws.numel(), ctypes.c_void_p(_stream(dev)))
    _lib.check(rc, "rslrl_rnd_update")


# --------------------------------------------------------------------------------------------------
# distillation.py:120-123 + :130 -- behaviour-cloning loss of a window of stored steps and its gradient
# --------------------------------------------------------------------------------------------------
BC_LOSS_TYPES = {"mse": _lib.BC_LOSS_MSE, "huber": _lib.BC_LOSS_HUBER}


def bc_loss(pred, target, N: int, loss_type, step_loss_out, grad_out=None):
    """One launch for the behaviour-cloning loss of S = rows / N stored steps (include/rslrl_amd.h
    rslrl_bc_loss_fwd_bwd): step_loss_out[s] = loss_fn(pred[s*N:(s+1)*N], target[s*N:(s+1)*N]) with loss_fn torch's
    mse_loss ("mse" / 0) or huber_loss ("huber" / 1), and, when grad_out is given, grad_out = d(sum_s step loss) /
    d pred.  pred [S*N, A] fp32 with unit column stride (any row stride); target [S*N, A] fp32 contiguous;
    step_loss_out: S contiguous fp32 elements (e.g. a slice of an update's loss buffer); grad_out: contiguous fp32
    [S*N, A] or [S*N, A rounded up to 4] (pad columns are zeroed: train_backward's dy_padded operand).
    Deterministic (two calls give the same bits) and stream-ordered; returns step_loss_out."""
    _require_device(pred, target, step_loss_out, grad_out)
    code = BC_LOSS_TYPES.get(loss_type, loss_type) if isinstance(loss_type, str) else int(loss_type)
    if code not in (_lib.BC_LOSS_MSE, _lib.BC_LOSS_HUBER):
        raise ValueError(f"bc_loss: unknown loss type {loss_type!r} (supported: {list(BC_LOSS_TYPES)})")
    if pred.dim() != 2 or pred.dtype != torch.float32 or pred.stride(1) != 1:
        raise ValueError("bc_loss: pred must be fp32 [rows, A] with unit column stride")
    rows, A = pred.shape
    N = int(N)
    if N < 1 or rows % N:
        raise ValueError(f"bc_loss: {rows} rows are not a whole number of steps of N = {N}")
    S = rows // N
    if target.dtype != torch.float32 or not target.is_contiguous() or target.numel() != rows * A:
        raise ValueError("bc_loss: target must be contiguous fp32 with pred's shape")
    if step_loss_out.dtype != torch.float32 or not step_loss_out.is_contiguous() or step_loss_out.numel() != S:
        raise ValueError(f"bc_loss: step_loss_out must hold {S} contiguous fp32 elements")
    a = _lib.BCLossArgs()
    a.S, a.N, a.A, a.loss_type = S, N, A, code
    a.pred, a.pred_stride = pred.data_ptr(), pred.stride(0) if rows > 1 else max(pred.stride(0), A)
    a.target, a.step_loss = target.data_ptr(), step_loss_out.data_ptr()
    if grad_out is not None:
        if (grad_out.dtype != torch.float32 or not grad_out.is_contiguous() or grad_out.dim() != 2
                or grad_out.shape[0] != rows or grad_out.shape[1] not in (A, A + (-A) % 4)):
            raise ValueError("bc_loss: grad_out must be contiguous fp32 [rows, A] or [rows, A rounded up to 4]")
        a.grad, a.grad_stride = grad_out.data_ptr(), grad_out.shape[1]
    L = _lib.lib()
    dev = pred.device
    ws = _ws.get(dev, "bc_loss", L.rslrl_bc_loss_workspace_bytes(S, N, A))
    with timer.span(f"bc_loss[S={S},N={N},A={A}]", dev, (12 if grad_out is not None else 8) * rows * A):
        rc = L.rslrl_bc_loss_fwd_bwd(ctypes.byref(a), _ptr(ws), ws.numel(), ctypes.c_void_p(_stream(dev)))
    _lib.check(rc, "rslrl_bc_loss_fwd_bwd")
    return step_loss_out


class BCLossFunction(torch.autograd.Function):
    """loss_fn(actions, privileged_actions) of one stored step (distillation.py:120) on kernels.bc_loss: the forward
    launch also writes d loss / d actions, which backward scales by the incoming gradient."""

    @staticmethod
    def forward(ctx, pred, target, loss_type):
        p = pred.detach()
        p = p if p.stride(-1) == 1 else p.contiguous()
        t = target.detach().contiguous()
        out = torch.empty(1, dtype=torch.float32, device=p.device)
        grad = torch.empty(p.shape, dtype=torch.float32, device=p.device)
        bc_loss(p, t, p.shape[0], loss_type, out, grad)
        ctx.save_for_backward(grad)
        return out.reshape(())

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return grad * g, None, None


# --------------------------------------------------------------------------------------------------
# trajectory bookkeeping of recurrent PPO (include/rslrl_amd.h rslrl_trajectory_*; utils.py:78-141,
# rollout_storage.py:206-260)
# --------------------------------------------------------------------------------------------------
class TrajectoryIndex:
    """What rslrl_trajectory_index wrote for dones [T, N] and a number of mini-batches: traj_id / traj_off [T, N]
    int32 (global trajectory number, env-major then time, and the offset inside it), env_prefix [N + 1] int32,
    bounds [num_mini_batches + 1] int32 -- all on the device.  read_bounds() is the one host read-back (the padded
    buffers are sized by it); nothing else here synchronises."""

    def __init__(self, T, N, num_mini_batches, traj_id, traj_off, env_prefix, bounds):
        self.T, self.N, self.num_mini_batches = T, N, num_mini_batches
        self.mb_envs = N // num_mini_batches
        self.traj_id, self.traj_off, self.env_prefix, self.bounds = traj_id, traj_off, env_prefix, bounds
        self.bounds_host = None

    def read_bounds(self):
        if self.bounds_host is None:
            self.bounds_host = self.bounds.tolist()
        return self.bounds_host


class TrajectoryMap:
    """One mini-batch's view of a TrajectoryIndex: envs [env0, env0 + envs) and trajectories [first, first + n_b).
    recurrent_mini_batch_generator attaches it to the yielded masks (`masks.trajectory_map`), which is how
    networks.Memory reaches the index map through the reference's forward(input, masks, hidden_states) signature."""

    def __init__(self, index: TrajectoryIndex, env0: int, envs: int, first: int, n_b: int):
        self.index, self.env0, self.envs, self.first, self.n_b = index, env0, envs, first, n_b


def trajectory_index(dones: torch.Tensor, num_mini_batches: int = 1) -> TrajectoryIndex:
    """dones: [T, N] or [T, N, 1] uint8 / bool on the device (the storage's buffer)."""
    _require_device(dones)
    if dones.dim() == 3 and dones.shape[-1] == 1:
        dones = dones[..., 0]
    if dones.dim() != 2:
        raise ValueError("trajectory_index: dones must be [T, N] or [T, N, 1]")
    if dones.dtype == torch.bool:
        dones = dones.view(torch.uint8) if dones.is_contiguous() else dones.to(torch.uint8)
    elif dones.dtype != torch.uint8:
        dones = (dones != 0).to(torch.uint8)
    dones = dones if dones.is_contiguous() else dones.contiguous()
    T, N = dones.shape
    M = int(num_mini_batches)
    if T < 1 or N < 1 or not 1 <= M <= N:
        raise ValueError(f"trajectory_index: T = {T}, N = {N}, num_mini_batches = {M}")
    dev = dones.device
    ints = torch.empty(2 * T * N + N + 1 + M + 1, dtype=torch.int32, device=dev)
    tid, toff = ints[:T * N].view(T, N), ints[T * N:2 * T * N].view(T, N)
    prefix, bounds = ints[2 * T * N:2 * T * N + N + 1], ints[2 * T * N + N + 1:]
    a = _lib.TrajectoryIndexArgs(dones.data_ptr(), T, N, M, tid.data_ptr(), toff.data_ptr(), prefix.data_ptr(),
                                 bounds.data_ptr())
    L = _lib.lib()
    ws = _ws.get(dev, "trajectory_index", L.rslrl_trajectory_index_workspace_bytes(T, N))
    with timer.span(f"trajectory_index[T={T},N={N}]", dev, 2 * T * N + 8 * T * N + 4 * N):
        rc = L.rslrl_trajectory_index(ctypes.byref(a), _ptr(ws), ws.numel(), ctypes.c_void_p(_stream(dev)))
    _lib.check(rc, "rslrl_trajectory_index")
    return TrajectoryIndex(T, N, M, tid, toff, prefix, bounds)


def trajectory_pad(index: TrajectoryIndex, groups, states=()):
    """Zero-padded trajectories, masks and the saved states at trajectory starts in one launch (+ the memsets).
    groups: [T, N, D] fp32 tensors with unit last stride and row (t, n) at (t * N + n) * stride(1) (contiguous, or the
    record layout's strided views); states: contiguous [T, L, N, H] fp32 tensors of one (L, H).
    Returns (padded, masks, gathered): padded[k] / gathered[q] are flat fp32 buffers and masks a flat bool buffer, each
    the concatenation over the index's mini-batches b of a contiguous [T, n_b, D] / [L, n_b, H] / [T, n_b] block
    (trajectory_views cuts them); with one mini-batch they are the reference's whole arrays.  Reads the index's
    bounds (one host read-back) unless they were read before."""
    T, N, M = index.T, index.N, index.num_mini_batches
    if len(groups) > _lib.TRAJECTORY_MAX_GROUPS or len(states) > _lib.TRAJECTORY_MAX_STATES:
        raise ValueError(f"trajectory_pad: at most {_lib.TRAJECTORY_MAX_GROUPS} groups and "
                         f"{_lib.TRAJECTORY_MAX_STATES} states per launch")
    dev = index.traj_id.device
    a = _lib.TrajectoryPadArgs()
    moved = 0
    keep = []  # copies that must outlive the launch's enqueue
    for k, g in enumerate(groups):
        _require_device(g)
        D = g.shape[-1]
        if g.dtype != torch.float32 or g.dim() != 3 or tuple(g.shape[:2]) != (T, N):
            raise ValueError("trajectory_pad: a group must be fp32 [T, N, D]")
        if T == 1 or N == 1 or D == 1:
            # torch reports arbitrary strides for size-1 dimensions: a contiguous copy has the ones the kernel reads
            g = g.contiguous()
            keep.append(g)
        if g.stride(2) != 1 or g.stride(1) < D or g.stride(0) != N * g.stride(1):
            raise ValueError("trajectory_pad: a group's rows must sit at one stride with unit column stride")
        a.groups[k].src, a.groups[k].src_stride, a.groups[k].width = g.data_ptr(), g.stride(1), D
    LH = None
    for q, st in enumerate(states):
        _require_device(st)
        if st.dtype != torch.float32 or st.dim() != 4 or not st.is_contiguous() or st.shape[0] != T \
                or st.shape[2] != N or (LH is not None and tuple(st.shape[1::2]) != LH):
            raise ValueError("trajectory_pad: states must be contiguous fp32 [T, L, N, H] of one (L, H)")
        LH = tuple(st.shape[1::2])
        a.state_src[q] = st.data_ptr()
    n_traj = index.read_bounds()[-1]
    padded = [torch.empty(T * n_traj * g.shape[-1], dtype=torch.float32, device=dev) for g in groups]
    masks = torch.empty(T * n_traj, dtype=torch.bool, device=dev)
    gathered = [torch.empty(LH[0] * n_traj * LH[1], dtype=torch.float32, device=dev) for _ in states]
    for k, g in enumerate(groups):
        a.groups[k].dst = padded[k].data_ptr()
        moved += 4 * g.shape[-1] * T * (index.mb_envs * M + n_traj)
    for q in range(len(states)):
        a.state_dst[q] = gathered[q].data_ptr()
        moved += 8 * LH[0] * LH[1] * n_traj
    a.T, a.N, a.num_mini_batches, a.n_traj = T, N, M, n_traj
    a.traj_id, a.traj_off, a.bounds = index.traj_id.data_ptr(), index.traj_off.data_ptr(), index.bounds.data_ptr()
    a.num_groups, a.num_states, a.masks = len(groups), len(states), masks.data_ptr()
    a.layers, a.hidden = LH if LH is not None else (0, 0)
    with timer.span(f"trajectory_pad[T={T},N={N}]", dev, moved):
        rc = _lib.lib().rslrl_trajectory_pad(ctypes.byref(a), ctypes.c_void_p(_stream(dev)))
    _lib.check(rc, "rslrl_trajectory_pad")
    return padded, masks, gathered


def trajectory_views(index: TrajectoryIndex, flat: torch.Tensor, lead: int, width: int | None):
    """The per-mini-batch [lead, n_b, width] (or [lead, n_b] with width None) blocks of a trajectory_pad buffer."""
    b = index.read_bounds()
    w = 1 if width is None else width
    out = []
    for i in range(index.num_mini_batches):
        n_b = b[i + 1] - b[i]
        v = flat[lead * b[i] * w: lead * b[i + 1] * w]
        out.append(v.view(lead, n_b) if width is None else v.view(lead, n_b, width))
    return out


def trajectory_unpad(padded: torch.Tensor, tmap: TrajectoryMap, scatter_from: torch.Tensor | None = None):
    """unpad_trajectories of one mini-batch through the index map: padded [T, n_b, H] -> [T, envs, H]; with
    scatter_from ([T, envs, H]) the transpose instead: returns the zero-filled [T, n_b, H] with the valid positions
    set (the backward)."""
    ix = tmap.index
    T, n_b, E = ix.T, tmap.n_b, tmap.envs
    src = padded if scatter_from is None else scatter_from
    _require_device(src)
    H = src.shape[-1]
    want = (T, n_b, H) if scatter_from is None else (T, E, H)
    if src.dtype != torch.float32 or tuple(src.shape) != want:
        raise ValueError(f"trajectory_unpad: expected fp32 {want}, got {src.dtype} {tuple(src.shape)}")
    src = src if src.is_contiguous() else src.contiguous()
    dev = src.device
    out = torch.empty((T, E, H) if scatter_from is None else (T, n_b, H), dtype=torch.float32, device=dev)
    pad_t, flat_t = (src, out) if scatter_from is None else (out, src)
    a = _lib.TrajectoryUnpadArgs(pad_t.data_ptr(), flat_t.data_ptr(), ix.traj_id.data_ptr(), ix.traj_off.data_ptr(),
                                 T, ix.N, E, tmap.env0, tmap.first, n_b, H, 0 if scatter_from is None else 1)
    with timer.span(f"trajectory_unpad[T={T},E={E},H={H}]", dev, 8 * T * E * H):
        rc = _lib.lib().rslrl_trajectory_unpad(ctypes.byref(a), ctypes.c_void_p(_stream(dev)))
    _lib.check(rc, "rslrl_trajectory_unpad")
    return out


class TrajectoryUnpadFunction(torch.autograd.Function):
    """unpad_trajectories (utils.py:134-141) as a gather through the index map; backward is the scatter, in which every
    padded position receives 0."""

    @staticmethod
    def forward(ctx, padded, tmap):
        ctx.tmap = tmap
        return trajectory_unpad(padded.detach(), tmap)

    @staticmethod
    def backward(ctx, g):
        return trajectory_unpad(None, ctx.tmap, scatter_from=g), None


# --------------------------------------------------------------------------------------------------
# fused LSTM and GRU cells (include/rslrl_amd.h rslrl_lstm_cell / rslrl_gru_cell with their _pair, _train and _bwd forms;
# networks/memory.py).  The C entry points and their argument structs come in twins, one per kind; here every operation
# has one body that takes the kind (Cell, at the end of the section), the public wrappers keep
# their names and signatures, and only the builders of the argument structs, which really differ, exist per kind.  A
# GRU's wrappers take a bare h where the LSTM's take (h, c), and its gate tensors hold the blocks r, z, n, a.
# H below is the hidden size of the call: 256, or 512 on the `_h` entry points.
# --------------------------------------------------------------------------------------------------
LSTM_CELL_HIDDEN, LSTM_CELL_ROWS = 256, 64


def lstm_cell_supported(M: int, D: int, hidden: int, layers: int = 1) -> bool:
    """The shapes rslrl_lstm_cell takes (anything else returns RSLRL_E_UNSUPPORTED there)."""
    return (hidden == LSTM_CELL_HIDDEN and layers == 1 and D % 16 == 0 and 16 <= D <= 256 and M >= LSTM_CELL_ROWS
            and M % LSTM_CELL_ROWS == 0)


# The `_anyd` entry points (ABI 31) take any input width 1 <= D <= RNN_ANYD_MAX.  The wrappers
# below dispatch on D: a width the original entry takes keeps going there (same bits, same launch), every other width
# goes to its `_anyd` twin.  RSLRL_RNN_ANY_INPUT=0 (read at import) keeps the original routing: other widths are
# refused.
_RNN_ANY_INPUT = os.environ.get("RSLRL_RNN_ANY_INPUT", "1") != "0"
RNN_ANYD_MAX = 1024


def _rnn_first_width(D: int) -> bool:
    """The widths of the original entry points: a multiple of 16 in [16, 256]."""
    return D % 16 == 0 and 16 <= D <= 256


def _rnn_anyd(*widths) -> bool:
    """Whether a call with these input widths goes to the `_anyd` entry points."""
    return _RNN_ANY_INPUT and not all(_rnn_first_width(D) for D in widths)


def lstm_cell_anyd_supported(M: int, D: int, hidden: int, layers: int = 1) -> bool:
    """The shapes kernels.lstm_cell and its pair / training forms take: those of rslrl_lstm_cell_anyd (anything else
    returns RSLRL_E_UNSUPPORTED there), which include rslrl_lstm_cell's; with RSLRL_RNN_ANY_INPUT=0
    lstm_cell_supported."""
    if not _RNN_ANY_INPUT:
        return lstm_cell_supported(M, D, hidden, layers)
    return (hidden == LSTM_CELL_HIDDEN and layers == 1 and 1 <= D <= RNN_ANYD_MAX and M >= LSTM_CELL_ROWS
            and M % LSTM_CELL_ROWS == 0)


def gru_cell_supported(M: int, D: int, hidden: int, layers: int = 1) -> bool:
    """The shapes rslrl_gru_cell takes (anything else returns RSLRL_E_UNSUPPORTED there): the LSTM cell's."""
    return lstm_cell_supported(M, D, hidden, layers)


def gru_cell_anyd_supported(M: int, D: int, hidden: int, layers: int = 1) -> bool:
    """The shapes kernels.gru_cell and its pair / training forms take (rslrl_gru_cell_anyd's): the LSTM cell's."""
    return lstm_cell_anyd_supported(M, D, hidden, layers)


# The `_h` entry points take hidden size RNN_HIDDEN_WIDE at any input width.  The wrappers below
# dispatch on the width of the state, which they read off the weights (the biases of a forward form, dh of a reverse
# step): 256 keeps going where it went, 512 goes to the `_h` entry.  RSLRL_RNN_HIDDEN_512=0 (read at import) keeps the
# original routing: every operand is [M, 256] and a 512-wide memory stays on the RNN library.
_RNN_HIDDEN_512 = os.environ.get("RSLRL_RNN_HIDDEN_512", "1") != "0"
RNN_HIDDEN_WIDE = 512


# The recurrent PPO update of an LSTM policy on the ground DESIGN.md section 27 added -- hidden size 512, or wide MLPs
# behind the memories at either size -- takes the fused kernels from this many rows (envs per mini-batch) on: at 1,024
# rows nn.LSTM under autograd was as fast or faster (210 against 205 ms and 123 against 122 ms per update; obs 235 at 512
# was 3 % ahead and is gated with the rest), at 4,096 rows the fused update is 1.8-2.2x ahead
# (scripts/rnn_h512_probe.py, profiles/rnn_h512_probe.json).  GRU policies are ahead at every size and are not gated;
# the rollout step is not gated.
RNN_H512_LSTM_UPDATE_MIN_ROWS = 4096


def lstm_cell_h_supported(M: int, D: int, hidden: int, layers: int = 1) -> bool:
    """The shapes rslrl_lstm_cell_h and its pair / training forms take (anything else returns RSLRL_E_UNSUPPORTED
    there); the reverse step's are these without the input width."""
    return (hidden == RNN_HIDDEN_WIDE and layers == 1 and 1 <= D <= RNN_ANYD_MAX and M >= LSTM_CELL_ROWS
            and M % LSTM_CELL_ROWS == 0)


def gru_cell_h_supported(M: int, D: int, hidden: int, layers: int = 1) -> bool:
    """The shapes rslrl_gru_cell_h takes: the LSTM cell's."""
    return lstm_cell_h_supported(M, D, hidden, layers)


def _rnn_width(numel: int, per: int) -> int:
    """The hidden size of a call whose weights or states hold `numel` floats in `per` rows or blocks: RNN_HIDDEN_WIDE
    where that is their width and the `_h` forms are on, LSTM_CELL_HIDDEN otherwise (a tensor of any other width then
    fails the [M, 256] checks as it always has)."""
    return RNN_HIDDEN_WIDE if _RNN_HIDDEN_512 and per > 0 and numel == per * RNN_HIDDEN_WIDE else LSTM_CELL_HIDDEN


def _cell_image(cell, w_ih, w_hh):
    H, name = _rnn_width(w_hh.shape[-1], 1), cell.name + "_image"
    rows = cell.blocks * H
    _require_device(w_ih, w_hh)
    w_ih, w_hh = w_ih.detach(), w_hh.detach()
    D = w_ih.shape[1]
    if (w_ih.dtype != torch.float32 or w_hh.dtype != torch.float32 or tuple(w_ih.shape) != (rows, D)
            or tuple(w_hh.shape) != (rows, H) or not w_ih.is_contiguous() or not w_hh.is_contiguous()):
        raise ValueError(f"{name}: contiguous fp32 W_ih [{rows}, D] and W_hh [{rows}, {H}]")
    L = _lib.lib()
    wide = H == RNN_HIDDEN_WIDE
    sfx = "_h" if wide else "_anyd" if _rnn_anyd(D) else ""
    nbytes = getattr(L, f"rslrl_{name}_bytes{sfx}")(*((D, H) if wide else (D,)))
    if nbytes == 0:
        raise _lib.RslrlError(f"{name}: unsupported input width {D}")
    image = torch.empty(nbytes // 4, dtype=torch.float32, device=w_ih.device)
    entry = f"rslrl_{cell.name}_prepare_image{sfx}"
    rc = getattr(L, entry)(_ptr(w_ih), _ptr(w_hh), D, H, _ptr(image), ctypes.c_void_p(_stream(w_ih.device)))
    _lib.check(rc, entry)
    return image


def _cell_whh_t_image(cell, w_hh):
    H, name = _rnn_width(w_hh.shape[-1], 1), cell.name + "_whh_t_image"
    rows = cell.blocks * H
    _require_device(w_hh)
    w_hh = w_hh.detach()
    if w_hh.dtype != torch.float32 or tuple(w_hh.shape) != (rows, H) or not w_hh.is_contiguous():
        raise ValueError(f"{name}: contiguous fp32 W_hh [{rows}, {H}]")
    L = _lib.lib()
    wide = H == RNN_HIDDEN_WIDE
    nbytes = getattr(L, f"rslrl_{name}_bytes_h")(H) if wide else getattr(L, f"rslrl_{name}_bytes")()
    image = torch.empty(nbytes // 4, dtype=torch.float32, device=w_hh.device)
    entry = f"rslrl_{cell.name}_prepare_whh_t_image" + ("_h" if wide else "")
    rc = getattr(L, entry)(_ptr(w_hh), H, _ptr(image), ctypes.c_void_p(_stream(w_hh.device)))
    _lib.check(rc, entry)
    return image


# [M, H] tensors that one problem of a rollout step, a training step and a reverse step moves beside its input rows
# (the timer spans' byte counts)
_CELL_TENSORS = {"lstm": {"cell": 4, "cell_train": 8, "cell_bwd": 16}, "gru": {"cell": 2, "cell_train": 7, "cell_bwd": 15}}


def _cell_span(cell, op, name, M, dev, widths, n, H=LSTM_CELL_HIDDEN):
    """The timer span of one launch: the name and the algorithmic bytes and flops each wrapper has always stated."""
    tensors = n * _CELL_TENSORS[cell.name][op]
    if widths is None:
        return timer.span(f"{name}[M={M}]", dev, 4 * M * H * tensors, n * 2 * M * cell.blocks * H * H * 6)
    shape = f"M={M}" if n == 2 else f"M={M},D={widths[0]}"
    return timer.span(f"{name}[{shape}]", dev, 4 * M * (sum(widths) + tensors * H))


def _cell_launch(cell, op, structs, rows, forward=True):
    """One launch of rslrl_<kind>_<op> ("cell", "cell_train", "cell_bwd") on one problem, or of its `_pair` form on two
    of one row count, under the timer span of that name.  structs: the argument struct per problem; rows: per problem
    a tensor of M rows -- of a forward form the input x, whose width decides whether the `_anyd` twin takes the launch
    (the reverse forms do not read the input)."""
    pair = len(structs) == 2
    name = f"{cell.name}_{op}_pair" if pair else f"{cell.name}_{op}"
    M, dev = rows[0].shape[0], rows[0].device
    if pair and rows[1].shape[0] != M:
        raise ValueError(f"{name}: both problems need the same number of rows")
    widths = [x.shape[1] for x in rows] if forward else None
    H = getattr(structs[0], "cell", structs[0]).hidden  # the builders put the width of the state there
    if pair and getattr(structs[1], "cell", structs[1]).hidden != H:
        raise ValueError(f"{name}: both problems need the same hidden size")
    if H == RNN_HIDDEN_WIDE:  # the `_h` entry takes every input width
        entry = "rslrl_" + name + "_h"
    else:
        entry = "rslrl_" + name + "_anyd" if forward and _rnn_anyd(*widths) else "rslrl_" + name
    launch, stream = getattr(_lib.lib(), entry), ctypes.c_void_p(_stream(dev))
    # (disabled, every call outside bench.py's timed region, the span's name and figures are not even put together)
    with _cell_span(cell, op, name, M, dev, widths, len(structs), H) if timer.enabled else _NO_SPAN:
        if pair:
            rc = launch(ctypes.byref(structs[0]), ctypes.byref(structs[1]), M, stream)
        else:
            rc = launch(ctypes.byref(structs[0]), M, stream)
    _lib.check(rc, entry)


def _cell_step(cell, build, *problems):
    """The rollout step of one problem (x, state, image, b_ih, b_hh), or of two in one launch: per problem the output
    `build` (_lstm_args / _gru_args) allocated."""
    keep = []
    built = [build(*p, keep) for p in problems]
    _cell_launch(cell, "cell", [b[0] for b in built], [p[0] for p in problems])
    return [b[1] for b in built]


def _cell_pair(cell, op, build, args0, args1):
    """Two problems of "cell_train" or "cell_bwd" (dicts of `build`'s arguments) in one launch."""
    keep = []
    key, forward = ("x", True) if op == "cell_train" else ("dh", False)
    _cell_launch(cell, op, [build(**args0, keep=keep), build(**args1, keep=keep)], [args0[key], args1[key]], forward)


def lstm_image(w_ih: torch.Tensor, w_hh: torch.Tensor) -> torch.Tensor:
    """The cell's weight image of W_ih [4 H, D] and W_hh [4 H, H] (one launch); rebuild it when they change."""
    return _cell_image(LSTM, w_ih, w_hh)


def gru_image(w_ih: torch.Tensor, w_hh: torch.Tensor) -> torch.Tensor:
    """The cell's weight image of W_ih [3 H, D] and W_hh [3 H, H] (one launch); rebuild it when they change."""
    return _cell_image(GRU, w_ih, w_hh)


def lstm_whh_t_image(w_hh: torch.Tensor) -> torch.Tensor:
    """The backward's image of W_hh^T (W_hh [4 H, H]); rebuild it when W_hh changes."""
    return _cell_whh_t_image(LSTM, w_hh)


def gru_whh_t_image(w_hh: torch.Tensor) -> torch.Tensor:
    """The backward's image of W_hh^T (W_hh [3 H, H]); rebuild it when W_hh changes."""
    return _cell_whh_t_image(GRU, w_hh)


def _lstm_args(x, state, image, b_ih, b_hh, keep, out=None):
    h, c = state if state is not None else (None, None)
    _require_device(x, h, c, image, b_ih, b_hh)
    M, D = x.shape
    H = _rnn_width(b_ih.numel(), 4)
    ts = [x] + [t for t in (h, c) if t is not None]
    if any(t.dtype != torch.float32 for t in ts) or (h is None) != (c is None):
        raise ValueError(f"lstm_cell: fp32 x [M, D] and (h, c) [M, {H}] or no state")
    x = x if x.is_contiguous() else x.contiguous()
    if h is not None:
        h = h.reshape(M, H)
        c = c.reshape(M, H)
        h, c = (h if h.is_contiguous() else h.contiguous()), (c if c.is_contiguous() else c.contiguous())
    if out is None:  # (h', c'), or the caller's
        out = torch.empty(2, M, H, dtype=torch.float32, device=x.device)
    b_ih, b_hh = b_ih.detach(), b_hh.detach()
    keep += [x, h, c, b_ih, b_hh]
    a = _lib.LstmCell(x.data_ptr(), h.data_ptr() if h is not None else None, c.data_ptr() if c is not None else None,
                      image.data_ptr(), b_ih.data_ptr(), b_hh.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), D,
                      H, 1, 0)
    return a, out


def lstm_cell(x, state, image, b_ih, b_hh):
    """One LSTM step (include/rslrl_amd.h rslrl_lstm_cell): x [M, D], state (h, c) of [M, H] (or [1, M, H]) or
    None for zeros; returns (h', c') as [M, H] views of one buffer.  Raises on an unsupported shape."""
    (out,) = _cell_step(LSTM, _lstm_args, (x, state, image, b_ih, b_hh))
    return out[0], out[1]


def lstm_cell_pair(x0, state0, image0, b_ih0, b_hh0, x1, state1, image1, b_ih1, b_hh1):
    """Two LSTM steps of one M (the actor's and the critic's memories) in one launch: the bits of two lstm_cell
    calls.  Returns ((h0', c0'), (h1', c1'))."""
    o0, o1 = _cell_step(LSTM, _lstm_args, (x0, state0, image0, b_ih0, b_hh0), (x1, state1, image1, b_ih1, b_hh1))
    return (o0[0], o0[1]), (o1[0], o1[1])


def _gate_major(t, M, name, H=LSTM_CELL_HIDDEN):
    """(tensor, gate stride) of a gate-major fp32 tensor [4, ..., M, H] view whose gate blocks are [M, H] contiguous."""
    if t.dtype != torch.float32 or t.shape[0] != 4 or t[0].numel() != M * H or not t[0].is_contiguous():
        raise ValueError(f"{name}: gate-major fp32 [4, M, {H}] with contiguous gate blocks")
    return t, t.stride(0)


def _reset_vec(reset, M, name):
    if reset is None:
        return None
    if reset.dtype != torch.uint8 or reset.numel() != M or not reset.is_contiguous():
        raise ValueError(f"{name}: a contiguous uint8 [M] vector (the storage's dones)")
    return reset


def _state_rows(t, M, name, H=LSTM_CELL_HIDDEN):
    if t is None:
        return None
    if t.dtype != torch.float32 or t.numel() != M * H or not t.is_contiguous():
        raise ValueError(f"{name}: contiguous fp32 [M, {H}]")
    return t


def _lstm_train_args(x, state, image, b_ih, b_hh, reset, h_out, c_out, gates, h_restart=None, c_restart=None,
                     h_in_out=None, *, keep):
    M, H = x.shape[0], _rnn_width(b_ih.numel(), 4)
    _require_device(h_out, c_out, gates, reset, h_restart, c_restart, h_in_out)
    if not (h_out.is_contiguous() and c_out.is_contiguous() and h_out.dtype == c_out.dtype == torch.float32
            and h_out.numel() == c_out.numel() == M * H):
        raise ValueError(f"lstm_cell_train: contiguous fp32 h_out, c_out [M, {H}]")
    a, _ = _lstm_args(x, state, image, b_ih, b_hh, keep, out=(h_out, c_out))
    t = _lib.LstmTrain()
    t.cell = a
    gates, t.gate_stride = _gate_major(gates, M, "lstm_cell_train gates", H)
    t.gates = gates.data_ptr()
    reset = _reset_vec(reset, M, "lstm_cell_train reset")
    t.reset = reset.data_ptr() if reset is not None else None
    for field, v in (("h_restart", h_restart), ("c_restart", c_restart), ("h_in_out", h_in_out)):
        v = _state_rows(v, M, f"lstm_cell_train {field}", H)
        setattr(t, field, v.data_ptr() if v is not None else None)
    keep += [gates, reset, h_restart, c_restart, h_in_out]
    return t


def lstm_cell_train(x, state, image, b_ih, b_hh, reset, h_out, c_out, gates, h_restart=None, c_restart=None,
                    h_in_out=None):
    """The training form of lstm_cell (include/rslrl_amd.h rslrl_lstm_cell_train): rows whose `reset` (uint8 [M] or
    None) is set read their state as zero -- or from h_restart / c_restart [M, H] where given (ABI 27); writes h',
    c' [M, H] and the activated gates (gate-major [4, M, H], a view into a [4, steps, M, H] window buffer is
    fine) into the given tensors, and the h as consumed into h_in_out [M, H] where given."""
    keep = []
    t = _lstm_train_args(x, state, image, b_ih, b_hh, reset, h_out, c_out, gates, h_restart, c_restart, h_in_out,
                         keep=keep)
    _cell_launch(LSTM, "cell_train", [t], [x])
    return h_out, c_out, gates


def lstm_cell_train_pair(args0, args1):
    """Two lstm_cell_train problems of one M (the actor's and the critic's memories; D may differ) in one launch: the
    bits of the two single calls.  args0 / args1: dicts of lstm_cell_train's arguments."""
    _cell_pair(LSTM, "cell_train", _lstm_train_args, args0, args1)


def _lstm_bwd_args(dh, gates, c_out, c_prev, reset_cur, dg_next, dc_next, reset_next, whh_t_image, dg, dc_prev,
                   c_restart=None, *, keep):
    M = dh.shape[0]
    H = _rnn_width(dh.numel(), M)
    _require_device(dh, gates, c_out, c_prev, reset_cur, dg_next, dc_next, reset_next, whh_t_image, dg, dc_prev,
                    c_restart)
    for t in (dh, c_out, c_prev, dc_next, dc_prev, c_restart):
        if t is not None and not (t.dtype == torch.float32 and t.is_contiguous() and t.numel() == M * H):
            raise ValueError(f"lstm_cell_bwd: contiguous fp32 [M, {H}] operands")
    a = _lib.LstmBwd()
    a.hidden, a.layers = H, 1
    gates, a.gate_stride = _gate_major(gates, M, "lstm_cell_bwd gates", H)
    dg, stride = _gate_major(dg, M, "lstm_cell_bwd dg", H)
    if stride != a.gate_stride:
        raise ValueError("lstm_cell_bwd: gates and dg share one gate stride")
    a.dh, a.gates, a.c_out, a.dg, a.dc_prev = (dh.data_ptr(), gates.data_ptr(), c_out.data_ptr(), dg.data_ptr(),
                                              dc_prev.data_ptr())
    a.c_prev = c_prev.data_ptr() if c_prev is not None else None
    a.c_restart = c_restart.data_ptr() if c_restart is not None else None
    a.dc_next = dc_next.data_ptr() if dc_next is not None else None
    if dg_next is not None:
        dg_next, a.next_stride = _gate_major(dg_next, M, "lstm_cell_bwd dg_next", H)
        a.dg_next, a.whh_t_image = dg_next.data_ptr(), whh_t_image.data_ptr()
    reset_cur = _reset_vec(reset_cur, M, "lstm_cell_bwd reset_cur")
    reset_next = _reset_vec(reset_next, M, "lstm_cell_bwd reset_next")
    a.reset_cur = reset_cur.data_ptr() if reset_cur is not None else None
    a.reset_next = reset_next.data_ptr() if reset_next is not None else None
    keep += [dh, gates, c_out, c_prev, reset_cur, dg_next, dc_next, reset_next, whh_t_image, dg, dc_prev, c_restart]
    return a


def lstm_cell_bwd(dh, gates, c_out, c_prev, reset_cur, dg_next, dc_next, reset_next, whh_t_image, dg, dc_prev,
                  c_restart=None):
    """One reverse LSTM step (include/rslrl_amd.h rslrl_lstm_cell_bwd): from dh [M, H] of this step's output, the
    next step's gate gradient dg_next (gate-major) and dc_next or None, the reset vectors on either side, and this
    step's saved gates, c' and entering c -- writes this step's gate gradient dg (gate-major) and dc_prev.
    c_restart [M, H] (ABI 27): the entering c of the rows whose reset_cur is set (None: zero)."""
    a = _lstm_bwd_args(dh, gates, c_out, c_prev, reset_cur, dg_next, dc_next, reset_next, whh_t_image, dg, dc_prev,
                       c_restart, keep=[])
    _cell_launch(LSTM, "cell_bwd", [a], [dh], forward=False)
    return dg, dc_prev


def lstm_cell_bwd_pair(args0, args1):
    """Two lstm_cell_bwd problems of one M in one launch: the bits of the two single calls.  args0 / args1: dicts of
    lstm_cell_bwd's arguments."""
    _cell_pair(LSTM, "cell_bwd", _lstm_bwd_args, args0, args1)


def _gru_args(x, h, image, b_ih, b_hh, keep, out=None):
    _require_device(x, h, image, b_ih, b_hh)
    if x.dim() != 2 or x.dtype != torch.float32 or (h is not None and h.dtype != torch.float32):
        raise ValueError("gru_cell: fp32 x [M, D] and h [M, H] or no state")
    M, D = x.shape
    H = _rnn_width(b_ih.numel(), 3)
    x = x if x.is_contiguous() else x.contiguous()
    if h is not None:
        h = h.reshape(M, H)
        h = h if h.is_contiguous() else h.contiguous()
    if out is None:  # h', or the caller's
        out = torch.empty(M, H, dtype=torch.float32, device=x.device)
    b_ih, b_hh = b_ih.detach(), b_hh.detach()
    keep += [x, h, b_ih, b_hh, image, out]
    a = _lib.GruCell(x.data_ptr(), h.data_ptr() if h is not None else None, image.data_ptr(), b_ih.data_ptr(),
                     b_hh.data_ptr(), out.data_ptr(), D, H, 1, 0)
    return a, out


def gru_cell(x, h, image, b_ih, b_hh):
    """One GRU step (include/rslrl_amd.h rslrl_gru_cell): x [M, D], h [M, H] (or [1, M, H]) or None for zeros;
    returns h' [M, H].  Raises on an unsupported shape."""
    return _cell_step(GRU, _gru_args, (x, h, image, b_ih, b_hh))[0]


def gru_cell_pair(x0, h0, image0, b_ih0, b_hh0, x1, h1, image1, b_ih1, b_hh1):
    """Two GRU steps of one M (the actor's and the critic's memories) in one launch: the bits of two gru_cell calls.
    Returns (h0', h1')."""
    return tuple(_cell_step(GRU, _gru_args, (x0, h0, image0, b_ih0, b_hh0), (x1, h1, image1, b_ih1, b_hh1)))


def _gru_train_args(x, h, image, b_ih, b_hh, reset, h_out, gates, h_restart=None, h_in_out=None, *, keep):
    M, H = x.shape[0], _rnn_width(b_ih.numel(), 3)
    _require_device(h_out, gates, reset, h_restart, h_in_out)
    if not (h_out.is_contiguous() and h_out.dtype == torch.float32 and h_out.numel() == M * H):
        raise ValueError(f"gru_cell_train: contiguous fp32 h_out [M, {H}]")
    a, _ = _gru_args(x, h, image, b_ih, b_hh, keep, out=h_out)
    t = _lib.GruTrain()
    t.cell = a
    gates, t.gate_stride = _gate_major(gates, M, "gru_cell_train gates", H)
    t.gates = gates.data_ptr()
    reset = _reset_vec(reset, M, "gru_cell_train reset")
    t.reset = reset.data_ptr() if reset is not None else None
    for field, v in (("h_restart", h_restart), ("h_in_out", h_in_out)):
        v = _state_rows(v, M, f"gru_cell_train {field}", H)
        setattr(t, field, v.data_ptr() if v is not None else None)
    keep += [gates, reset, h_restart, h_in_out]
    return t


def gru_cell_train(x, h, image, b_ih, b_hh, reset, h_out, gates, h_restart=None, h_in_out=None):
    """The training form of gru_cell (include/rslrl_amd.h rslrl_gru_cell_train): rows whose `reset` (uint8 [M] or
    None) is set read their state from h_restart [M, H] (None: zero); writes h' [M, H] and r, z, n, a (gate-major
    [4, M, H], a view into a [4, steps, M, H] buffer is fine) into the given tensors, and the h as consumed into
    h_in_out [M, H] where given."""
    keep = []
    t = _gru_train_args(x, h, image, b_ih, b_hh, reset, h_out, gates, h_restart, h_in_out, keep=keep)
    _cell_launch(GRU, "cell_train", [t], [x])
    return h_out, gates


def gru_cell_train_pair(args0, args1):
    """Two gru_cell_train problems of one M (the actor's and the critic's memories; D may differ) in one launch: the
    bits of the two single calls.  args0 / args1: dicts of gru_cell_train's arguments."""
    _cell_pair(GRU, "cell_train", _gru_train_args, args0, args1)


def _gru_bwd_args(dh, gates, h_in, dg_next, dhz_next, reset_next, whh_t_image, dg, dhz_out, *, keep):
    M = dh.shape[0]
    H = _rnn_width(dh.numel(), M)
    _require_device(dh, gates, h_in, dg_next, dhz_next, reset_next, whh_t_image, dg, dhz_out)
    for t in (dh, h_in, dhz_next, dhz_out):
        if t is not None and not (t.dtype == torch.float32 and t.is_contiguous() and t.numel() == M * H):
            raise ValueError(f"gru_cell_bwd: contiguous fp32 [M, {H}] operands")
    a = _lib.GruBwd()
    a.hidden, a.layers = H, 1
    gates, a.gate_stride = _gate_major(gates, M, "gru_cell_bwd gates", H)
    dg, stride = _gate_major(dg, M, "gru_cell_bwd dg", H)
    if stride != a.gate_stride:
        raise ValueError("gru_cell_bwd: gates and dg share one gate stride")
    a.dh, a.gates, a.h_in, a.dg, a.dhz_out = (dh.data_ptr(), gates.data_ptr(), h_in.data_ptr(), dg.data_ptr(),
                                              dhz_out.data_ptr())
    a.dhz_next = dhz_next.data_ptr() if dhz_next is not None else None
    if dg_next is not None:
        dg_next, a.next_stride = _gate_major(dg_next, M, "gru_cell_bwd dg_next", H)
        a.dg_next, a.whh_t_image = dg_next.data_ptr(), whh_t_image.data_ptr()
    reset_next = _reset_vec(reset_next, M, "gru_cell_bwd reset_next")
    a.reset_next = reset_next.data_ptr() if reset_next is not None else None
    keep += [dh, gates, h_in, dg_next, dhz_next, reset_next, whh_t_image, dg, dhz_out]
    return a


def gru_cell_bwd(dh, gates, h_in, dg_next, dhz_next, reset_next, whh_t_image, dg, dhz_out):
    """One reverse GRU step (include/rslrl_amd.h rslrl_gru_cell_bwd): from dh [M, H] of this step's output, the next
    step's gate gradient dg_next (gate-major r, z, n, a; None: the last step of a chain) with its carry dhz_next, the
    reset vector between the two steps, and this step's saved gates and h as consumed -- writes this step's gate
    gradient dg (gate-major) and the carry dhz_out = dh~ z (may be dhz_next)."""
    a = _gru_bwd_args(dh, gates, h_in, dg_next, dhz_next, reset_next, whh_t_image, dg, dhz_out, keep=[])
    _cell_launch(GRU, "cell_bwd", [a], [dh], forward=False)
    return dg, dhz_out


def gru_cell_bwd_pair(args0, args1):
    """Two gru_cell_bwd problems of one M in one launch: the bits of the two single calls.  args0 / args1: dicts of
    gru_cell_bwd's arguments."""
    _cell_pair(GRU, "cell_bwd", _gru_bwd_args, args0, args1)


# The operands of one training step and of its reverse step, per kind.  The callers that walk a sequence (the recurrent
# PPO update, the distillation window) record each step of the forward in the terms both kinds share and hand the record
# to the backward:
#     step = (state entering, state leaving, reset vector or None, restart states or None, the h as consumed)
# with states as tuples of n_state [M, H] tensors and None for "none"; `carry_*` is the gradient that travels beside dG
# (an LSTM's d c, a GRU's dh~ z).  These four functions name what the kind's wrapper reads of that.
def _lstm_train_operands(x, image, b_ih, b_hh, gates, step, h_in_out):
    state, out, reset, restart, _ = step
    return dict(x=x, state=state, image=image, b_ih=b_ih, b_hh=b_hh, reset=reset, h_out=out[0], c_out=out[1],
                gates=gates, h_restart=restart[0] if restart else None, c_restart=restart[1] if restart else None,
                h_in_out=h_in_out)


def _gru_train_operands(x, image, b_ih, b_hh, gates, step, h_in_out):
    state, out, reset, restart, _ = step
    return dict(x=x, h=state[0] if state else None, image=image, b_ih=b_ih, b_hh=b_hh, reset=reset, h_out=out[0],
                gates=gates, h_restart=restart[0] if restart else None, h_in_out=h_in_out)


def _lstm_bwd_operands(dh, gates, step, dg_next, carry_next, reset_next, whh_t_image, dg, carry_out):
    state, out, reset, restart, _ = step  # the reverse step reads the c on both sides of the step, not the h
    return dict(dh=dh, gates=gates, c_out=out[1], c_prev=state[1] if state else None, reset_cur=reset,
                dg_next=dg_next, dc_next=carry_next, reset_next=reset_next, whh_t_image=whh_t_image, dg=dg,
                dc_prev=carry_out, c_restart=restart[1] if restart else None)


def _gru_bwd_operands(dh, gates, step, dg_next, carry_next, reset_next, whh_t_image, dg, carry_out):
    # (the h as consumed already holds this step's reset and restart)
    return dict(dh=dh, gates=gates, h_in=step[4], dg_next=dg_next, dhz_next=carry_next, reset_next=reset_next,
                whh_t_image=whh_t_image, dg=dg, dhz_out=carry_out)


@dataclasses.dataclass(frozen=True)
class Cell:
    """The kind of a fused cell, as far as the callers of this section branch on it: LSTM and
    GRU below are the two instances.  Here a state is always a tuple of n_state tensors -- (h, c) or (h,), each
    [M, 256] --, or None for zeros.  Every method goes through this module's function of that name, looked up when it is
    called (kernels.lstm_cell_train, ...), so replacing one of those replaces it here too."""
    name: str  # "lstm" / "gru"
    blocks: int  # gate blocks of the weights: i, f, g, o / r, z, n
    n_state: int
    knob: str  # the environment variable that, set to 0, keeps the RNN library for this kind
    window_hin_from_cell: bool  # the distillation window takes the h as consumed from the cell (else: built on the host)
    train_operands: Callable  # (x, image, b_ih, b_hh, gates, step, h_in_out) -> train's operands (_lstm_train_operands)
    bwd_operands: Callable  # (dh, gates, step, dg_next, carry_next, reset_next, whh_t_image, dg, carry_out) -> bwd's

    def _fn(self, what):
        return globals()[f"{self.name}_{what}"]

    def enabled(self) -> bool:
        return os.environ.get(self.knob, "1") != "0"

    def supported(self, M: int, D: int, hidden: int, layers: int = 1) -> bool:
        """lstm_cell_anyd_supported / gru_cell_anyd_supported: one predicate, the GRU cell takes the LSTM cell's shapes."""
        return lstm_cell_anyd_supported(M, D, hidden, layers)

    def takes(self, M: int, D: int, hidden: int, layers: int = 1) -> bool:
        """The shapes the wrappers below launch: `supported`'s, and with the `_h` forms on (RSLRL_RNN_HIDDEN_512, on by
        default) those of hidden size 512 (lstm_cell_h_supported).  What Memory and the recurrent PPO update ask;
        `supported` stays the predicate of the paths that are built for hidden size 256 only (the distillation
        window)."""
        return self.supported(M, D, hidden, layers) or (_RNN_HIDDEN_512 and lstm_cell_h_supported(M, D, hidden, layers))

    def unpack(self, hidden):
        """Memory.hidden_states -- (h, c), or the bare h (a 1-tuple is taken too) -- as a state tuple; None stays."""
        if hidden is None:
            return None
        return tuple(hidden) if isinstance(hidden, (tuple, list)) else (hidden,)

    def pack(self, state):
        """A state tuple in Memory.hidden_states' form: (h, c), or the bare h."""
        return tuple(state) if self.n_state == 2 else state[0]

    def image(self, w_ih, w_hh):
        return self._fn("image")(w_ih, w_hh)

    def whh_t_image(self, w_hh):
        return self._fn("whh_t_image")(w_hh)

    def step(self, x, state, image, b_ih, b_hh):
        """One rollout step: the new state tuple."""
        bare = self.n_state == 1
        out = self._fn("cell")(x, state[0] if bare and state else state, image, b_ih, b_hh)
        return (out,) if bare else out

    def step_pair(self, x0, state0, image0, b_ih0, b_hh0, x1, state1, image1, b_ih1, b_hh1):
        """Two rollout steps of one M in one launch: the two new state tuples."""
        bare = self.n_state == 1
        o0, o1 = self._fn("cell_pair")(x0, state0[0] if bare and state0 else state0, image0, b_ih0, b_hh0,
                                       x1, state1[0] if bare and state1 else state1, image1, b_ih1, b_hh1)
        return ((o0,), (o1,)) if bare else (o0, o1)

    def train(self, operands):
        """One training step; `operands` from train_operands (a dict in the wrapper's argument order: the call is
        positional, as callers of kernels.lstm_cell_train / gru_cell_train have always made it)."""
        self._fn("cell_train")(*operands.values())

    def train_pair(self, operands0, operands1):
        self._fn("cell_train_pair")(operands0, operands1)

    def bwd(self, operands):
        """One reverse step; `operands` from bwd_operands (positional, as train)."""
        self._fn("cell_bwd")(*operands.values())

    def bwd_pair(self, operands0, operands1):
        self._fn("cell_bwd_pair")(operands0, operands1)


LSTM = Cell("lstm", 4, 2, "RSLRL_LSTM_CELL", False, _lstm_train_operands, _lstm_bwd_operands)
GRU = Cell("gru", 3, 1, "RSLRL_GRU_CELL", True, _gru_train_operands, _gru_bwd_operands)


_CELLS = {torch.nn.LSTM: LSTM, torch.nn.GRU: GRU}


def cell_of(rnn) -> Cell | None:
    """The Cell of exactly an nn.LSTM or an nn.GRU, None for anything else (a subclass included)."""
    return _CELLS.get(type(rnn))
