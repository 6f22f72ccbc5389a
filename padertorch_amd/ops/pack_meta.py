"""Batch layouts: the tables the recurrence kernels and ``ops.lstm._LstmLayerFn`` read of one batch of sequences.

Contract - every layout is a :class:`Layout` and carries

* ``T``, ``max_batch``, ``rows``: time steps, rows of the first step, packed rows in all; ``key``: what it was made from;
* ``bs_host`` / ``offs_host`` (numpy int32 / int64 ``[T]``) and ``bs_dev`` / ``offs_dev``: rows of, and first packed row of, every step;
* ``bs0`` and ``equal_lengths``: every step has ``bs0`` rows of the SAME sequences (``h_{t-1}`` is then a shifted view);
* ``masks_dev``: per-step (alive, first, last) row masks of a row-slot grid, ``None`` for a PackedSequence batch;
* ``prev_dev`` ``[2, rows]``: predecessor row per direction (``rows``: none); ``prev_h0_dev``: the same with "none" pointing at
  row ``rows + 1 + b`` (= ``h0[b]``); ``first_rows`` / ``last_rows`` ``[2, max_batch]``; ``padded_rows`` (``ops.sequence``) -
  the last four ``None`` for row-slot grids, which take no initial states;
* :attr:`Layout.uniform_rows`.

:class:`_PackMeta` is the layout of a ``PackedSequence``; ``ops.sequence.slots`` has the two row-slot grids.
"""
import functools

import numpy as np
import torch

from .. import _lib


class Layout:
    masks_dev = None

    @property
    def uniform_rows(self):
        """The packed rows are ``[T, batch]`` with ``batch`` a multiple of 16: the recurrences' hand-off planes are GEMM operands as
        they lie (a row-slot grid's too: its kernels write zeros for the idle slot steps)."""
        return (self.equal_lengths or self.masks_dev is not None) and self.bs0 % 16 == 0

    def _set_uniform_grid(self, T, S, device):
        """The fields of a ``[T, S]`` grid whose rows belong to DIFFERENT sequences over time (row slots): no shifted-view shortcut,
        no initial / final states."""
        self.T, self.max_batch, self.rows = T, S, T * S
        self.bs_host = np.full(T, S, dtype=np.int32)
        self.offs_host = (np.arange(T, dtype=np.int64) * S)
        self.bs_dev = _lib.host_to_device(self.bs_host, torch.int32, device)
        self.offs_dev = _lib.host_to_device(self.offs_host, torch.int64, device)
        self.bs0 = S
        self.equal_lengths = False
        self.first_rows = self.last_rows = self.prev_h0_dev = self.padded_rows = None


class _PackMeta(Layout):
    """Device-side bookkeeping of one ``batch_sizes`` vector (cached: batches repeat shapes)."""

    def __init__(self, batch_sizes, device):
        self.key = tuple(batch_sizes)
        bs = np.asarray(batch_sizes, dtype=np.int64)
        assert np.all(bs[:-1] >= bs[1:]), 'batch_sizes must be non-increasing (sorted sequences)'
        self.T = int(len(bs))
        self.max_batch = int(bs[0]) if self.T else 0
        offs = np.concatenate([[0], np.cumsum(bs)])
        self.rows = int(offs[-1])
        # host-side copies: the C ABI turns them into per-launch kernel arguments
        self.bs_host = np.ascontiguousarray(bs, dtype=np.int32)
        self.offs_host = np.ascontiguousarray(offs[:-1], dtype=np.int64)
        # device copies for the persistent kernels (read in-kernel, step by step)
        self.bs_dev = _lib.host_to_device(self.bs_host, torch.int32, device)          # (no host synchronisation: _lib.host_to_device)
        self.offs_dev = _lib.host_to_device(self.offs_host, torch.int64, device)
        # index of the predecessor row (forward sense) per direction; `rows` = "no predecessor"
        # (vectorised: a new length pattern every step - real training data - must not cost the host milliseconds)
        t_row = np.repeat(np.arange(self.T), bs)                      # time step / batch index of every packed row
        b_row = np.arange(self.rows) - offs[t_row] if self.T else np.zeros(0, np.int64)
        bs_next = np.append(bs[1:], 0) if self.T else bs
        prev = np.full((2, self.rows), self.rows, dtype=np.int64)
        if self.T:
            prev[0] = np.where(t_row > 0, offs[np.maximum(t_row - 1, 0)] + b_row, self.rows)
            prev[1] = np.where(b_row < bs_next[t_row], offs[t_row + 1] + b_row, self.rows)
        self.prev_dev = _lib.host_to_device(prev, torch.int64, device)
        # equal-length batch: the predecessor of packed row r is row r - bs[0] (forward direction) or
        # r + bs[0] (reverse direction), which `_LstmLayerFn` turns into shifted views of a padded buffer
        self.bs0 = int(bs[0]) if self.T else 0
        self.equal_lengths = bool(self.T and (bs == bs[0]).all())
        # per sequence b: rows of its first / last processed step per direction (initial / final states),
        # and the predecessor table with "no predecessor" pointing at row rows + 1 + b (= h0[b])
        lens = (bs[None, :] > np.arange(self.max_batch)[:, None]).sum(1) if self.T else np.zeros(0, np.int64)
        b_idx = np.arange(self.max_batch)
        end_rows = offs[np.maximum(lens - 1, 0)] + b_idx
        self.first_rows = _lib.host_to_device(np.stack([b_idx, end_rows]), torch.int64, device)
        self.last_rows = _lib.host_to_device(np.stack([end_rows, b_idx]), torch.int64, device)
        prev_h0 = prev.copy()
        row_b = b_row
        for d in range(2):
            fresh = prev[d] == self.rows
            prev_h0[d, fresh] = self.rows + 1 + row_b[fresh]
        self.prev_h0_dev = _lib.host_to_device(prev_h0, torch.int64, device)
        # packed row (t, b) -> row t * max_batch + b of the time-major padded tensor (ops.sequence.unpack_sequence)
        self.padded_rows = _lib.host_to_device(t_row * self.max_batch + b_row, torch.int64, device)


@functools.lru_cache(maxsize=64)
def _meta(batch_sizes_key, device_key):
    return _PackMeta(batch_sizes_key, torch.device(*device_key))


def pack_meta(batch_sizes, device):
    return _meta(tuple(int(b) for b in batch_sizes.tolist()), (device.type, device.index))
